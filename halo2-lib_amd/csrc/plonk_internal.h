// What the prover's translation units share: the constraint-system shape (plonk_shape.h, which the verifier reads too), the evaluation
// domain, the proving key with its buffer pool, and (transcript.h) the transcript interface.  plonk.hip: keygen, sharding set-up, the C entry
// points.  plonk_prove.hip: one proof (ProofRun) and SHPLONK's bookkeeping.
#pragma once
#include <algorithm>
#include <chrono>
#include <map>
#include <vector>

#include "blake2b.h"
#include "host_field.h"
#include "internal.h"
#include "plonk_shape.h"
#include "transcript.h"

namespace h2 {
namespace plonk {

struct Domain {
    Fr omega, omega_inv, ext_omega, ext_omega_inv, zeta, zeta_inv, ifft_divisor, ext_ifft_divisor, delta;
    void init(uint32_t k, uint32_t ek) {
        ext_omega = fr_from_canonical_u64x4(ROOT_OF_UNITY);
        for (uint32_t i = ek; i < 28; ++i) ext_omega = fe_sqr(ext_omega);
        omega = ext_omega;
        for (uint32_t i = k; i < ek; ++i) omega = fe_sqr(omega);
        omega_inv = fe_inv(omega);
        ext_omega_inv = fe_inv(ext_omega);
        zeta = fr_from_canonical_u64x4(ZETA);
        zeta_inv = fe_sqr(zeta);
        ifft_divisor = fe_inv(fr_from_u64((uint64_t)1 << k));
        ext_ifft_divisor = fe_inv(fr_from_u64((uint64_t)1 << ek));
        delta = fr_from_canonical_u64x4(DELTA);
    }
};

// ---------------------------------------------------------------------------------------------- device buffers
// size-keyed pool: a proof's buffers go back to the key's pool when it is done, so a second proof allocates nothing
struct BufPool {
    std::multimap<size_t, void *> free_;
    std::vector<void *> all_;
    int take(size_t bytes, void **out) {
        auto it = free_.find(bytes);
        if (it != free_.end()) {
            *out = it->second;
            free_.erase(it);
            return H2HIP_OK;
        }
        hipError_t e = hipMalloc(out, bytes ? bytes : 256);
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
            return H2HIP_ERR_NOMEM;
        }
        all_.push_back(*out);
        return H2HIP_OK;
    }
    void give(size_t bytes, void *p) { free_.insert({bytes, p}); }
    void destroy() {
        for (void *p : all_) hipFree(p);
        all_.clear();
        free_.clear();
    }
};
// buffers taken during one call; returned to the pool on scope exit (also on the error paths)
struct Scope {
    BufPool *pool;
    std::vector<std::pair<size_t, void *>> held;
    explicit Scope(BufPool *p) : pool(p) {}
    ~Scope() {
        for (auto &h : held) pool->give(h.first, h.second);
    }
    int take(size_t elems, Fr **out) {
        void *p = nullptr;
        H2_CHK(pool->take(sizeof(Fr) * elems, &p));
        held.push_back({sizeof(Fr) * elems, p});
        *out = (Fr *)p;
        return H2HIP_OK;
    }
    void release(Fr *p) {   // early return of one buffer
        for (size_t i = 0; i < held.size(); ++i)
            if (held[i].second == (void *)p) {
                pool->give(held[i].first, held[i].second);
                held.erase(held.begin() + (long)i);
                return;
            }
    }
};

static inline G1Affine jacobian_to_affine(const G1Jac &p) {
    G1Affine r;
    if (p.z.is_zero()) {
        r.x = Fq::zero();
        r.y = Fq::zero();
        return r;
    }
    const Fq zi = fe_inv(p.z), zi2 = fe_sqr(zi);
    r.x = fe_mul(p.x, zi2);
    r.y = fe_mul(p.y, fe_mul(zi2, zi));
    return r;
}

// plonk_prove.hip: one proof.  Nothing of the run stays on the context: its callbacks into the batch MSM are arguments of the commitment calls.
// `tr`: the built-in Blake2b transcript (the caller takes its bytes) or the adapter over the caller's callbacks.
int create_proof_impl(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, bool advice_on_device, const void *const *instances,
                      const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user, ProverTranscript &tr, double *stage_ms,
                      const h2hip_phase_witness *witness = nullptr);

}  // namespace plonk
}  // namespace h2

using namespace h2;   // (an internal header of two translation units that both live in these namespaces)
using namespace h2::plonk;

struct h2hip_plonk_pk {
    Shape sh;
    Domain dom;
    h2hip_ctx *ctx = nullptr;
    const h2hip_bases *g = nullptr, *g_lagrange = nullptr;
    std::vector<Fr *> fixed_values, fixed_polys, fixed_cosets, sigma_values, sigma_polys, sigma_cosets;
    Fr *l0 = nullptr, *l_last = nullptr, *l_blind = nullptr;   // extended-domain evaluations
    void *table_sorted = nullptr;                               // sorted keys of the lookup table column (prepared once: the table is fixed)
    std::vector<G1Affine> fixed_commitments, permutation_commitments;
    Fr transcript_repr;
    bool have_repr = false;
    BufPool pool;
    std::vector<void *> owned;
    // multi-GPU (h2hip_plonk_pk_set_sharding): point-range sharding of every commitment, coset sharding of h(X)'s numerator
    const h2hip_bases *g_shard = nullptr, *g_lagrange_shard = nullptr;
    size_t shard_offset = 0, shard_len = 0;
    uint32_t shard_world = 1, shard_rank = 0;
    h2hip_comm *comm = nullptr;
    bool shard_quotient = false, shard_products = false, shard_ntt = false;
    std::vector<uint32_t> my_cosets;          // cosets of the extended domain (rows = coset mod 2^(ek-k)) this rank evaluates h(X) on
    uint32_t max_cosets = 1;                  // cosets of the busiest rank (the all-gather's uniform slot count)
    std::vector<Fr *> fixed_cosets_sh, sigma_cosets_sh;   // [my_cosets][n] slices of the key's extended-domain arrays
    Fr *l0_sh = nullptr, *l_last_sh = nullptr, *l_blind_sh = nullptr;
    std::vector<void *> shard_owned;
    // exchanges of the running sharded proof: every host exchange carries a status word, so that a rank that fails between two
    // exchanges can tell its peers (it takes part in the NEXT exchange with an error status and a zero payload of the scheduled size)
    std::vector<size_t> exch_sizes;
    size_t exch_next = 0;
    hipStream_t copy_stream = nullptr;   // the RNG-drawn random polynomial is uploaded on its own stream, next to the NTTs
    hipEvent_t copy_ev = nullptr;
    h2hip_ctx *side = nullptr;           // child context (own stream, NTT scratch and twiddle cache): the transforms that run next to an MSM's tail
    hipEvent_t side_ev = nullptr, side_ev1 = nullptr;   // side_ev: everything queued on the side stream so far; side_ev1: the first-round columns' transforms
    Fr *host_stage = nullptr;   // pinned staging for the RNG-drawn scalars (the n coefficients of the random polynomial, the blinding rows)
    size_t host_stage_elems = 0;
    // the copy cycles for h2hip_plonk_check_witness: sigma(c, r) = (sigma_c, sigma_r)[c * usable_rows + r] over the usable rows (copies stay in
    // them, so every other cell maps to itself).  Kept on the host; uploaded by the first check into buffers the key owns.
    std::vector<uint16_t> sigma_c_host;
    std::vector<uint32_t> sigma_r_host;
    uint16_t *sigma_c_dev = nullptr;
    uint32_t *sigma_r_dev = nullptr;
};
