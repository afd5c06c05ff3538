// What the prover's translation units share: the constraint-system shape, the evaluation domain, the proving key with its buffer pool,
// and (transcript.h) the transcript interface.  plonk.hip: shape construction's callers, keygen, sharding set-up, the C entry points.  plonk_prove.hip: one
// proof (ProofRun) and SHPLONK's bookkeeping.
#pragma once
#include <algorithm>
#include <chrono>
#include <map>
#include <vector>

#include "blake2b.h"
#include "host_field.h"
#include "internal.h"
#include "transcript.h"

namespace h2 {
namespace plonk {

static const uint64_t ROOT_OF_UNITY[4] = {0xd34f1ed960c37c9cULL, 0x3215cf6dd39329c8ULL, 0x98865ea93dd31f74ULL, 0x03ddb9f5166d18b7ULL};   // 7^((r-1)/2^28)
static const uint64_t ZETA[4] = {0xb8ca0b2d36636f23ULL, 0xcc37a73fec2bc5e9ULL, 0x048b6e193fd84104ULL, 0x30644e72e131a029ULL};            // 7^(2(r-1)/3)
static const uint64_t DELTA[4] = {0x870e56bbe533e9a2ULL, 0x5b5f898e5e963f25ULL, 0x64ec26aad4c86e71ULL, 0x09226b6e22c6f0caULL};           // 7^(2^28)

// ---------------------------------------------------------------------------------------------- constraint-system shape
struct ColumnRef {
    int kind;   // 0 = fixed, 1 = advice, 2 = instance
    int index;
};
struct Lookup {
    int q_col;   // fixed column of the complex selector, or -1
    int advice_col, table_col;
    std::vector<ColumnRef> in, tab;   // dynamic lookups (q_col = advice_col = table_col = -1): the expressions compressed by theta
};
struct Shape {
    h2hip_base_circuit_params p;
    uint32_t k, n;
    bool with_range, single;
    bool dyn = false;              // BasicDynLookupConfig + FlexGateConfig (init_dyn); otherwise BaseConfig (init)
    uint32_t key_cols = 0;         // dyn: KEY_COL; lookup expressions have key_cols + 1 columns
    uint32_t first_gate_advice = 0;   // advice index of gate column 0 (dyn: behind the table and key columns)
    bool from_phased = false;      // made by init_phased (h2hip_plonk_keygen_phased)
    bool phased = false;           // multi-phase BaseConfig (init_phased) with more than one used phase or a challenge
    std::vector<std::vector<int>> phase_cols;   // phased: the advice columns of every used phase, index order (gate, then lookup advice)
    uint32_t phase_challenges[H2HIP_MAX_PHASE] = {0, 0, 0};   // phased: challenges squeezed after each phase's commitments
    uint32_t num_rlc = 0;          // RLC columns (init_rlc): phase-1 advice columns behind every BaseConfig column, gate q_rlc * (a0 * gamma + a1 - a2)
    uint32_t first_rlc_advice = 0; // advice index of RLC column 0
    int first_q_rlc_col = -1;      // fixed column of RLC column 0's selector
    int table_col = -1, q_lookup_col = -1, first_constant_col = -1, first_q_enable_col = -1;
    uint32_t num_advice_total, num_fixed_total;
    std::vector<Lookup> lookups;
    std::vector<ColumnRef> perm_columns;
    std::vector<std::pair<int, int>> advice_queries, fixed_queries;   // (column, rotation) in first-query order
    uint32_t degree, blinding_factors, usable_rows, chunk_len, quotient_pieces, extended_k, num_perm_sets;

    int init(const h2hip_base_circuit_params &bp) {
        p = bp;
        k = bp.k;
        H2_REQUIRE(k >= 4 && k <= 26, "k out of range (4..26)");
        // the reference's configurations go up to 291 gate + 53 lookup advice columns (halo2-ecc/configs/secp256k1/bench_ecdsa.config:9)
        H2_REQUIRE(bp.num_advice >= 1 && bp.num_advice <= 1024 && bp.num_lookup_advice <= 256 && bp.num_fixed <= 16 && bp.num_instance <= 8,
                   "column counts out of range");
        H2_REQUIRE(bp.lookup_bits < (int32_t)k, "lookup_bits must be less than k");
        const bool range = bp.lookup_bits >= 0 && bp.num_lookup_advice != 0;
        const bool q_lookup = range && bp.num_advice == 1;   // range/mod.rs:93-95: the lookup sits on the gate column behind a complex selector
        return layout(bp, range, q_lookup, (q_lookup || !range) ? 0 : bp.num_lookup_advice);
    }
    // the columns, lookups and queries of FlexGateConfig + RangeConfig: bp.num_advice gate columns, `nla` dedicated lookup-advice columns,
    // the table iff `range`, the complex selector q_lookup on gate column 0 iff `q_lookup`
    int layout(const h2hip_base_circuit_params &bp, bool range, bool q_lookup, uint32_t nla) {
        n = 1u << k;
        with_range = range;
        single = q_lookup;
        int nf = 0;
        if (with_range) table_col = nf++;            // meta.lookup_table_column() is created first (range/mod.rs:82)
        first_constant_col = bp.num_fixed ? nf : -1;
        nf += (int)bp.num_fixed;                     // flex_gate/mod.rs:123-129
        // selectors are compressed into fixed columns after the circuit's own ones: the complex selector keeps a column of its own, and
        // the per-column gate selectors are enabled on common rows, so none of them can share a column either [UPSTREAM compress_selectors]
        if (single) q_lookup_col = nf++;
        first_q_enable_col = nf;
        nf += (int)bp.num_advice;
        if (num_rlc) first_q_rlc_col = nf;   // the RLC selectors are created after BaseConfig's
        nf += (int)num_rlc;
        num_fixed_total = (uint32_t)nf;
        first_rlc_advice = bp.num_advice + nla;
        num_advice_total = bp.num_advice + nla + num_rlc;
        if (single) lookups.push_back({q_lookup_col, 0, table_col});
        for (uint32_t i = 0; i < nla; ++i) lookups.push_back({-1, (int)(bp.num_advice + i), table_col});
        // enable_equality order: constants, gate advice, lookup advice, instance
        for (uint32_t i = 0; i < bp.num_fixed; ++i) perm_columns.push_back({0, first_constant_col + (int)i});
        for (uint32_t i = 0; i < first_rlc_advice; ++i) perm_columns.push_back({1, (int)i});
        for (uint32_t i = 0; i < bp.num_instance; ++i) perm_columns.push_back({2, (int)i});
        for (uint32_t i = 0; i < num_rlc; ++i) perm_columns.push_back({1, (int)(first_rlc_advice + i)});   // enable_equality is called on them last
        for (uint32_t a = 0; a < bp.num_advice; ++a)
            for (int r = 0; r < 4; ++r) advice_queries.push_back({(int)a, r});
        for (uint32_t i = 0; i < nla; ++i) advice_queries.push_back({(int)(bp.num_advice + i), 0});
        for (uint32_t i = 0; i < num_rlc; ++i)
            for (int r = 0; r < 3; ++r) advice_queries.push_back({(int)(first_rlc_advice + i), r});
        for (uint32_t i = 0; i < bp.num_fixed; ++i) fixed_queries.push_back({first_constant_col + (int)i, 0});
        if (with_range) fixed_queries.push_back({table_col, 0});
        if (single) fixed_queries.push_back({q_lookup_col, 0});
        for (uint32_t i = 0; i < bp.num_advice; ++i) fixed_queries.push_back({first_q_enable_col + (int)i, 0});
        for (uint32_t i = 0; i < num_rlc; ++i) fixed_queries.push_back({first_q_rlc_col + (int)i, 0});
        degree = 3;   // gate and permutation argument; the RLC gate is selector * degree 2 as well
        for (const Lookup &l : lookups) degree = std::max<uint32_t>(degree, std::max<uint32_t>(4, 2 + (l.q_col >= 0 ? 2 : 1) + 1));
        blinding_factors = std::max<uint32_t>(3, 4) + 2;   // a gate column is queried at four rotations (an RLC column at three)
        H2_REQUIRE(n > blinding_factors + 8, "k too small for the blinding rows");
        usable_rows = n - (blinding_factors + 1);
        chunk_len = degree - 2;
        quotient_pieces = degree - 1;
        extended_k = k;
        while (((uint64_t)1 << extended_k) < (uint64_t)n * quotient_pieces) ++extended_k;
        H2_REQUIRE(extended_k <= 28, "extended domain exceeds the 2-adicity of F_r");
        num_perm_sets = (uint32_t)((perm_columns.size() + chunk_len - 1) / chunk_len);
        // range/mod.rs:117-121: the table must fit gate.max_rows = 2^k - meta.minimum_rows() = n - (blinding_factors + 3)
        if (bp.lookup_bits >= 0 && with_range) H2_REQUIRE(((uint64_t)1 << bp.lookup_bits) <= n - (blinding_factors + 3), "lookup table is too large for the circuit degree plus blinding factors");
        return H2HIP_OK;
    }
    // BasicDynLookupConfig::new(meta, || FirstPhase, lu_sets) then FlexGateConfig::configure (memory.rs:92-98); include/h2hip.h states the layout
    int init_dyn(const h2hip_dyn_circuit_params &dp) {
        H2_REQUIRE(dp.k >= 4 && dp.k <= 26, "k out of range (4..26)");
        H2_REQUIRE(dp.key_cols >= 1 && dp.key_cols <= 4, "key_cols out of range (1..4)");
        H2_REQUIRE(dp.lu_sets >= 1 && dp.lu_sets <= 48, "lu_sets out of range (1..48)");
        H2_REQUIRE(dp.num_advice >= 1 && dp.num_advice <= 1024 && dp.num_fixed <= 16, "column counts out of range");
        p = h2hip_base_circuit_params{dp.k, dp.num_advice, 0, dp.num_fixed, 0, -1};
        k = dp.k;
        n = 1u << k;
        dyn = true;
        with_range = single = false;
        key_cols = dp.key_cols;
        const uint32_t m = dp.key_cols, L = dp.lu_sets, ndyn = m * (1 + L);
        first_gate_advice = ndyn;
        num_advice_total = ndyn + dp.num_advice;
        first_constant_col = dp.num_fixed ? (int)(1 + L) : -1;
        first_q_enable_col = (int)(1 + L + dp.num_fixed);
        num_fixed_total = 1 + L + dp.num_fixed + dp.num_advice;
        for (uint32_t s = 0; s < L; ++s) {
            Lookup l{-1, -1, -1, {}, {}};
            for (uint32_t j = 0; j < m; ++j) {
                l.in.push_back({1, (int)(m * (1 + s) + j)});
                l.tab.push_back({1, (int)j});
            }
            l.in.push_back({0, (int)(1 + s)});   // key_is_enabled of the set
            l.tab.push_back({0, 0});             // table_is_enabled
            lookups.push_back(l);
        }
        for (uint32_t c = 0; c < ndyn; ++c) perm_columns.push_back({1, (int)c});
        for (uint32_t i = 0; i < dp.num_fixed; ++i) perm_columns.push_back({0, first_constant_col + (int)i});
        for (uint32_t a = 0; a < dp.num_advice; ++a) perm_columns.push_back({1, (int)(ndyn + a)});
        for (uint32_t c = 0; c < ndyn; ++c) advice_queries.push_back({(int)c, 0});
        for (uint32_t a = 0; a < dp.num_advice; ++a)
            for (int r = 0; r < 4; ++r) advice_queries.push_back({(int)(ndyn + a), r});
        for (uint32_t c = 0; c < num_fixed_total; ++c) fixed_queries.push_back({(int)c, 0});
        degree = 4;             // max(gate 3, lookup max(4, 2 + 1 + 1))
        blinding_factors = 6;   // max(3, four queries of a gate column) + 2, as init's
        H2_REQUIRE(n > blinding_factors + 8, "k too small for the blinding rows");
        usable_rows = n - (blinding_factors + 1);
        chunk_len = degree - 2;
        quotient_pieces = degree - 1;
        extended_k = k;
        while (((uint64_t)1 << extended_k) < (uint64_t)n * quotient_pieces) ++extended_k;
        num_perm_sets = (uint32_t)((perm_columns.size() + chunk_len - 1) / chunk_len);
        return H2HIP_OK;
    }
    // FlexGateConfig / RangeConfig::configure with num_advice_per_phase / num_lookup_advice_per_phase (flex_gate/mod.rs:121-137,
    // range/mod.rs:87-108); include/h2hip.h states the layout.  One used phase and no challenge is init() of that phase's BaseCircuitParams.
    // rlc != 0 (init_rlc): `rlc` RLC columns join phase 1 behind every column of this layout
    int init_phased(const h2hip_phased_circuit_params &pp, uint32_t rlc = 0) {
        from_phased = true;
        num_rlc = rlc;
        const uint32_t *g = pp.num_advice_per_phase, *la = pp.num_lookup_advice_per_phase;
        uint64_t G = 0, LA = 0, CH = 0;
        for (int ph = 0; ph < H2HIP_MAX_PHASE; ++ph) {
            G += g[ph];
            LA += la[ph];
            CH += pp.num_challenges_per_phase[ph];
        }
        H2_REQUIRE(G >= 1 && G <= 1024 && LA <= 256 && pp.num_fixed <= 16 && pp.num_instance <= 8, "column counts out of range");
        H2_REQUIRE(CH <= H2HIP_MAX_CHALLENGES, "more than 8 challenges");
        const bool range = pp.lookup_bits >= 0 && LA != 0;   // gates/circuit/mod.rs:74-85
        const bool q_lookup = range && g[0] == 1 && la[0] != 0;
        uint32_t ded[H2HIP_MAX_PHASE], cols[H2HIP_MAX_PHASE];
        for (int ph = 0; ph < H2HIP_MAX_PHASE; ++ph) {
            ded[ph] = !range || (ph == 0 && q_lookup) ? 0 : la[ph];   // range/mod.rs:93-95: later phases always get dedicated columns
            cols[ph] = g[ph] + ded[ph] + (ph == 1 ? rlc : 0);
        }
        uint32_t used = 0;
        for (int ph = 0; ph < H2HIP_MAX_PHASE; ++ph) {
            if (cols[ph]) {
                H2_REQUIRE(ph == 0 || cols[ph - 1], "a phase has advice columns but the phase before it has none (phases must be contiguous)");
                used = (uint32_t)ph + 1;
            }
            H2_REQUIRE(!pp.num_challenges_per_phase[ph] || cols[ph], "a challenge follows a phase that has no advice column");
        }
        if (used == 1 && CH == 0 && !rlc) {
            H2_CHK(init(h2hip_base_circuit_params{pp.k, g[0], la[0], pp.num_fixed, pp.num_instance, pp.lookup_bits}));
            phase_cols.push_back({});
            for (uint32_t c = 0; c < num_advice_total; ++c) phase_cols[0].push_back((int)c);
            return H2HIP_OK;
        }
        const uint32_t nd = ded[0] + ded[1] + ded[2];
        const h2hip_base_circuit_params bp{pp.k, (uint32_t)G, nd, pp.num_fixed, pp.num_instance, pp.lookup_bits};
        p = bp;
        k = pp.k;
        H2_REQUIRE(k >= 4 && k <= 26, "k out of range (4..26)");
        H2_REQUIRE(pp.lookup_bits < (int32_t)k, "lookup_bits must be less than k");
        H2_CHK(layout(bp, range, q_lookup, nd));
        phased = true;
        uint32_t go = 0, lo = (uint32_t)G;
        for (uint32_t ph = 0; ph < used; ++ph) {
            std::vector<int> c;
            for (uint32_t i = 0; i < g[ph]; ++i) c.push_back((int)(go + i));
            for (uint32_t i = 0; i < ded[ph]; ++i) c.push_back((int)(lo + i));
            if (ph == 1)
                for (uint32_t i = 0; i < rlc; ++i) c.push_back((int)(first_rlc_advice + i));
            go += g[ph];
            lo += ded[ph];
            phase_cols.push_back(c);
            phase_challenges[ph] = pp.num_challenges_per_phase[ph];
        }
        return H2HIP_OK;
    }
    // BaseConfig::configure(base) followed by num_rlc_advice RLC columns (downstream's RlcConfig); include/h2hip.h states the layout
    int init_rlc(const h2hip_rlc_circuit_params &rp) {
        H2_REQUIRE(rp.num_rlc_advice >= 1 && rp.num_rlc_advice <= 64, "num_rlc_advice out of range (1..64; a circuit without RLC columns uses h2hip_phased_circuit_params)");
        H2_REQUIRE(rp.base.num_challenges_per_phase[0] >= 1, "the RLC gate needs a challenge usable after phase 0 (num_challenges_per_phase[0] >= 1)");
        H2_CHK(init_phased(rp.base, rp.num_rlc_advice));
        // the gate has degree 2 + selector and three rotations: degree, extended_k and the blinding factors stay the base layout's
        H2_REQUIRE(blinding_factors == 6, "internal: the RLC columns changed the blinding factors");
        Shape base;
        if (base.init_phased(rp.base) == H2HIP_OK)   // (a base that is only legal with phase 1's RLC columns has nothing to compare with)
            H2_REQUIRE(degree == base.degree && extended_k == base.extended_k && blinding_factors == base.blinding_factors && usable_rows == base.usable_rows,
                       "internal: the RLC gate changed the degree, the extended domain or the blinding factors of the base layout");
        else
            set_error("");
        return H2HIP_OK;
    }
    uint32_t num_commitments() const {
        return num_advice_total + 3 * (uint32_t)lookups.size() + num_perm_sets + 1 + quotient_pieces + 2;
    }
    uint32_t num_evals() const {
        return (uint32_t)advice_queries.size() + (uint32_t)fixed_queries.size() + 1 + (uint32_t)perm_columns.size() +
               (num_perm_sets ? 3 * num_perm_sets - 1 : 0) + 5 * (uint32_t)lookups.size();
    }
};

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
