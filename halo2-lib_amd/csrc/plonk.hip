// plonk::create_proof for halo2-base circuits with every polynomial resident in HBM.
//
// What the reference runs at halo2-base/src/utils/testing.rs:32-50
//     create_proof::<KZGCommitmentScheme<Bn256>, ProverSHPLONK<'_, Bn256>, Challenge255<_>, _, Blake2bWrite<Vec<u8>, G1Affine, _>, _>
// lives in the un-vendored halo2-axiom 0.5.3 (Cargo.lock:1063-1065); the protocol below restates it [UPSTREAM-RECALL, SURVEY.md §3.2
// and Appendix A] for the one constraint system halo2-lib builds, BaseConfig::configure (halo2-base/src/gates/circuit/mod.rs:70-96):
//     FlexGateConfig   one selector + the gate q*(a + b*c - d) at rotations 0..3 per advice column, constants columns with equality
//                      (halo2-base/src/gates/flex_gate/mod.rs:61-91,120-146)
//     RangeConfig      table column first; with a single advice column the lookup is (q_lookup * a, table) on that column, else
//                      dedicated lookup-advice columns (a, table)  (halo2-base/src/gates/range/mod.rs:71-150)
//     instance columns with equality (gates/circuit/mod.rs:89-91)
// This file is host code: the Blake2b transcript, the order of operations, and SHPLONK's O(#openings) bookkeeping.  All vector work
// goes through the kernels behind the C ABI (include/h2hip.h).  First phase only.
#include "plonk_internal.h"

// ---------------------------------------------------------------------------------------------- permutation keygen
// permutation::keygen::Assembly [UPSTREAM-RECALL]: cycles merged by `copy`; sigma_i(omega^j) = delta^i' * omega^j' for mapping[i][j] = (i', j')
struct Assembly {
    uint32_t m, n;
    std::vector<uint32_t> map_c, map_r, aux_c, aux_r, sizes;
    Assembly(uint32_t m_, uint32_t n_) : m(m_), n(n_), map_c((size_t)m_ * n_), map_r((size_t)m_ * n_), aux_c((size_t)m_ * n_), aux_r((size_t)m_ * n_), sizes((size_t)m_ * n_, 1) {
        for (uint32_t c = 0; c < m; ++c)
            for (uint32_t r = 0; r < n; ++r) {
                size_t i = (size_t)c * n + r;
                map_c[i] = aux_c[i] = c;
                map_r[i] = aux_r[i] = r;
            }
    }
    void copy(uint32_t lc, uint32_t lr, uint32_t rc, uint32_t rr) {
        size_t li = (size_t)lc * n + lr, ri = (size_t)rc * n + rr;
        uint32_t lcy_c = aux_c[li], lcy_r = aux_r[li], rcy_c = aux_c[ri], rcy_r = aux_r[ri];
        if (lcy_c == rcy_c && lcy_r == rcy_r) return;
        size_t lcy = (size_t)lcy_c * n + lcy_r, rcy = (size_t)rcy_c * n + rcy_r;
        if (sizes[lcy] < sizes[rcy]) {
            std::swap(lcy, rcy);
            std::swap(lcy_c, rcy_c);
            std::swap(lcy_r, rcy_r);
        }
        sizes[lcy] += sizes[rcy];
        size_t i = rcy;
        do {
            aux_c[i] = lcy_c;
            aux_r[i] = lcy_r;
            i = (size_t)map_c[i] * n + map_r[i];
        } while (i != rcy);
        std::swap(map_c[li], map_c[ri]);
        std::swap(map_r[li], map_r[ri]);
    }
};

static int dev_alloc(h2hip_plonk_pk *pk, size_t elems, Fr **out) {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, sizeof(Fr) * (elems ? elems : 1));
    if (e != hipSuccess) {
        set_error("hipMalloc for the proving key failed: %s", hipGetErrorString(e));
        return H2HIP_ERR_NOMEM;
    }
    pk->owned.push_back(p);
    *out = (Fr *)p;
    return H2HIP_OK;
}

// values (n, resident) -> (poly, coset): lagrange_to_coeff then coeff_to_extended
static int to_poly_and_coset(h2hip_plonk_pk *pk, const Fr *values, Fr **poly, Fr **coset) {
    h2hip_ctx *ctx = pk->ctx;
    const Shape &sh = pk->sh;
    const Domain &d = pk->dom;
    H2_CHK(dev_alloc(pk, sh.n, poly));
    H2_CHK(dev_alloc(pk, (size_t)1 << sh.extended_k, coset));
    H2_HIPCHK(hipMemcpyAsync(*poly, values, sizeof(Fr) * sh.n, hipMemcpyDeviceToDevice, ctx->stream));
    H2_CHK(h2hip_ifft_dev(ctx, *poly, &d.omega_inv, sh.k, &d.ifft_divisor));
    return h2hip_coeff_to_extended_dev(ctx, *poly, sh.k, *coset, sh.extended_k, &d.ext_omega, &d.zeta);
}

static int keygen_impl(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *fixed_host, const uint32_t *copies, size_t ncopies) {
    const Shape &sh = pk->sh;
    const uint32_t n = sh.n, m = (uint32_t)sh.perm_columns.size();
    // ---- fixed columns
    for (uint32_t c = 0; c < sh.num_fixed_total; ++c) {
        H2_REQUIRE(fixed_host[c], "NULL fixed column");
        Fr *v = nullptr, *p = nullptr, *e = nullptr;
        H2_CHK(dev_alloc(pk, n, &v));
        H2_HIPCHK(hipMemcpyAsync(v, fixed_host[c], sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->stream));
        H2_CHK(to_poly_and_coset(pk, v, &p, &e));
        pk->fixed_values.push_back(v);
        pk->fixed_polys.push_back(p);
        pk->fixed_cosets.push_back(e);
    }
    // ---- permutation: cycles on the host, sigma values delta^c' * omega^r'
    Assembly as(m, n);
    for (size_t i = 0; i < ncopies; ++i) {
        const uint32_t *c = copies + 4 * i;
        H2_REQUIRE(c[0] < m && c[2] < m, "copy constraint names a column outside the permutation");
        H2_REQUIRE(c[1] < sh.usable_rows && c[3] < sh.usable_rows, "copy constraint outside the usable rows (NotEnoughRowsAvailable)");
        as.copy(c[0], c[1], c[2], c[3]);
    }
    H2_REQUIRE(m <= 65536, "more than 65536 permutation columns");
    pk->sigma_c_host.resize((size_t)m * sh.usable_rows);
    pk->sigma_r_host.resize((size_t)m * sh.usable_rows);
    for (uint32_t c = 0; c < m; ++c)
        for (uint32_t r = 0; r < sh.usable_rows; ++r) {
            const size_t i = (size_t)c * n + r, o = (size_t)c * sh.usable_rows + r;
            pk->sigma_c_host[o] = (uint16_t)as.map_c[i];
            pk->sigma_r_host[o] = as.map_r[i];
        }
    std::vector<Fr> wpow(n), dpow(m ? m : 1), col(n);
    wpow[0] = Fr::one();
    for (uint32_t j = 1; j < n; ++j) wpow[j] = fe_mul(wpow[j - 1], pk->dom.omega);
    dpow[0] = Fr::one();
    for (uint32_t i = 1; i < m; ++i) dpow[i] = fe_mul(dpow[i - 1], pk->dom.delta);
    for (uint32_t c = 0; c < m; ++c) {
        for (uint32_t r = 0; r < n; ++r) {
            size_t i = (size_t)c * n + r;
            col[r] = as.map_c[i] == 0 ? wpow[as.map_r[i]] : fe_mul(dpow[as.map_c[i]], wpow[as.map_r[i]]);
        }
        Fr *v = nullptr, *p = nullptr, *e = nullptr;
        H2_CHK(dev_alloc(pk, n, &v));
        H2_HIPCHK(hipMemcpyAsync(v, col.data(), sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->stream));
        H2_HIPCHK(hipStreamSynchronize(ctx->stream));   // `col` is reused
        H2_CHK(to_poly_and_coset(pk, v, &p, &e));
        pk->sigma_values.push_back(v);
        pk->sigma_polys.push_back(p);
        pk->sigma_cosets.push_back(e);
    }
    if (!sh.lookups.empty() && !sh.dyn) {   // every lookup of a BaseConfig circuit uses the one range table (a dynamic table is sorted per proof)
        void *ts = nullptr;
        hipError_t e = hipMalloc(&ts, h2hip_lookup_sorted_table_bytes(sh.usable_rows));
        if (e != hipSuccess) {
            set_error("hipMalloc for the sorted lookup table failed: %s", hipGetErrorString(e));
            return H2HIP_ERR_NOMEM;
        }
        pk->owned.push_back(ts);
        pk->table_sorted = ts;
        H2_CHK(h2hip_lookup_table_sort_dev(ctx, pk->fixed_values[sh.table_col], sh.usable_rows, ts));
    }
    // ---- commitments of the verifying key
    std::vector<const void *> cols;
    for (Fr *v : pk->fixed_values) cols.push_back(v);
    for (Fr *v : pk->sigma_values) cols.push_back(v);
    std::vector<G1Affine> comm(cols.size());
    if (!cols.empty()) H2_CHK(h2hip_msm_g1_batch_dev(ctx, pk->g_lagrange, cols.data(), n, cols.size(), H2HIP_POINT_AFFINE, comm.data()));
    pk->fixed_commitments.assign(comm.begin(), comm.begin() + sh.num_fixed_total);
    pk->permutation_commitments.assign(comm.begin() + sh.num_fixed_total, comm.end());
    // ---- l_0, l_last, l_blind on the extended domain
    Fr *tmp = nullptr, *tp = nullptr;
    H2_CHK(dev_alloc(pk, n, &tmp));
    std::vector<Fr> lv(n);
    const Fr one = Fr::one(), zero = Fr::zero();
    const uint32_t bf = sh.blinding_factors;
    Fr **dst[3] = {&pk->l0, &pk->l_last, &pk->l_blind};
    for (int which = 0; which < 3; ++which) {
        for (uint32_t r = 0; r < n; ++r) lv[r] = zero;
        if (which == 0) lv[0] = one;
        if (which == 1) lv[n - bf - 1] = one;
        if (which == 2)
            for (uint32_t r = n - bf; r < n; ++r) lv[r] = one;
        H2_HIPCHK(hipMemcpyAsync(tmp, lv.data(), sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->stream));
        H2_HIPCHK(hipStreamSynchronize(ctx->stream));
        H2_CHK(to_poly_and_coset(pk, tmp, &tp, dst[which]));
    }
    H2_HIPCHK(hipStreamSynchronize(ctx->stream));
    return H2HIP_OK;
}

extern "C" {

static void fill_shape(const Shape &sh, h2hip_plonk_shape *out) {
    out->num_advice_total = sh.num_advice_total;
    out->num_fixed_total = sh.num_fixed_total;
    out->table_col = sh.table_col;
    out->first_constant_col = sh.first_constant_col;
    out->q_lookup_col = sh.q_lookup_col;
    out->first_q_enable_col = sh.first_q_enable_col;
    out->num_lookups = (uint32_t)sh.lookups.size();
    out->num_perm_columns = (uint32_t)sh.perm_columns.size();
    out->num_perm_sets = sh.num_perm_sets;
    out->degree = sh.degree;
    out->extended_k = sh.extended_k;
    out->blinding_factors = sh.blinding_factors;
    out->usable_rows = sh.usable_rows;
    out->quotient_pieces = sh.quotient_pieces;
    out->num_commitments = sh.num_commitments();
    out->num_evals = sh.num_evals();
}

static int shape_of(int kind, const void *params, h2hip_plonk_shape *out) {
    Shape sh;
    H2_CHK(shape_of_kind(kind, params, sh));
    fill_shape(sh, out);
    return H2HIP_OK;
}
int h2hip_plonk_shape_of(const h2hip_base_circuit_params *params, h2hip_plonk_shape *out) {
    H2_REQUIRE(params && out, "NULL argument");
    return shape_of(H2HIP_CIRCUIT_BASE, params, out);
}
int h2hip_plonk_shape_of_dyn(const h2hip_dyn_circuit_params *params, h2hip_plonk_shape *out) {
    H2_REQUIRE(params && out, "NULL argument");
    return shape_of(H2HIP_CIRCUIT_DYN, params, out);
}
int h2hip_plonk_shape_of_phased(const h2hip_phased_circuit_params *params, h2hip_plonk_shape *out) {
    H2_REQUIRE(params && out, "NULL argument");
    return shape_of(H2HIP_CIRCUIT_PHASED, params, out);
}
int h2hip_plonk_shape_of_rlc(const h2hip_rlc_circuit_params *params, h2hip_plonk_shape *out) {
    H2_REQUIRE(params && out, "NULL argument");
    return shape_of(H2HIP_CIRCUIT_RLC, params, out);
}

// Shape::init gives every gate column's q_enable selector a fixed column of its own.  Upstream's compress_selectors [UPSTREAM-RECALL] would
// instead COMBINE simple selectors that are never enabled on a common row (as far as the degree bound allows) — e.g. a gate column that the
// circuit left empty — which changes the number of fixed columns, the verifying key and the proof size.  Such circuits are rejected here
// rather than proven against a key halo2 would not derive: every pair of q_enable columns must share an enabled row.
// The rule covers the union of the q_enable and the q_rlc columns (simple selectors alike); a = 0 .. num_advice - 1 names a gate column, the
// indices behind them the RLC columns.  A q_rlc enabled where the gate would read blinding rows is rejected here too.
static int check_selectors_stay_apart(const Shape &sh, const void *const *fixed_host) {
    const uint32_t ng = sh.p.num_advice, na = ng + sh.num_rlc;
    const size_t words = (sh.n + 63) / 64;
    for (uint32_t j = 0; j < sh.num_rlc; ++j) {
        const Fr *col = (const Fr *)fixed_host[sh.first_q_rlc_col + (int)j];
        H2_REQUIRE(col, "NULL fixed column");
        for (size_t r = sh.usable_rows >= 2 ? sh.usable_rows - 2 : 0; r < sh.usable_rows; ++r)
            if (!col[r].is_zero()) {
                set_error("h2hip_plonk_keygen_rlc: q_rlc of RLC column %u is enabled on row %zu, but the gate reads rows r .. r + 2 and only %u rows are usable", j, r,
                          sh.usable_rows);
                return H2HIP_ERR_INVALID;
            }
    }
    if (na < 2) return H2HIP_OK;
    std::vector<uint64_t> bits((size_t)na * words, 0);
    for (uint32_t a = 0; a < na; ++a) {
        const Fr *col = (const Fr *)fixed_host[a < ng ? sh.first_q_enable_col + (int)a : sh.first_q_rlc_col + (int)(a - ng)];
        H2_REQUIRE(col, "NULL fixed column");
        for (size_t r = 0; r < sh.usable_rows; ++r)
            if (!col[r].is_zero()) bits[a * words + (r >> 6)] |= 1ull << (r & 63);
    }
    // a row enabled in EVERY column settles all pairs at once (the usual case: gates start at row 0 of every column)
    for (size_t w = 0; w < words; ++w) {
        uint64_t all = ~0ull;
        for (uint32_t a = 0; a < na && all; ++a) all &= bits[a * words + w];
        if (all) return H2HIP_OK;
    }
    for (uint32_t a = 0; a < na; ++a)
        for (uint32_t b = a + 1; b < na; ++b) {
            bool share = false;
            for (size_t w = 0; w < words && !share; ++w) share = (bits[a * words + w] & bits[b * words + w]) != 0;
            if (!share) {
                set_error("h2hip_plonk_keygen: the selectors of gate columns %u and %u are never enabled on a common row (an empty gate column?): "
                          "halo2's selector compression would merge them into one fixed column, which this backend's fixed-column layout does not model%s", a, b,
                          sh.num_rlc ? " (indices from the number of gate columns on name RLC columns)" : "");
                return H2HIP_ERR_INVALID;
            }
        }
    return H2HIP_OK;
}

static int keygen_common(h2hip_ctx *ctx, int kind, const void *params, const h2hip_bases *g, const h2hip_bases *g_lagrange, const void *const *fixed_host,
                         const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out);
static void sync_proof_streams(h2hip_ctx *ctx, h2hip_plonk_pk *pk) {
    if (pk->copy_stream) hipStreamSynchronize(pk->copy_stream);
    if (pk->side) hipStreamSynchronize(pk->side->stream);
    for (h2hip_ctx *l : ctx->lane)
        if (l) hipStreamSynchronize(l->stream);
    hipStreamSynchronize(ctx->stream);
}

int h2hip_plonk_keygen(h2hip_ctx *ctx, const h2hip_base_circuit_params *params, const h2hip_bases *g, const h2hip_bases *g_lagrange,
                       const void *const *fixed_host, const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && params && g && g_lagrange && fixed_host && out && (ncopies == 0 || copies), "NULL argument");
    return keygen_common(ctx, H2HIP_CIRCUIT_BASE, params, g, g_lagrange, fixed_host, copies, ncopies, out);
}

int h2hip_plonk_keygen_dyn(h2hip_ctx *ctx, const h2hip_dyn_circuit_params *params, const h2hip_bases *g, const h2hip_bases *g_lagrange,
                           const void *const *fixed_host, const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && params && g && g_lagrange && fixed_host && out && (ncopies == 0 || copies), "NULL argument");
    return keygen_common(ctx, H2HIP_CIRCUIT_DYN, params, g, g_lagrange, fixed_host, copies, ncopies, out);
}

int h2hip_plonk_keygen_phased(h2hip_ctx *ctx, const h2hip_phased_circuit_params *params, const h2hip_bases *g, const h2hip_bases *g_lagrange,
                              const void *const *fixed_host, const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && params && g && g_lagrange && fixed_host && out && (ncopies == 0 || copies), "NULL argument");
    return keygen_common(ctx, H2HIP_CIRCUIT_PHASED, params, g, g_lagrange, fixed_host, copies, ncopies, out);
}

int h2hip_plonk_keygen_rlc(h2hip_ctx *ctx, const h2hip_rlc_circuit_params *params, const h2hip_bases *g, const h2hip_bases *g_lagrange,
                           const void *const *fixed_host, const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && params && g && g_lagrange && fixed_host && out && (ncopies == 0 || copies), "NULL argument");
    return keygen_common(ctx, H2HIP_CIRCUIT_RLC, params, g, g_lagrange, fixed_host, copies, ncopies, out);
}

static int keygen_common(h2hip_ctx *ctx, int kind, const void *params, const h2hip_bases *g, const h2hip_bases *g_lagrange, const void *const *fixed_host,
                         const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out) {
    h2hip_plonk_pk *pk = new h2hip_plonk_pk();
    int rc = shape_of_kind(kind, params, pk->sh);
    if (rc == H2HIP_OK && (g->n < pk->sh.n || g_lagrange->n < pk->sh.n)) {
        set_error("h2hip_plonk_keygen: the SRS holds fewer than 2^k bases");
        rc = H2HIP_ERR_INVALID;
    }
    if (rc == H2HIP_OK) rc = check_selectors_stay_apart(pk->sh, fixed_host);
    if (rc == H2HIP_OK) {
        pk->ctx = ctx;
        pk->g = g;
        pk->g_lagrange = g_lagrange;
        pk->dom.init(pk->sh.k, pk->sh.extended_k);
        rc = keygen_impl(ctx, pk, fixed_host, copies, ncopies);
    }
    if (rc != H2HIP_OK) {
        h2hip_plonk_pk_free(ctx, pk);
        return rc;
    }
    // Warm-up (r04): one throw-away proof of the all-zero witness, so that what a FIRST create_proof used to pay for — the key's buffer pool,
    // the twiddle tables of both domains, the MSM lanes and their scratch, the pinned staging buffer, the LDS attributes — exists when keygen
    // returns (the first proof after keygen took 22-27 ms against 15 ms warm).  Best effort: a failure here only leaves the first proof cold.
    if (ctx->plonk_warm_keygen) {
        std::vector<Fr *> zero_cols(pk->sh.num_advice_total, nullptr);
        bool ok = true;
        for (auto &c : zero_cols) {
            if (hipMalloc((void **)&c, sizeof(Fr) * pk->sh.n) != hipSuccess) {
                c = nullptr;
                ok = false;
                break;
            }
            hipMemsetAsync(c, 0, sizeof(Fr) * pk->sh.n, ctx->stream);
        }
        if (ok) {
            std::vector<const void *> adv(zero_cols.begin(), zero_cols.end());
            std::vector<Fr> inst_zero(1, Fr::zero());
            std::vector<const void *> inst(pk->sh.p.num_instance, inst_zero.data());
            std::vector<size_t> inst_len(pk->sh.p.num_instance, 0);
            h2hip_chacha_rng wr;
            uint8_t seed[32] = {0};
            h2hip_chacha_rng_init(&wr, seed, 8);
            Transcript throwaway;
            const Fr saved = pk->transcript_repr;
            pk->transcript_repr = Fr::zero();
            const int wrc = create_proof_impl(ctx, pk, adv.data(), true, inst.data(), inst_len.data(), h2hip_chacha_rng_fill, &wr, throwaway, nullptr);
            pk->transcript_repr = saved;
            sync_proof_streams(ctx, pk);
            if (wrc != H2HIP_OK) set_error("");   // not the caller's error
        }
        hipStreamSynchronize(ctx->stream);
        for (Fr *c : zero_cols)
            if (c) hipFree(c);
    }
    *out = pk;
    return H2HIP_OK;
}

void h2hip_plonk_pk_free(h2hip_ctx *ctx, h2hip_plonk_pk *pk) {
    H2_DEVICE_GUARD(ctx);
    if (!pk) return;
    if (ctx) hipStreamSynchronize(ctx->stream);
    for (void *p : pk->owned) hipFree(p);
    for (void *p : pk->shard_owned) hipFree(p);
    if (pk->host_stage) hipHostFree(pk->host_stage);
    if (pk->copy_ev) hipEventDestroy(pk->copy_ev);
    if (pk->copy_stream) hipStreamDestroy(pk->copy_stream);
    if (pk->side_ev) hipEventDestroy(pk->side_ev);
    if (pk->side_ev1) hipEventDestroy(pk->side_ev1);
    if (pk->side) h2hip_destroy(pk->side);
    pk->pool.destroy();
    delete pk;
}

int h2hip_plonk_pk_commitments(const h2hip_plonk_pk *pk, void *fixed_out, void *permutation_out) {
    H2_REQUIRE(pk, "NULL argument");
    if (fixed_out && !pk->fixed_commitments.empty()) memcpy(fixed_out, pk->fixed_commitments.data(), sizeof(G1Affine) * pk->fixed_commitments.size());
    if (permutation_out && !pk->permutation_commitments.empty())
        memcpy(permutation_out, pk->permutation_commitments.data(), sizeof(G1Affine) * pk->permutation_commitments.size());
    return H2HIP_OK;
}

int h2hip_plonk_pk_set_transcript_repr(h2hip_plonk_pk *pk, const void *fr) {
    H2_REQUIRE(pk && fr, "NULL argument");
    memcpy(&pk->transcript_repr, fr, sizeof(Fr));
    pk->have_repr = true;
    return H2HIP_OK;
}

static void shard_release(h2hip_plonk_pk *pk) {
    if (pk->ctx) hipStreamSynchronize(pk->ctx->stream);
    for (void *q : pk->shard_owned) hipFree(q);
    pk->shard_owned.clear();
    pk->fixed_cosets_sh.clear();
    pk->sigma_cosets_sh.clear();
    pk->l0_sh = pk->l_last_sh = pk->l_blind_sh = nullptr;
    pk->my_cosets.clear();
    pk->shard_world = 1;
    pk->shard_rank = 0;
    pk->g_shard = pk->g_lagrange_shard = nullptr;
    pk->comm = nullptr;
    pk->shard_quotient = false;
    pk->shard_products = false;
    pk->shard_ntt = false;
}

// the host exchanges of the key's last sharded proof, in order: payload bytes per rank (each travels with an 8-byte status word); what a
// multi-GPU run reports about itself (bench.py --gpus N).  count: the number of exchanges; sizes: the first min(count, cap) of them
int h2hip_plonk_pk_last_exchanges(const h2hip_plonk_pk *pk, size_t *sizes, size_t cap, size_t *count) {
    H2_REQUIRE(pk && count && (cap == 0 || sizes), "NULL argument");
    *count = pk->exch_sizes.size();
    for (size_t i = 0; i < pk->exch_sizes.size() && i < cap; ++i) sizes[i] = pk->exch_sizes[i];
    return H2HIP_OK;
}

int h2hip_plonk_pk_set_sharding(h2hip_plonk_pk *pk, h2hip_comm *comm, const h2hip_bases *g_shard, const h2hip_bases *g_lagrange_shard, size_t offset,
                                size_t len, uint32_t flags) {
    H2_REQUIRE(pk, "NULL argument");
    H2_DEVICE_GUARD(pk->ctx);
    shard_release(pk);
    int world = 1, rank = 0;
    if (comm) H2_CHK(h2hip_comm_info(comm, &world, &rank, nullptr));
    H2_REQUIRE(!(comm && pk->sh.dyn), "h2hip_plonk_pk_set_sharding: proofs with a dynamic lookup table run on one GPU");
    H2_REQUIRE(!(comm && pk->sh.phased), "h2hip_plonk_pk_set_sharding: multi-phase proofs run on one GPU");
    if (!comm || (world <= 1 && !(flags & H2HIP_SHARD_FORCE))) return H2HIP_OK;
    H2_REQUIRE(g_shard && g_lagrange_shard, "NULL argument");
    H2_REQUIRE(offset <= pk->sh.n && len <= pk->sh.n - offset && g_shard->n >= len && g_lagrange_shard->n >= len, "shard range outside the SRS / shard base sets too small");
    pk->g_shard = g_shard;
    pk->g_lagrange_shard = g_lagrange_shard;
    pk->shard_offset = offset;
    pk->shard_len = len;
    pk->shard_world = (uint32_t)world;
    pk->shard_rank = (uint32_t)rank;
    pk->comm = comm;
    pk->shard_quotient = (flags & H2HIP_SHARD_QUOTIENT) != 0;
    pk->shard_products = (flags & H2HIP_SHARD_PRODUCTS) != 0;
    pk->shard_ntt = (flags & H2HIP_SHARD_NTT_COLUMNS) != 0;
    if (!pk->shard_quotient) return H2HIP_OK;
    // this rank's cosets of the extended domain: c = rank, rank + world, ... < 2^(ek - k), and the [coset][n] slices of the key's arrays
    const uint32_t log_c = pk->sh.extended_k - pk->sh.k, ncos = 1u << log_c, n = pk->sh.n;
    H2_REQUIRE(log_c <= 4, "more than 16 cosets");
    for (uint32_t c = (uint32_t)rank; c < ncos; c += (uint32_t)world) pk->my_cosets.push_back(c);
    pk->max_cosets = (ncos + (uint32_t)world - 1) / (uint32_t)world;
    const size_t cnt = pk->my_cosets.size(), elems = std::max<size_t>(cnt * (size_t)n, 1);
    auto slice = [&](const Fr *full, Fr **out) -> int {
        void *d = nullptr;
        if (hipMalloc(&d, sizeof(Fr) * elems) != hipSuccess) {
            set_error("hipMalloc for the sharded proving key failed");
            return H2HIP_ERR_NOMEM;
        }
        pk->shard_owned.push_back(d);
        *out = (Fr *)d;
        return h2hip_fr_coset_gather_dev(pk->ctx, d, full, pk->my_cosets.data(), (uint32_t)cnt, log_c, n);
    };
    int rc = H2HIP_OK;
    pk->fixed_cosets_sh.assign(pk->fixed_cosets.size(), nullptr);
    pk->sigma_cosets_sh.assign(pk->sigma_cosets.size(), nullptr);
    for (size_t i = 0; rc == H2HIP_OK && i < pk->fixed_cosets.size(); ++i) rc = slice(pk->fixed_cosets[i], &pk->fixed_cosets_sh[i]);
    for (size_t i = 0; rc == H2HIP_OK && i < pk->sigma_cosets.size(); ++i) rc = slice(pk->sigma_cosets[i], &pk->sigma_cosets_sh[i]);
    if (rc == H2HIP_OK) rc = slice(pk->l0, &pk->l0_sh);
    if (rc == H2HIP_OK) rc = slice(pk->l_last, &pk->l_last_sh);
    if (rc == H2HIP_OK) rc = slice(pk->l_blind, &pk->l_blind_sh);
    if (rc == H2HIP_OK && hipStreamSynchronize(pk->ctx->stream) != hipSuccess) rc = H2HIP_ERR_HIP;
    if (rc != H2HIP_OK) shard_release(pk);
    return rc;
}

void h2hip_array_rng_fill(void *user, void *out_fr, size_t n) {
    h2hip_array_rng *r = (h2hip_array_rng *)user;
    if (!r || !out_fr) return;
    const size_t have = r->pos < r->count ? r->count - r->pos : 0, take = n < have ? n : have;
    if (take) memcpy(out_fr, (const char *)r->values + sizeof(Fr) * r->pos, sizeof(Fr) * take);
    if (take < n) {
        memset((char *)out_fr + sizeof(Fr) * take, 0, sizeof(Fr) * (n - take));
        r->exhausted = 1;
    }
    r->pos += take;
}


// one proof over `tr`, behind the argument checks every entry shares; on failure every stream of the proof is drained
static int create_proof_run(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device, const void *const *instances_host,
                            const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user, const h2hip_phase_witness *witness,
                            ProverTranscript &tr, double *stage_ms) {
    H2_REQUIRE(pk->ctx == ctx, "the proving key belongs to another context");
    H2_REQUIRE(pk->have_repr, "h2hip_plonk_pk_set_transcript_repr has not been called");
    H2_REQUIRE(pk->sh.p.num_instance == 0 || instance_lens, "instance_lens is required");
    if (rng == h2hip_chacha_rng_fill) {   // the library's own generator: the device fill reads its state, so check it once, here
        const h2hip_chacha_rng *cr = (const h2hip_chacha_rng *)rng_user;
        H2_REQUIRE(cr, "h2hip_chacha_rng_fill needs its h2hip_chacha_rng as rng_user");
        H2_REQUIRE(cr->rounds == 8 || cr->rounds == 12 || cr->rounds == 20, "h2hip_chacha_rng: rounds must be 8, 12 or 20");
    }
    int rc = create_proof_impl(ctx, pk, advice, advice_on_device != 0, instances_host, instance_lens, rng, rng_user, tr, stage_ms, witness);
    if (pk->side && ctx->profiling && ctx->prof_filter.empty()) prof_fold_child(ctx, pk->side);   // (the lanes' timers are folded when the table is read)
    if (rc != H2HIP_OK) {
        sync_proof_streams(ctx, pk);   // nothing of the failed proof may still run on buffers that go back to the pool
        if (rc != H2HIP_ERR_PEER && pk->comm && pk->exch_next < pk->exch_sizes.size()) {
            // a sharded proof failed HERE (a lookup value missing from the table, an identity commitment, an allocation ...): the other
            // ranks are on their way into the next exchange — take part in it with an error status so that all of them return too
            const std::string msg = h2hip_last_error();
            const size_t bytes = 8 + pk->exch_sizes[pk->exch_next];
            std::vector<uint8_t> send(bytes, 0), all(bytes * (size_t)pk->shard_world);
            const uint64_t status = 1;
            memcpy(send.data(), &status, 8);
            h2hip_comm_allgather_host(pk->comm, ctx, send.data(), bytes, all.data());
            pk->exch_next = pk->exch_sizes.size();
            set_error("%s", msg.c_str());
        }
    }
    return rc;
}

static int create_proof_entry(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device, const void *const *instances_host,
                              const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user, const h2hip_phase_witness *witness,
                              uint8_t *proof_out, size_t proof_cap, size_t *proof_len, double *stage_ms) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && pk && advice && rng && proof_out && proof_len, "NULL argument");
    const size_t need = 32 * (size_t)(pk->sh.num_commitments() + pk->sh.num_evals());
    H2_REQUIRE(proof_cap >= need, "proof buffer too small");
    Transcript tr;
    H2_CHK(create_proof_run(ctx, pk, advice, advice_on_device, instances_host, instance_lens, rng, rng_user, witness, tr, stage_ms));
    const std::vector<uint8_t> &proof = tr.proof;
    if (proof.size() != need) {
        set_error("create_proof: internal error: proof has %zu bytes, expected %zu", proof.size(), need);
        return H2HIP_ERR_INVALID;
    }
    memcpy(proof_out, proof.data(), need);
    *proof_len = need;
    return H2HIP_OK;
}

int h2hip_plonk_create_proof(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device, const void *const *instances_host,
                             const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user, uint8_t *proof_out, size_t proof_cap,
                             size_t *proof_len, double *stage_ms) {
    H2_REQUIRE(!pk || pk->sh.phase_cols.size() <= 1, "h2hip_plonk_create_proof: the key has more than one phase (use h2hip_plonk_create_proof_phased)");
    return create_proof_entry(ctx, pk, advice, advice_on_device, instances_host, instance_lens, rng, rng_user, nullptr, proof_out, proof_cap, proof_len,
                              stage_ms);
}

int h2hip_plonk_create_proof_phased(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device,
                                    const void *const *instances_host, const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user,
                                    const h2hip_phase_witness *witness, uint8_t *proof_out, size_t proof_cap, size_t *proof_len, double *stage_ms) {
    H2_REQUIRE(!pk || pk->sh.from_phased, "h2hip_plonk_create_proof_phased: the key is not of the multi-phase configuration");
    H2_REQUIRE(!pk || pk->sh.phase_cols.size() <= 1 || (witness && witness->fill), "h2hip_plonk_create_proof_phased: a later phase needs the witness callback");
    return create_proof_entry(ctx, pk, advice, advice_on_device, instances_host, instance_lens, rng, rng_user, witness, proof_out, proof_cap, proof_len,
                              stage_ms);
}

// create_proof over the caller's transcript (include/h2hip.h): the same run, every transcript operation through the callbacks
int h2hip_plonk_create_proof_transcript(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device,
                                        const void *const *instances_host, const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user,
                                        const h2hip_phase_witness *witness, const h2hip_transcript *t, double *stage_ms) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && pk && advice && rng && t, "NULL argument");
    H2_REQUIRE(t->common_scalar && t->write_point && t->write_scalar && t->squeeze_challenge,
               "h2hip_plonk_create_proof_transcript: the transcript lacks common_scalar, write_point, write_scalar or squeeze_challenge");
    H2_REQUIRE(!pk->comm, "h2hip_plonk_create_proof_transcript: the key is sharded (h2hip_plonk_pk_set_sharding); sharded proofs use the built-in transcript");
    H2_REQUIRE(pk->sh.phase_cols.size() <= 1 || (witness && witness->fill), "h2hip_plonk_create_proof_transcript: a later phase needs the witness callback");
    CallbackTranscript tr(t);
    return create_proof_run(ctx, pk, advice, advice_on_device, instances_host, instance_lens, rng, rng_user, witness, tr, stage_ms);
}

// MockProver's verdict on the GPU (include/h2hip.h): the key's layout as a WitnessCheckJob for witness_check.hip
static int check_witness_entry(h2hip_ctx *ctx, const h2hip_plonk_pk *pk_in, const void *const *advice, int advice_on_device,
                               const void *const *instances_host, const size_t *instance_lens, const Fr *challenge0, h2hip_witness_failure *failures_out,
                               size_t max_failures, size_t *num_failures);
int h2hip_plonk_check_witness(h2hip_ctx *ctx, const h2hip_plonk_pk *pk_in, const void *const *advice, int advice_on_device,
                              const void *const *instances_host, const size_t *instance_lens, h2hip_witness_failure *failures_out,
                              size_t max_failures, size_t *num_failures) {
    H2_REQUIRE(!pk_in || !pk_in->sh.num_rlc, "the key has RLC gates, which query a challenge (use h2hip_plonk_check_witness_challenges)");
    return check_witness_entry(ctx, pk_in, advice, advice_on_device, instances_host, instance_lens, nullptr, failures_out, max_failures, num_failures);
}
int h2hip_plonk_check_witness_challenges(h2hip_ctx *ctx, const h2hip_plonk_pk *pk_in, const void *const *advice, int advice_on_device,
                                         const void *const *instances_host, const size_t *instance_lens, const void *challenges_fr,
                                         size_t num_challenges, h2hip_witness_failure *failures_out, size_t max_failures, size_t *num_failures) {
    H2_REQUIRE(num_challenges == 0 || challenges_fr, "NULL argument");
    H2_REQUIRE(!pk_in || !pk_in->sh.num_rlc || num_challenges >= 1, "the key's RLC gates need challenge 0");
    Fr c0 = Fr::zero();
    if (num_challenges) c0 = ld_fr(challenges_fr);
    return check_witness_entry(ctx, pk_in, advice, advice_on_device, instances_host, instance_lens, num_challenges ? &c0 : nullptr, failures_out, max_failures,
                               num_failures);
}
static int check_witness_entry(h2hip_ctx *ctx, const h2hip_plonk_pk *pk_in, const void *const *advice, int advice_on_device,
                               const void *const *instances_host, const size_t *instance_lens, const Fr *challenge0, h2hip_witness_failure *failures_out,
                               size_t max_failures, size_t *num_failures) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE_AS("h2hip_plonk_check_witness", ctx && pk_in && advice && num_failures, "NULL argument");
    H2_REQUIRE_AS("h2hip_plonk_check_witness", failures_out || max_failures == 0, "failures_out is NULL and max_failures > 0");
    h2hip_plonk_pk *pk = const_cast<h2hip_plonk_pk *>(pk_in);   // (its buffer pool and the one-time upload of the cycles)
    H2_REQUIRE_AS("h2hip_plonk_check_witness", pk->ctx == ctx, "the proving key belongs to another context");
    const Shape &sh = pk->sh;
    const uint32_t n = sh.n, u = sh.usable_rows, F = sh.num_fixed_total, A = sh.num_advice_total, I = sh.p.num_instance;
    H2_REQUIRE_AS("h2hip_plonk_check_witness", I == 0 || instance_lens, "instance_lens is required");
    for (uint32_t c = 0; c < A; ++c) H2_REQUIRE_AS("h2hip_plonk_check_witness", advice[c], "NULL advice column");
    for (uint32_t i = 0; i < I; ++i) {
        H2_REQUIRE_AS("h2hip_plonk_check_witness", instance_lens[i] <= u, "InstanceTooLarge");
        H2_REQUIRE_AS("h2hip_plonk_check_witness", instance_lens[i] == 0 || (instances_host && instances_host[i]), "NULL instance column");
    }
    *num_failures = 0;
    hipStream_t st = ctx->stream;
    const uint32_t m = (uint32_t)sh.perm_columns.size();
    if (m && !pk->sigma_c_dev) {
        void *c = nullptr, *r = nullptr;
        H2_HIPCHK(hipMalloc(&c, sizeof(uint16_t) * pk->sigma_c_host.size()));
        pk->owned.push_back(c);
        H2_HIPCHK(hipMalloc(&r, sizeof(uint32_t) * pk->sigma_r_host.size()));
        pk->owned.push_back(r);
        H2_HIPCHK(hipMemcpyAsync(c, pk->sigma_c_host.data(), sizeof(uint16_t) * pk->sigma_c_host.size(), hipMemcpyHostToDevice, st));
        H2_HIPCHK(hipMemcpyAsync(r, pk->sigma_r_host.data(), sizeof(uint32_t) * pk->sigma_r_host.size(), hipMemcpyHostToDevice, st));
        H2_HIPCHK(hipStreamSynchronize(st));
        pk->sigma_c_dev = (uint16_t *)c;
        pk->sigma_r_dev = (uint32_t *)r;
    }
    Scope sc(&pk->pool);
    WitnessCheckJob job;
    job.u = u;
    for (uint32_t c = 0; c < F; ++c) job.cols.push_back(pk->fixed_values[c]);
    int rc = H2HIP_OK;
    for (uint32_t c = 0; c < A && rc == H2HIP_OK; ++c) {
        if (advice_on_device) {
            job.cols.push_back((const Fr *)advice[c]);
            continue;
        }
        Fr *d = nullptr;
        rc = sc.take(n, &d);
        if (rc == H2HIP_OK && hipMemcpyAsync(d, advice[c], sizeof(Fr) * u, hipMemcpyHostToDevice, st) != hipSuccess) {
            set_error("h2hip_plonk_check_witness: advice upload failed");
            rc = H2HIP_ERR_HIP;
        }
        job.cols.push_back(d);
    }
    for (uint32_t i = 0; i < I && rc == H2HIP_OK; ++i) {   // zero-padded as create_proof pads them
        Fr *d = nullptr;
        rc = sc.take(n, &d);
        if (rc == H2HIP_OK && (hipMemsetAsync(d, 0, sizeof(Fr) * u, st) != hipSuccess ||
                               (instance_lens[i] && hipMemcpyAsync(d, instances_host[i], sizeof(Fr) * instance_lens[i], hipMemcpyHostToDevice, st) != hipSuccess))) {
            set_error("h2hip_plonk_check_witness: instance upload failed");
            rc = H2HIP_ERR_HIP;
        }
        job.cols.push_back(d);
    }
    if (rc == H2HIP_OK) {
        auto flat = [&](const ColumnRef &c) -> uint32_t { return c.kind == 0 ? (uint32_t)c.index : c.kind == 1 ? F + (uint32_t)c.index : F + A + (uint32_t)c.index; };
        std::vector<std::pair<int, int>> gates = sh.gates(), rlc = sh.rlc_gates();
        gates.insert(gates.end(), rlc.begin(), rlc.end());   // behind the flex gates, as the prover folds them
        for (const auto &g : gates) {
            job.gate_report.push_back((uint32_t)g.second);
            job.gate_adv.push_back(F + (uint32_t)g.second);
            job.gate_q.push_back((uint32_t)g.first);
        }
        job.num_rlc_gates = sh.num_rlc;
        if (sh.num_rlc) job.rlc_gamma = *challenge0;
        job.num_lookups = (uint32_t)sh.lookups.size();
        if (sh.dyn) {
            job.dyn_width = sh.key_cols + 1;
            for (const Lookup &l : sh.lookups)
                for (const ColumnRef &c : l.in) job.dyn_in.push_back(flat(c));
            if (!sh.lookups.empty())
                for (const ColumnRef &c : sh.lookups[0].tab) job.dyn_tab.push_back(flat(c));
        } else {
            for (const Lookup &l : sh.lookups) {
                job.lk_in.push_back(F + (uint32_t)l.advice_col);
                job.lk_q.push_back(l.q_col >= 0 ? (uint32_t)l.q_col : WC_NONE);
            }
            job.table_sorted = pk->table_sorted;
        }
        for (const ColumnRef &c : sh.perm_columns) job.perm_col.push_back(flat(c));
        job.sigma_c = pk->sigma_c_dev;
        job.sigma_r = pk->sigma_r_dev;
        rc = witness_check_run(ctx, job, failures_out, max_failures, num_failures);
    }
    hipStreamSynchronize(st);   // nothing of the check may still read buffers that go back to the pool
    if (rc != H2HIP_OK) *num_failures = 0;
    return rc;
}

}  // extern "C"
