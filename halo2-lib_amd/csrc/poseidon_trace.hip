// In-circuit Poseidon traces filled on the device: every flex-gate cell that PoseidonHasher::hash_fix_len_array / PoseidonSponge::squeeze
// (fix_len_array_squeeze, halo2-base/src/poseidon/hasher/mod.rs:344-361) writes into a gate column, for many hashes at once (include/h2hip.h
// states the cell form).  The permutation is OptimizedPoseidonSpec's (hasher/state.rs:35-83): the host derives that spec from the textbook
// arrays (h2hip_poseidon_spec_optimize: spec.rs:108-175, mds.rs:118-171) and keeps it on the context, canonical Montgomery Fr.
//
// One lane per unit (the unit's code is poseidon_trace.cuh's trace_unit, host and device code).  The round program is the same in every lane (len is a parameter of the call; only the flags differ, by at most one
// permutation and the T constant cells), the constants are read from the one spec buffer at wave-uniform indices, the state stays in
// registers (its loops are field.cuh's static_for: indexed by constants only), and every cell is one 32-byte store to the lane's own run of rows.  Every value of the trace IS a cell, so the arithmetic is
// the saturated, fully reduced Fr (fe_mul / fe_add) and a cell is stored as computed.  No LDS, no atomics, no workgroup waits for another.
#include "internal.h"
#include "host_field.h"
#include "poseidon_trace.cuh"
#include "trace_host.h"

namespace h2 {

constexpr uint32_t TRACE_BLOCK = 64;   // one wave per workgroup: a level of a 1,024-leaf tree (512 units) spreads over eight CUs' worth of SIMDs
constexpr uint32_t TRACE_FLAGS = H2HIP_POSEIDON_ABSORB_ONLY | H2HIP_POSEIDON_WITH_CONSTS;

static inline size_t popt_elems(uint32_t t, uint32_t r_f, uint32_t r_p) {
    return (size_t)r_f * t + r_p + 2 * (size_t)t * t + (size_t)r_p * (2 * t - 1) + 1;
}

// cells of one permutation that absorbs m <= RATE inputs: add (4) on s[0]; sum of three (7) per input; add (4) on the lanes behind; per full
// round T S-boxes (mul, mul, mul_add: 12) and T inner products (1 + 3 T); per partial round one S-box, one inner product, T - 1 mul_add (4)
static inline uint64_t trace_perm_cells(uint32_t t, uint32_t r_f, uint32_t r_p, uint32_t m) {
    const uint64_t ip = 1 + 3 * (uint64_t)t;
    return 4 + 7 * (uint64_t)m + 4 * (uint64_t)(t - 1 - m) + (uint64_t)r_f * (12 * t + t * ip) + (uint64_t)r_p * (12 + ip + 4 * (t - 1));
}
// the permutations of one unit: one per chunk of RATE, one more on the empty chunk when len is a multiple of RATE (unless ABSORB_ONLY)
static inline uint64_t trace_perms(uint32_t t, uint32_t len, uint32_t flags) {
    const uint32_t rate = t - 1;
    return (uint64_t)(len + rate - 1) / rate + ((len % rate == 0 && !(flags & H2HIP_POSEIDON_ABSORB_ONLY)) ? 1 : 0);
}
static inline uint64_t trace_unit_cells(uint32_t t, uint32_t r_f, uint32_t r_p, uint32_t len, uint32_t flags) {
    const uint32_t rate = t - 1;
    uint64_t cells = (flags & H2HIP_POSEIDON_WITH_CONSTS) ? t : 0;
    cells += (uint64_t)(len / rate) * trace_perm_cells(t, r_f, r_p, rate);
    if (len % rate) cells += trace_perm_cells(t, r_f, r_p, len % rate);
    else if (!(flags & H2HIP_POSEIDON_ABSORB_ONLY)) cells += trace_perm_cells(t, r_f, r_p, 0);
    return cells;
}

// inputs / states_in may point into the columns (at cells this call does not write: the host checked)
template <int T>
__global__ __launch_bounds__(TRACE_BLOCK) void poseidon_trace_kernel(TraceCols tc, const Fr *inputs, uint32_t len, const Fr *states_in, Fr *states_out,
                                                                     const h2hip_poseidon_hash *__restrict__ units, uint32_t count, PoseidonOptDev sp) {
    const uint32_t u = blockIdx.x * TRACE_BLOCK + threadIdx.x;
    if (u < count) trace_unit<T>(tc, inputs, len, states_in, states_out, units[u], u, sp);
}

// ------------------------------------------------------------------ the optimised spec (host)
struct PMat {   // t x t, row major
    uint32_t t;
    Fr m[25];
    Fr &at(uint32_t i, uint32_t j) { return m[i * t + j]; }
    const Fr &at(uint32_t i, uint32_t j) const { return m[i * t + j]; }
};
static PMat pmat_identity(uint32_t t) {
    PMat r;
    r.t = t;
    for (uint32_t i = 0; i < t * t; ++i) r.m[i] = Fr::zero();
    for (uint32_t i = 0; i < t; ++i) r.at(i, i) = Fr::one();
    return r;
}
static PMat pmat_transpose(const PMat &a) {
    PMat r;
    r.t = a.t;
    for (uint32_t i = 0; i < a.t; ++i)
        for (uint32_t j = 0; j < a.t; ++j) r.at(i, j) = a.at(j, i);
    return r;
}
static PMat pmat_mul(const PMat &a, const PMat &b) {
    PMat r;
    r.t = a.t;
    for (uint32_t i = 0; i < a.t; ++i)
        for (uint32_t j = 0; j < a.t; ++j) {
            Fr acc = Fr::zero();
            for (uint32_t k = 0; k < a.t; ++k) acc = fe_add(acc, fe_mul(a.at(i, k), b.at(k, j)));
            r.at(i, j) = acc;
        }
    return r;
}
static void pmat_mul_vector(const PMat &a, const Fr *v, Fr *out) {
    for (uint32_t i = 0; i < a.t; ++i) {
        Fr acc = Fr::zero();
        for (uint32_t j = 0; j < a.t; ++j) acc = fe_add(acc, fe_mul(a.at(i, j), v[j]));
        out[i] = acc;
    }
}
// Gauss-Jordan; false when the matrix is singular
static bool pmat_inverse(const PMat &a, PMat *out) {
    const uint32_t t = a.t;
    PMat w = a, inv = pmat_identity(t);
    for (uint32_t c = 0; c < t; ++c) {
        uint32_t p = c;
        while (p < t && w.at(p, c).is_zero()) ++p;
        if (p == t) return false;
        for (uint32_t j = 0; j < t; ++j) {
            std::swap(w.at(p, j), w.at(c, j));
            std::swap(inv.at(p, j), inv.at(c, j));
        }
        const Fr d = fe_inv(w.at(c, c));
        for (uint32_t j = 0; j < t; ++j) {
            w.at(c, j) = fe_mul(w.at(c, j), d);
            inv.at(c, j) = fe_mul(inv.at(c, j), d);
        }
        for (uint32_t i = 0; i < t; ++i) {
            if (i == c) continue;
            const Fr f = w.at(i, c);
            for (uint32_t j = 0; j < t; ++j) {
                w.at(i, j) = fe_sub(w.at(i, j), fe_mul(f, w.at(c, j)));
                inv.at(i, j) = fe_sub(inv.at(i, j), fe_mul(f, inv.at(c, j)));
            }
        }
    }
    *out = inv;
    return true;
}
// factorise (mds.rs:118-171): M = M' * M'' with M' = [[1, 0], [0, m_hat]]; M'' is returned as row = [m_00, w_hat...] (its first column) and
// col_hat = m_0,1.. (its first row behind m_00), w_hat = m_hat^-1 * w, w = the first column of M below m_00
static bool pmat_factorise(const PMat &m, PMat *m_prime, Fr *row, Fr *col_hat) {
    const uint32_t t = m.t, rate = t - 1;
    PMat hat;
    hat.t = rate;
    for (uint32_t i = 0; i < rate; ++i)
        for (uint32_t j = 0; j < rate; ++j) hat.at(i, j) = m.at(i + 1, j + 1);
    PMat hat_inv;
    if (!pmat_inverse(hat, &hat_inv)) return false;
    Fr w[4];
    for (uint32_t i = 0; i < rate; ++i) w[i] = m.at(i + 1, 0);
    row[0] = m.at(0, 0);
    pmat_mul_vector(hat_inv, w, row + 1);
    for (uint32_t j = 0; j < rate; ++j) col_hat[j] = m.at(0, j + 1);
    *m_prime = pmat_identity(t);
    for (uint32_t i = 0; i < rate; ++i)
        for (uint32_t j = 0; j < rate; ++j) m_prime->at(i + 1, j + 1) = hat.at(i, j);
    return true;
}
static bool trace_spec_ok(uint32_t t, uint32_t r_f, uint32_t r_p) {
    return (t == 3 || t == 5) && r_f >= 2 && (r_f % 2) == 0 && r_f <= 16 && r_p <= 256;
}
// inner_product_simple takes another cell form when its right operand starts with Constant(1) (flex_gate/mod.rs:953-962)
static const char *const ROW_ONE_MSG =
    "a matrix row (mds, pre_sparse_mds or a sparse row) begins with 1: inner_product_simple writes another cell form for it "
    "(flex_gate/mod.rs:953-962), which the fill does not write";
static bool row_starts_with_one(const void *rows, size_t nrows, size_t row_len) {
    const Fr one = Fr::one();
    for (size_t i = 0; i < nrows; ++i)
        if (ld_fr((const char *)rows + sizeof(Fr) * i * row_len) == one) return true;
    return false;
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2hip_poseidon_spec_optimize(uint32_t t, uint32_t r_f, uint32_t r_p, const void *round_constants, const void *mds, void *start_out, void *partial_out,
                                 void *end_out, void *pre_sparse_mds_out, void *sparse_out) {
    H2_REQUIRE(round_constants && mds && start_out && partial_out && end_out && pre_sparse_mds_out && sparse_out, "NULL argument");
    H2_REQUIRE(t == 3 || t == 5, "state width t must be 3 or 5");
    H2_REQUIRE(trace_spec_ok(t, r_f, r_p), "round numbers out of range");
    const uint32_t half = r_f / 2, rounds = r_f + r_p;
    std::vector<Fr> rc((size_t)rounds * t);
    for (size_t j = 0; j < rc.size(); ++j) rc[j] = ld_fr((const char *)round_constants + sizeof(Fr) * j);
    PMat m;
    m.t = t;
    for (uint32_t j = 0; j < t * t; ++j) m.m[j] = ld_fr((const char *)mds + sizeof(Fr) * j);
    PMat inv;
    H2_REQUIRE(pmat_inverse(m, &inv), "the MDS matrix is singular");
    // ---- calculate_optimized_constants (spec.rs:108-157)
    std::vector<Fr> start((size_t)(half + 1) * t), partial(r_p), end((size_t)(half - 1) * t);
    for (uint32_t k = 0; k < t; ++k) start[k] = rc[k];
    for (uint32_t r = 1; r < half; ++r) pmat_mul_vector(inv, &rc[(size_t)r * t], &start[(size_t)r * t]);
    Fr acc[5], tmp[5];
    for (uint32_t k = 0; k < t; ++k) acc[k] = rc[(size_t)(half + r_p) * t + k];
    for (uint32_t i = 0; i < r_p; ++i) {   // partial[r_p - 1 - i] with the constants of round half + r_p - 1 - i
        pmat_mul_vector(inv, acc, tmp);
        partial[r_p - 1 - i] = tmp[0];
        tmp[0] = Fr::zero();
        const Fr *c = &rc[(size_t)(half + r_p - 1 - i) * t];
        for (uint32_t k = 0; k < t; ++k) acc[k] = fe_add(tmp[k], c[k]);
    }
    pmat_mul_vector(inv, acc, &start[(size_t)half * t]);
    for (uint32_t r = 0; r + 1 < half; ++r) pmat_mul_vector(inv, &rc[(size_t)(half + r_p + 1 + r) * t], &end[(size_t)r * t]);
    // ---- calculate_sparse_matrices (spec.rs:159-175)
    const PMat mt = pmat_transpose(m);
    PMat a = mt;
    std::vector<Fr> sparse((size_t)r_p * (2 * t - 1));
    for (uint32_t i = 0; i < r_p; ++i) {
        PMat mp;
        Fr *dst = &sparse[(size_t)(r_p - 1 - i) * (2 * t - 1)];   // (the list is reversed)
        H2_REQUIRE(pmat_factorise(a, &mp, dst, dst + t), "a sub-matrix of the MDS matrix is singular");
        a = pmat_mul(mt, mp);
    }
    const PMat pre = pmat_transpose(a);
    H2_REQUIRE(!row_starts_with_one(m.m, t, t) && !row_starts_with_one(pre.m, t, t) && !row_starts_with_one(sparse.data(), r_p, 2 * t - 1), ROW_ONE_MSG);
    memcpy(start_out, start.data(), sizeof(Fr) * start.size());
    if (r_p) memcpy(partial_out, partial.data(), sizeof(Fr) * partial.size());
    if (half > 1) memcpy(end_out, end.data(), sizeof(Fr) * end.size());
    memcpy(pre_sparse_mds_out, pre.m, sizeof(Fr) * t * t);
    if (r_p) memcpy(sparse_out, sparse.data(), sizeof(Fr) * sparse.size());
    return H2HIP_OK;
}

int h2hip_poseidon_set_optimized_spec(h2hip_ctx *ctx, uint32_t t, uint32_t r_f, uint32_t r_p, const void *start, const void *partial, const void *end,
                                      const void *mds, const void *pre_sparse_mds, const void *sparse) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && start && partial && end && mds && pre_sparse_mds && sparse, "NULL argument");
    H2_REQUIRE(t == 3 || t == 5, "state width t must be 3 or 5");
    H2_REQUIRE(trace_spec_ok(t, r_f, r_p), "round numbers out of range");
    H2_REQUIRE(!row_starts_with_one(mds, t, t) && !row_starts_with_one(pre_sparse_mds, t, t) && !row_starts_with_one(sparse, r_p, 2 * t - 1),
               ROW_ONE_MSG);
    const uint32_t half = r_f / 2;
    const size_t n = popt_elems(t, r_f, r_p);
    std::vector<Fr> buf;
    buf.reserve(n);
    auto push = [&](const void *src, size_t cnt) {
        for (size_t j = 0; j < cnt; ++j) buf.push_back(ld_fr((const char *)src + sizeof(Fr) * j));
    };
    push(start, (size_t)(half + 1) * t);
    push(partial, r_p);
    push(end, (size_t)(half - 1) * t);
    push(mds, (size_t)t * t);
    push(pre_sparse_mds, (size_t)t * t);
    push(sparse, (size_t)r_p * (2 * t - 1));
    Fr two64 = Fr::zero();
    two64.l[2] = 1u;
    buf.push_back(fe_to_mont(two64));
    Fr *dev = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_POSEIDON_OPT, sizeof(Fr) * n, (void **)&dev));
    ctx->popt_t = 0;
    H2_HIPCHK(hipMemcpyAsync(dev, buf.data(), sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->stream));
    H2_HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->popt_t = t;
    ctx->popt_rf = r_f;
    ctx->popt_rp = r_p;
    return H2HIP_OK;
}

int h2hip_poseidon_trace_layout(uint32_t t, uint32_t r_f, uint32_t r_p, uint32_t len, uint32_t flags, size_t *num_cells, uint32_t *state_out_offsets) {
    H2_REQUIRE(num_cells && state_out_offsets, "NULL argument");
    H2_REQUIRE(t == 3 || t == 5, "state width t must be 3 or 5");
    H2_REQUIRE(trace_spec_ok(t, r_f, r_p), "round numbers out of range");
    H2_REQUIRE((flags & ~TRACE_FLAGS) == 0, "unknown flags");
    H2_REQUIRE(trace_perms(t, len, flags) >= 1, "a unit without a permutation (len == 0 with ABSORB_ONLY)");
    const uint64_t cells = trace_unit_cells(t, r_f, r_p, len, flags);
    H2_REQUIRE(cells < ((uint64_t)1 << 31), "a unit of 2^31 cells or more");
    *num_cells = (size_t)cells;
    // the final state: the last cells of the T inner products of the last apply_mds
    for (uint32_t i = 0; i < t; ++i) state_out_offsets[i] = (uint32_t)(cells - (uint64_t)(t - 1 - i) * (1 + 3 * t) - 1);
    return H2HIP_OK;
}

int h2hip_poseidon_fill_hashes_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                                   const void *inputs_dev, size_t inputs_len, uint32_t len, const void *states_in_dev, void *states_out_dev,
                                   const h2hip_poseidon_hash *hashes_host, size_t count) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (count == 0 || (hashes_host && columns_dev && (inputs_dev || len == 0))), "NULL argument");
    H2_REQUIRE(count < 0xFFFFFFFFu, "too many units");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched or uploaded
    H2_REQUIRE(ctx->popt_t != 0, "no optimised spec set: call h2hip_poseidon_set_optimized_spec first");
    TraceRuns runs{columns_dev, num_columns, usable_rows, break_points_host};
    const char *bad = runs.args_bad(SIZE_MAX);   // (this fill has never bounded usable_rows: its rows are the units' own)
    H2_REQUIRE(!bad, bad);
    H2_REQUIRE(inputs_len <= SIZE_MAX / sizeof(Fr), "inputs_len is no count of field elements");
    const uint32_t t = ctx->popt_t, r_f = ctx->popt_rf, r_p = ctx->popt_rp;
    std::vector<ByteRange> in_reads, st_reads;
    runs.written.reserve(count + 8);
    in_reads.reserve(count);
    for (size_t j = 0; j < count; ++j) {
        const h2hip_poseidon_hash &h = hashes_host[j];
        H2_REQUIRE((h.flags & ~TRACE_FLAGS) == 0, "unknown flags");
        H2_REQUIRE(trace_perms(t, len, h.flags) >= 1, "a unit without a permutation (len == 0 with ABSORB_ONLY)");
        const uint64_t cells = trace_unit_cells(t, r_f, r_p, len, h.flags);
        H2_REQUIRE(cells < ((uint64_t)1 << 31), "a unit of 2^31 cells or more");
        bad = runs.run(h.column, h.row, cells);
        H2_REQUIRE(!bad, bad);
        // input indices in 64 bits: (len - 1) * stride < 2^64, and the sum is checked against inputs_len without wrapping
        H2_REQUIRE(!len || operand_range(inputs_dev, inputs_len, h.input_offset, (uint64_t)(len - 1) * h.input_stride, in_reads),
                   "a unit's inputs lie outside inputs_len");
    }
    const size_t st_bytes = sizeof(Fr) * count * t;
    if (states_out_dev) runs.written.push_back(ByteRange{(uintptr_t)states_out_dev, (uintptr_t)states_out_dev + st_bytes});
    if (states_in_dev) st_reads.push_back(ByteRange{(uintptr_t)states_in_dev, (uintptr_t)states_in_dev + st_bytes});
    bad = byte_ranges_clash(runs.written, {&in_reads, &st_reads}, "two units' cells overlap (or a unit's cells and states_out_dev)");
    H2_REQUIRE(!bad, bad);
    // ---- tables: [unit table][column pointers][break points]
    DevTables tabs;
    H2_CHK(pack_tables(ctx, {{hashes_host, sizeof(h2hip_poseidon_hash) * count}, columns_table(runs), breaks_table(runs)}, tabs));
    const Fr *base = (const Fr *)ctx->ws[h2hip_ctx::WS_POSEIDON_OPT].p;
    const uint32_t half = r_f / 2;
    PoseidonOptDev sp;
    sp.start = base;
    sp.partial = sp.start + (size_t)(half + 1) * t;
    sp.end = sp.partial + r_p;
    sp.mds = sp.end + (size_t)(half - 1) * t;
    sp.pre = sp.mds + (size_t)t * t;
    sp.sparse = sp.pre + (size_t)t * t;
    sp.init0 = sp.sparse + (size_t)r_p * (2 * t - 1);
    sp.half = half;
    sp.r_p = r_p;
    const dim3 grid((uint32_t)((count + TRACE_BLOCK - 1) / TRACE_BLOCK)), blk(TRACE_BLOCK);
    prof_begin(ctx, "poseidon_trace_kernel");
    if (t == 3)
        hipLaunchKernelGGL(poseidon_trace_kernel<3>, grid, blk, 0, ctx->stream, tabs.tc, (const Fr *)inputs_dev, len, (const Fr *)states_in_dev,
                           (Fr *)states_out_dev, (const h2hip_poseidon_hash *)tabs.at[0], (uint32_t)count, sp);
    else
        hipLaunchKernelGGL(poseidon_trace_kernel<5>, grid, blk, 0, ctx->stream, tabs.tc, (const Fr *)inputs_dev, len, (const Fr *)states_in_dev,
                           (Fr *)states_out_dev, (const h2hip_poseidon_hash *)tabs.at[0], (uint32_t)count, sp);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

}  // extern "C"
