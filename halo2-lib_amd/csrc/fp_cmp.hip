// FpChip's comparisons filled on the device: every gate cell that enforce_less_than_p writes for one or both of two CRT integers lying on
// the device and that big_is_equal::assign writes for the pair — gate.add of the borrow, is_less_than's seven cells, is_zero, gate.sub,
// gate.and — except the cells of the k range checks per enforced operand, which are left as gaps for h2hip_range_fill_checks_dev
// (halo2-ecc/src/fields/fp.rs:123-142, bigint/big_is_equal.rs, halo2-base/src/gates/range/mod.rs:646-687, flex_gate/mod.rs:789-823;
// include/h2hip.h states the cell form).  The unit sits in front of a curve operation where the reference's check_points_are_unequal
// puts it (ecc/mod.rs:183-202).
//
// Two kernels on the context's stream, their code in fp_cmp.cuh as host and device code.  fp_cmp_solve_kernel: one lane per unit, Fr
// additions and one limb extraction per cell, no inversion.  fp_cmp_place_kernel: one lane per (unit, segment); the lane of an is_zero
// segment inverts its own cell (up to 3 k independent inversions per unit, none waiting for another).  No LDS, no atomics, no workgroup
// waits for another.
#include "internal.h"
#include "fp_cmp.cuh"
#include "trace_host.h"

namespace h2 {

constexpr uint32_t CMP_SOLVE_BLOCK = 64, CMP_PLACE_BLOCK = 256;

static_assert(sizeof(CmpSeg) == 8, "the segment table is uploaded as the host laid it out");

__global__ __launch_bounds__(CMP_SOLVE_BLOCK) void fp_cmp_solve_kernel(CmpCall cc, const h2hip_fp_mul *__restrict__ units, uint32_t count) {
    const uint32_t u = blockIdx.x * CMP_SOLVE_BLOCK + threadIdx.x;
    if (u >= count) return;
    cmp_solve_unit(cc, units[u], u);
}
// cc.values may point into the columns or at an earlier call's results (at cells this call does not write: the host checked)
__global__ __launch_bounds__(CMP_PLACE_BLOCK) void fp_cmp_place_kernel(CmpCall cc, const h2hip_fp_mul *__restrict__ units, uint32_t slots, uint64_t lanes) {
    const uint64_t g = (uint64_t)blockIdx.x * CMP_PLACE_BLOCK + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t u = (uint32_t)(g / slots);
    cmp_place_slot(cc, units[u], u, (uint32_t)(g - (uint64_t)u * slots));
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2hip_fp_cmp_layout(const h2hip_fp_params *params, uint32_t op, size_t *num_cells, size_t *num_own_cells, size_t *num_lookup_cells,
                        size_t *results_per_unit, h2hip_fp_mul_range *ranges, uint32_t *out_cell_offsets) {
    H2_REQUIRE(params && num_cells && num_own_cells && num_lookup_cells && results_per_unit && ranges && out_cell_offsets, "NULL argument");
    CmpShape sh;
    const char *bad = cmp_prepare(*params, op, sh, nullptr, nullptr);
    H2_REQUIRE(!bad, bad);
    unit_layout_out(sh, num_cells, num_own_cells, num_lookup_cells, ranges);
    *results_per_unit = cmp_result_len(sh.k, op);
    for (uint32_t j = 0; j < 3; ++j) out_cell_offsets[j] = sh.out_offsets[j];
    return H2HIP_OK;
}

int h2hip_fp_cmp_range_checks(const uint32_t *break_points_host, size_t num_columns, const h2hip_fp_params *params, uint32_t op,
                              const h2hip_fp_mul *units_host, const uint64_t *lookup_slots_host, size_t count, h2hip_range_check *checks_out) {
    if (!count) return H2HIP_OK;
    H2_REQUIRE(params && units_host && lookup_slots_host && checks_out, "NULL argument");
    CmpShape sh;
    const char *bad = cmp_prepare(*params, op, sh, nullptr, nullptr);
    H2_REQUIRE(!bad, bad);
    // one width; unit-major: rows and lookup slots ascend with the units
    const uint32_t ngaps = sh.ngaps;
    return fp_gap_checks(break_points_host, num_columns, sh, cmp_result_len(sh.k, op), units_host, lookup_slots_host, count, checks_out,
                         [ngaps](size_t u, uint32_t j) { return u * ngaps + j; });
}

int h2hip_fp_cmp_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                          const h2hip_fp_params *params, uint32_t op, const void *values_dev, size_t values_len, void *results_dev, size_t results_len,
                          const h2hip_fp_mul *units_host, size_t count) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "NULL argument");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched or uploaded
    H2_REQUIRE(columns_dev && params && values_dev && units_host, "NULL argument");
    CmpShape sh;
    CmpCall cc;
    Fr consts[CMP_CONSTS];
    const char *bad = cmp_prepare(*params, op, sh, &cc, consts);
    H2_REQUIRE(!bad, bad);
    const uint32_t k = sh.k;
    const bool reads_a = op & (H2HIP_FP_CMP_REDUCE_A | H2HIP_FP_CMP_EQUAL), reads_b = op & (H2HIP_FP_CMP_REDUCE_B | H2HIP_FP_CMP_EQUAL);
    const FusedKind kind{__func__, sh.total, sh.nsegs, cmp_result_len(k, op), cmp_record_len(k), {{reads_a, k}, {reads_b, k}}, {consts, sizeof(Fr) * CMP_CONSTS},
                         {sh.segs, sizeof(CmpSeg) * sh.nsegs}, "fp_cmp_solve_kernel", "fp_cmp_place_kernel", CMP_SOLVE_BLOCK, CMP_PLACE_BLOCK};
    return fused_fill(
        ctx, columns_dev, num_columns, usable_rows, break_points_host, values_dev, values_len, results_dev, results_len, units_host, count, kind, cc,
        [&](dim3 grid, const h2hip_fp_mul *units, const void *segs) {
            cc.segs = (const CmpSeg *)segs;
            hipLaunchKernelGGL(fp_cmp_solve_kernel, grid, dim3(CMP_SOLVE_BLOCK), 0, ctx->stream, cc, units, (uint32_t)count);
        },
        [&](dim3 grid, const h2hip_fp_mul *units, uint32_t slots, uint64_t lanes) {
            hipLaunchKernelGGL(fp_cmp_place_kernel, grid, dim3(CMP_PLACE_BLOCK), 0, ctx->stream, cc, units, slots, lanes);
        });
}

}  // extern "C"
