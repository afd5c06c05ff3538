// FpChip::mul filled on the device: every gate cell that mul_no_carry::crt and carry_mod::crt (with check_carry_to_zero::truncate and two
// evaluate_native) write for two proper CRT integers lying on the device, except the cells of their nine range checks, which are left as gaps
// for h2hip_range_fill_checks_dev (halo2-ecc/src/fields/mod.rs:188-196, bigint/mul_no_carry.rs, bigint/carry_mod.rs,
// bigint/check_carry_to_zero.rs, bigint/mod.rs:66-74; include/h2hip.h states the cell form).
//
// Two kernels on the context's stream, their code in fp_mul.cuh as host and device code.  fp_mul_solve_kernel: one lane per unit does the
// big-integer step once — the 2 n k-bit product, the division by p (Barrett: p and mu = floor(2^S / p) are wave-uniform kernel arguments, the
// correction a bounded loop), the limbs of quotient and remainder, P_i / prod_i / check_i in Fr, the signed carry chain — and stores a record
// of 5 k + 3 Fr per unit and the results entries.  k is a template parameter: every limb array is indexed by compile-time constants.
// fp_mul_place_kernel: one lane per (unit, slot), 4 k + 3 slots, recomputes the slot's running sums from the operands and the record (at
// most k products) and writes its cells through TraceOut; neighbouring lanes write neighbouring groups of cells.  No LDS, no atomics, no
// workgroup waits for another.
#include "internal.h"
#include "fp_mul.cuh"
#include "trace_host.h"

namespace h2 {

constexpr uint32_t FP_SOLVE_BLOCK = 64, FP_PLACE_BLOCK = 256;

static_assert(sizeof(h2hip_fp_mul) == 24 && sizeof(h2hip_fp_params) == 64, "the tables are uploaded / read as the caller laid them out");

template <int K>
__global__ __launch_bounds__(FP_SOLVE_BLOCK) void fp_mul_solve_kernel(FpCall fc, const h2hip_fp_mul *__restrict__ units, uint32_t count) {
    const uint32_t u = blockIdx.x * FP_SOLVE_BLOCK + threadIdx.x;
    if (u >= count) return;
    fp_solve_unit<K>(fc, units[u], u);
}
// fc.values may point into the columns or at an earlier call's results (at cells this call does not write: the host checked)
__global__ __launch_bounds__(FP_PLACE_BLOCK) void fp_mul_place_kernel(FpCall fc, const h2hip_fp_mul *__restrict__ units, uint32_t slots, uint64_t lanes) {
    const uint64_t g = (uint64_t)blockIdx.x * FP_PLACE_BLOCK + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t u = (uint32_t)(g / slots);
    fp_place_slot(fc, units[u], u, (uint32_t)(g - (uint64_t)u * slots));
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2hip_fp_mul_layout(const h2hip_fp_params *params, size_t *num_cells, size_t *num_own_cells, size_t *num_lookup_cells, h2hip_fp_mul_range *ranges,
                        uint32_t *out_cell_offsets) {
    H2_REQUIRE(params && num_cells && num_own_cells && num_lookup_cells && ranges && out_cell_offsets, "NULL argument");
    FpShape sh;
    const char *bad = fp_prepare(*params, sh, nullptr, nullptr);
    H2_REQUIRE(!bad, bad);
    const uint32_t k = sh.k;
    unit_layout_out(sh, num_cells, num_own_cells, num_lookup_cells, ranges);
    for (uint32_t i = 0; i < k; ++i) out_cell_offsets[i] = sh.lay.base3 + fp_tri(i) + 10 * i + 3 * (i + 1) + 1 + 4;   // o_i: the fifth cell behind prod_i
    out_cell_offsets[k] = sh.lay.off9 - 1;   // out_native: the last cell of S8
    return H2HIP_OK;
}

int h2hip_fp_mul_range_checks(const uint32_t *break_points_host, size_t num_columns, const h2hip_fp_params *params, const h2hip_fp_mul *units_host,
                              const uint64_t *lookup_slots_host, size_t count, h2hip_range_check *checks_out) {
    if (!count) return H2HIP_OK;
    H2_REQUIRE(params && units_host && lookup_slots_host && checks_out, "NULL argument");
    FpShape sh;
    const char *bad = fp_prepare(*params, sh, nullptr, nullptr);
    H2_REQUIRE(!bad, bad);
    // gap-major: the gaps of one width are consecutive
    return fp_gap_checks(break_points_host, num_columns, sh, fp_result_len(sh.k), units_host, lookup_slots_host, count, checks_out,
                         [count](size_t u, uint32_t j) { return (size_t)j * count + u; });
}

int h2hip_fp_mul_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                          const h2hip_fp_params *params, const void *values_dev, size_t values_len, void *results_dev, size_t results_len,
                          const h2hip_fp_mul *units_host, size_t count) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "NULL argument");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched or uploaded
    H2_REQUIRE(columns_dev && params && values_dev && units_host, "NULL argument");
    FpShape sh;
    FpCall fc;
    Fr consts[FP_CONSTS];
    const char *bad = fp_prepare(*params, sh, &fc, consts);
    H2_REQUIRE(!bad, bad);
    const uint32_t k = sh.k;
    const FusedKind kind{__func__, sh.total, fp_unit_slots(k), fp_result_len(k), fp_record_len(k), {{true, k}, {true, k}}, {consts, sizeof(Fr) * FP_CONSTS}, {nullptr, 0},
                         "fp_mul_solve_kernel", "fp_mul_place_kernel", FP_SOLVE_BLOCK, FP_PLACE_BLOCK};
    return fused_fill(
        ctx, columns_dev, num_columns, usable_rows, break_points_host, values_dev, values_len, results_dev, results_len, units_host, count, kind, fc,
        [&](dim3 grid, const h2hip_fp_mul *units, const void *) {
            if (k == 2)
                hipLaunchKernelGGL(fp_mul_solve_kernel<2>, grid, dim3(FP_SOLVE_BLOCK), 0, ctx->stream, fc, units, (uint32_t)count);
            else if (k == 3)
                hipLaunchKernelGGL(fp_mul_solve_kernel<3>, grid, dim3(FP_SOLVE_BLOCK), 0, ctx->stream, fc, units, (uint32_t)count);
            else
                hipLaunchKernelGGL(fp_mul_solve_kernel<4>, grid, dim3(FP_SOLVE_BLOCK), 0, ctx->stream, fc, units, (uint32_t)count);
        },
        [&](dim3 grid, const h2hip_fp_mul *units, uint32_t slots, uint64_t lanes) {
            hipLaunchKernelGGL(fp_mul_place_kernel, grid, dim3(FP_PLACE_BLOCK), 0, ctx->stream, fc, units, slots, lanes);
        });
}

}  // extern "C"
