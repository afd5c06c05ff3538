// EccChip's ec_add_unequal, ec_sub_unequal (both non-strict) and ec_double filled on the device: every gate cell the reference writes for one
// curve operation on points lying on the device — sub_no_carry / add_no_carry / scalar_mul_no_carry / mul_no_carry, divide_unsafe or
// neg_divide_unsafe (load_private of lambda and check_carry_mod_to_zero) and two carry_mod — except the cells of its 9 k range checks, which
// are left as gaps for h2hip_range_fill_checks_dev (halo2-ecc/src/ecc/mod.rs:153-179, :219-246, :302-327, fields/mod.rs:217-238, :256-277;
// include/h2hip.h states the cell form).
//
// Two kernels on the context's stream, their code in ec_fill.cuh as host and device code.  ec_solve_kernel: one lane per unit, templated on
// k and on the operation, does lambda's inversion mod p (division steps, the modulus a kernel argument) and the three signed floor divisions
// one after the other, each stage's cells going to the unit's record before the next stage begins.  ec_place_kernel: one lane per (unit,
// segment) writes a segment's cells through TraceOut from the record.  No LDS, no atomics, no workgroup waits for another.
#include "internal.h"
#include "ec_fill.cuh"
#include "trace_host.h"

namespace h2 {

constexpr uint32_t EC_SOLVE_BLOCK = 64, EC_PLACE_BLOCK = 256;

static_assert(sizeof(h2hip_ec_op) == 24 && sizeof(EcSeg) == 12, "the tables are uploaded / read as the host laid them out");

template <int K, uint32_t OP>
__global__ __launch_bounds__(EC_SOLVE_BLOCK) void ec_solve_kernel(EcCall ec, const h2hip_ec_op *__restrict__ units, uint32_t count) {
    const uint32_t u = blockIdx.x * EC_SOLVE_BLOCK + threadIdx.x;
    if (u >= count) return;
    ec_solve_unit<K, OP>(ec, units[u], u);
}
// ec.values may point into the columns or at an earlier call's results (at cells this call does not write: the host checked)
__global__ __launch_bounds__(EC_PLACE_BLOCK) void ec_place_kernel(EcCall ec, const h2hip_ec_op *__restrict__ units, uint32_t slots, uint64_t lanes) {
    const uint64_t g = (uint64_t)blockIdx.x * EC_PLACE_BLOCK + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t u = (uint32_t)(g / slots);
    ec_place_slot(ec, units[u], u, (uint32_t)(g - (uint64_t)u * slots));
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2hip_ec_layout(const h2hip_fp_params *params, uint32_t op, size_t *num_cells, size_t *num_own_cells, size_t *num_lookup_cells,
                    h2hip_fp_mul_range *ranges, uint32_t *out_cell_offsets) {
    H2_REQUIRE(params && num_cells && num_own_cells && num_lookup_cells && ranges && out_cell_offsets, "NULL argument");
    EcShape sh;
    const char *bad = ec_prepare(*params, op, sh, nullptr, nullptr);
    H2_REQUIRE(!bad, bad);
    unit_layout_out(sh, num_cells, num_own_cells, num_lookup_cells, ranges);
    for (uint32_t j = 0; j < 3 * (sh.k + 1); ++j) out_cell_offsets[j] = sh.out_offsets[j];
    return H2HIP_OK;
}

int h2hip_ec_range_checks(const uint32_t *break_points_host, size_t num_columns, const h2hip_fp_params *params, uint32_t op,
                          const h2hip_ec_op *units_host, const uint64_t *lookup_slots_host, size_t count, h2hip_range_check *checks_out) {
    if (!count) return H2HIP_OK;
    H2_REQUIRE(params && units_host && lookup_slots_host && checks_out, "NULL argument");
    EcShape sh;
    const char *bad = ec_prepare(*params, op, sh, nullptr, nullptr);
    H2_REQUIRE(!bad, bad);
    // width group by width group; inside a group unit-major: rows and lookup slots ascend with the units
    uint32_t width[EC_MAX_GAPS], group_of[EC_MAX_GAPS], gaps_in[EC_MAX_GAPS], rank[EC_MAX_GAPS], seen[EC_MAX_GAPS] = {0};
    const uint32_t ng = ec_width_groups(sh, width, group_of, gaps_in);
    size_t start[EC_MAX_GAPS];
    for (uint32_t g = 0; g < ng; ++g) start[g] = g ? start[g - 1] + (size_t)gaps_in[g - 1] * count : 0;
    for (uint32_t j = 0; j < sh.ngaps; ++j) rank[j] = seen[group_of[j]]++;
    return fp_gap_checks(break_points_host, num_columns, sh, ec_result_len(sh.k), units_host, lookup_slots_host, count, checks_out,
                         [&](size_t u, uint32_t j) { return start[group_of[j]] + u * gaps_in[group_of[j]] + rank[j]; });
}

int h2hip_ec_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                      const h2hip_fp_params *params, uint32_t op, const void *values_dev, size_t values_len, void *results_dev, size_t results_len,
                      const h2hip_ec_op *units_host, size_t count) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "NULL argument");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched or uploaded
    H2_REQUIRE(columns_dev && params && values_dev && units_host, "NULL argument");
    EcShape sh;
    EcCall ec;
    Fr consts[EC_CONSTS];
    const char *bad = ec_prepare(*params, op, sh, &ec, consts);
    H2_REQUIRE(!bad, bad);
    const uint32_t k = sh.k, point = 2 * (k + 1);
    const bool two = op != H2HIP_EC_DOUBLE, sub = op == H2HIP_EC_SUB_UNEQUAL;
    const FusedKind kind{__func__, sh.total, sh.nsegs, ec_result_len(k), ec_record_len(k), {{true, point - 1}, {two, point - 1}}, {consts, sizeof(Fr) * EC_CONSTS},
                         {sh.segs, sizeof(EcSeg) * sh.nsegs}, "ec_solve_kernel", "ec_place_kernel", EC_SOLVE_BLOCK, EC_PLACE_BLOCK};
    return fused_fill(
        ctx, columns_dev, num_columns, usable_rows, break_points_host, values_dev, values_len, results_dev, results_len, units_host, count, kind, ec,
        [&](dim3 grid, const h2hip_ec_op *units, const void *segs) {
            ec.segs = (const EcSeg *)segs;
            if (k == 3 && sub)
                hipLaunchKernelGGL((ec_solve_kernel<3, H2HIP_EC_SUB_UNEQUAL>), grid, dim3(EC_SOLVE_BLOCK), 0, ctx->stream, ec, units, (uint32_t)count);
            else if (sub)
                hipLaunchKernelGGL((ec_solve_kernel<4, H2HIP_EC_SUB_UNEQUAL>), grid, dim3(EC_SOLVE_BLOCK), 0, ctx->stream, ec, units, (uint32_t)count);
            else if (k == 3 && two)
                hipLaunchKernelGGL((ec_solve_kernel<3, H2HIP_EC_ADD_UNEQUAL>), grid, dim3(EC_SOLVE_BLOCK), 0, ctx->stream, ec, units, (uint32_t)count);
            else if (k == 3)
                hipLaunchKernelGGL((ec_solve_kernel<3, H2HIP_EC_DOUBLE>), grid, dim3(EC_SOLVE_BLOCK), 0, ctx->stream, ec, units, (uint32_t)count);
            else if (two)
                hipLaunchKernelGGL((ec_solve_kernel<4, H2HIP_EC_ADD_UNEQUAL>), grid, dim3(EC_SOLVE_BLOCK), 0, ctx->stream, ec, units, (uint32_t)count);
            else
                hipLaunchKernelGGL((ec_solve_kernel<4, H2HIP_EC_DOUBLE>), grid, dim3(EC_SOLVE_BLOCK), 0, ctx->stream, ec, units, (uint32_t)count);
        },
        [&](dim3 grid, const h2hip_ec_op *units, uint32_t slots, uint64_t lanes) {
            hipLaunchKernelGGL(ec_place_kernel, grid, dim3(EC_PLACE_BLOCK), 0, ctx->stream, ec, units, slots, lanes);
        });
}

}  // extern "C"
