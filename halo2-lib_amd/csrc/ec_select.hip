// EccChip's point selections and GateChip::num_to_bits filled on the device: every gate cell ec_select writes (select::crt for x and y, one
// GateChip::select per limb and native cell), every cell of ec_select_from_bits (bits_to_indicator, then select_by_indicator::crt for x and y
// with its evaluate_native) and every cell of num_to_bits (the inner product against the powers of two, then assert_bit per bit), for points,
// tables, selectors and scalars lying on the device (halo2-ecc/src/ecc/mod.rs:402-456, bigint/select.rs:26-50, bigint/select_by_indicator.rs:29-69,
// halo2-base/src/gates/flex_gate/mod.rs:609-656, :1144-1170, :1215-1241; include/h2hip.h states the cell form).  With them every cell of
// multi_scalar_multiply's window loop is written on the device, and the selected point is left in results_dev as the operand the strict
// addition behind it reads.
//
// The selections are a fused unit (trace_host.h's fused_fill), their code in ec_select.cuh as host and device code.  ec_select_solve_kernel:
// one lane per unit, Fr arithmetic only (2^(w+1) - 4 products for the indicator, one per table entry and chain).  ec_select_place_kernel: one
// lane per (unit, segment); a lane of a chain piece starts from the sum the solve kernel left for it, so no lane waits for another.
// num_to_bits_kernel: one lane per (unit, bit); the sums are bit masks of the value, as in range_fill.hip.  No LDS, no atomics, no workgroup
// waits for another.
#include "internal.h"
#include "ec_select.cuh"
#include "trace_host.h"

namespace h2 {

constexpr uint32_t SEL_SOLVE_BLOCK = 64, SEL_PLACE_BLOCK = 256, BITS_BLOCK = 256;

static_assert(sizeof(h2hip_ec_select) == 32 && sizeof(h2hip_bits_unit) == 16, "the unit tables are uploaded as the caller laid them out");

__global__ __launch_bounds__(SEL_SOLVE_BLOCK) void ec_select_solve_kernel(SelCall sc, const h2hip_ec_select *__restrict__ units, uint32_t count) {
    const uint32_t u = blockIdx.x * SEL_SOLVE_BLOCK + threadIdx.x;
    if (u >= count) return;
    sel_solve_unit(sc, units[u], u);
}
// sc.values may point into the columns or at an earlier call's results (at cells this call does not write: the host checked)
__global__ __launch_bounds__(SEL_PLACE_BLOCK) void ec_select_place_kernel(SelCall sc, const h2hip_ec_select *__restrict__ units, uint32_t slots, uint64_t lanes) {
    const uint64_t g = (uint64_t)blockIdx.x * SEL_PLACE_BLOCK + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t u = (uint32_t)(g / slots);
    sel_place_slot(sc, units[u], u, (uint32_t)(g - (uint64_t)u * slots));
}
__global__ __launch_bounds__(BITS_BLOCK) void num_to_bits_kernel(BitsCall bc, const h2hip_bits_unit *__restrict__ units, uint64_t lanes) {
    const uint64_t g = (uint64_t)blockIdx.x * BITS_BLOCK + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t u = (uint32_t)(g / bc.nb);
    bits_slot(bc, units[u], u, (uint32_t)(g - (uint64_t)u * bc.nb));
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2hip_ec_select_layout(const h2hip_fp_params *params, uint32_t op, uint32_t window_bits, size_t *num_cells, uint32_t *out_cell_offsets) {
    H2_REQUIRE(params && num_cells && out_cell_offsets, "NULL argument");
    SelShape sh;
    const char *bad = sel_prepare(*params, op, window_bits, sh, nullptr, nullptr);
    H2_REQUIRE(!bad, bad);
    *num_cells = sh.total;
    for (uint32_t j = 0; j < sel_result_len(sh.k); ++j) out_cell_offsets[j] = sh.out_offsets[j];
    return H2HIP_OK;
}

int h2hip_ec_select_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                             const h2hip_fp_params *params, uint32_t op, uint32_t window_bits, const void *values_dev, size_t values_len,
                             void *results_dev, size_t results_len, const h2hip_ec_select *units_host, size_t count) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "NULL argument");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched or uploaded
    H2_REQUIRE(columns_dev && params && values_dev && units_host, "NULL argument");
    SelShape sh;
    SelCall sc;
    Fr consts[FP_CONSTS];
    const char *bad = sel_prepare(*params, op, window_bits, sh, &sc, consts);
    H2_REQUIRE(!bad, bad);
    const uint32_t point = sel_result_len(sh.k);
    const bool from_bits = op == H2HIP_EC_SELECT_FROM_BITS;
    // a point and Q and sel, or the packed table and the w bits
    const FusedKind kind{__func__, sh.total, sel_unit_slots(sc), point, sel_record_len(sc),
                         {{true, from_bits ? sc.m * point - 1 : point - 1}, {!from_bits, point - 1}, {true, from_bits ? sc.w - 1 : 0}},
                         {consts, sizeof(Fr) * FP_CONSTS}, {nullptr, 0}, "ec_select_solve_kernel", "ec_select_place_kernel", SEL_SOLVE_BLOCK, SEL_PLACE_BLOCK};
    return fused_fill(
        ctx, columns_dev, num_columns, usable_rows, break_points_host, values_dev, values_len, results_dev, results_len, units_host, count, kind, sc,
        [&](dim3 grid, const h2hip_ec_select *units, const void *) {
            hipLaunchKernelGGL(ec_select_solve_kernel, grid, dim3(SEL_SOLVE_BLOCK), 0, ctx->stream, sc, units, (uint32_t)count);
        },
        [&](dim3 grid, const h2hip_ec_select *units, uint32_t slots, uint64_t lanes) {
            hipLaunchKernelGGL(ec_select_place_kernel, grid, dim3(SEL_PLACE_BLOCK), 0, ctx->stream, sc, units, slots, lanes);
        });
}

int h2hip_num_to_bits_layout(uint32_t num_bits, size_t *num_cells, uint32_t *sum_cell_offset) {
    H2_REQUIRE(num_cells && sum_cell_offset, "NULL argument");
    H2_REQUIRE(num_bits >= 1 && num_bits <= BITS_MAX, "num_bits outside 1 .. 254");
    *num_cells = bits_unit_cells(num_bits);
    *sum_cell_offset = 3 * num_bits - 3;
    return H2HIP_OK;
}

int h2hip_num_to_bits_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                               const void *values_dev, size_t values_len, void *results_dev, size_t results_len, uint32_t num_bits,
                               const h2hip_bits_unit *units_host, size_t count) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "NULL argument");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched or uploaded
    H2_REQUIRE(columns_dev && values_dev && units_host, "NULL argument");
    H2_REQUIRE(num_bits >= 1 && num_bits <= BITS_MAX, "num_bits outside 1 .. 254");
    H2_REQUIRE(count <= ((uint64_t)1 << 32) / num_bits, "more than 2^32 lanes (count * num_bits) in one call");
    TraceRuns runs{columns_dev, num_columns, usable_rows, break_points_host};
    const char *bad = runs.args_bad();
    H2_REQUIRE(!bad, bad);
    H2_REQUIRE(values_len <= SIZE_MAX / sizeof(Fr) && results_len <= SIZE_MAX / sizeof(Fr), "values_len / results_len is no count of field elements");
    H2_REQUIRE(!results_dev || results_len / num_bits >= count, "results_len < count * num_bits");
    const uint32_t cells = bits_unit_cells(num_bits);
    std::vector<ByteRange> reads;
    runs.written.reserve(count + 9);
    reads.reserve(count);
    for (size_t j = 0; j < count; ++j) {
        const h2hip_bits_unit &u = units_host[j];
        bad = runs.run(u.column, u.row, cells);
        H2_REQUIRE(!bad, bad);
        H2_REQUIRE(operand_range(values_dev, values_len, u.a_offset, 0, reads), "a unit's operand lies outside values_len");
    }
    // two units' cells are disjoint; the results lie in none of them; no value lies in anything written.  Address intervals, sorted and swept.
    bad = byte_ranges_clash(runs.written, {}, "two units' cells overlap (break copies included)");
    H2_REQUIRE(!bad, bad);
    if (results_dev) runs.written.push_back(ByteRange{(uintptr_t)results_dev, (uintptr_t)results_dev + sizeof(Fr) * num_bits * count});
    bad = byte_ranges_clash(runs.written, {&reads}, "the results overlap cells this call writes");
    H2_REQUIRE(!bad, bad);
    DevTables t;
    H2_CHK(pack_tables(ctx, {{units_host, sizeof(h2hip_bits_unit) * count}, columns_table(runs), breaks_table(runs)}, t));
    const BitsCall bc{t.tc, (const Fr *)values_dev, (Fr *)results_dev, num_bits};
    const uint64_t lanes = (uint64_t)count * num_bits;
    prof_begin(ctx, "num_to_bits_kernel");
    hipLaunchKernelGGL(num_to_bits_kernel, dim3((uint32_t)((lanes + BITS_BLOCK - 1) / BITS_BLOCK)), dim3(BITS_BLOCK), 0, ctx->stream, bc,
                       (const h2hip_bits_unit *)t.at[0], lanes);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

}  // extern "C"
