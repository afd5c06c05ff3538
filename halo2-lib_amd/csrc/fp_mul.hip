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
    *num_cells = sh.lay.total;
    *num_own_cells = sh.own;
    *num_lookup_cells = sh.num_lookups;
    for (uint32_t i = 0; i < k; ++i) {
        const bool last = i == k - 1;
        // the gaps in context order: o_i (behind S3), q_i + B (behind its four cells), -c_i + 2^rb (behind its eight cells)
        ranges[i] = h2hip_fp_mul_range{sh.lay.base4 + i * sh.gap[0], sh.gap[last ? 1 : 0], sh.width[last ? 1 : 0], i};
        ranges[k + i] = h2hip_fp_mul_range{sh.lay.base5 + i * (4 + sh.gap[2]) + 4, sh.gap[last ? 3 : 2], sh.width[last ? 3 : 2], k + 1 + i};
        ranges[2 * k + i] = h2hip_fp_mul_range{sh.lay.base6 + i * (8 + sh.gap[4]) + 8, sh.gap[4], sh.width[4], 2 * k + 1 + i};
        out_cell_offsets[i] = sh.lay.base3 + fp_tri(i) + 10 * i + 3 * (i + 1) + 1 + 4;   // o_i: the fifth cell behind prod_i
    }
    out_cell_offsets[k] = sh.lay.off9 - 1;   // out_native: the last cell of S8
    return H2HIP_OK;
}

int h2hip_trace_seek(const uint32_t *break_points_host, size_t num_columns, uint32_t column, uint32_t row, uint64_t offset, uint32_t *column_out,
                     uint32_t *row_out) {
    H2_REQUIRE(column_out && row_out, "NULL argument");
    H2_REQUIRE(column < num_columns, "the column index is out of range");
    uint64_t c = column, r = row;
    while (break_points_host && c + 1 < num_columns && break_points_host[c] >= r && offset > break_points_host[c] - r) {
        offset -= break_points_host[c] - r + 1;   // up to and including the break cell; the cell behind it lies at row 1 of the next column
        ++c;
        r = 1;
    }
    H2_REQUIRE(offset <= 0xFFFFFFFFull - r, "the cell lies past every row");
    *column_out = (uint32_t)c;
    *row_out = (uint32_t)(r + offset);
    return H2HIP_OK;
}

int h2hip_fp_mul_range_checks(const uint32_t *break_points_host, size_t num_columns, const h2hip_fp_params *params, const h2hip_fp_mul *units_host,
                              const uint64_t *lookup_slots_host, size_t count, h2hip_range_check *checks_out) {
    if (!count) return H2HIP_OK;
    H2_REQUIRE(params && units_host && lookup_slots_host && checks_out, "NULL argument");
    FpShape sh;
    const char *bad = fp_prepare(*params, sh, nullptr, nullptr);
    H2_REQUIRE(!bad, bad);
    const uint32_t k = sh.k;
    uint32_t off[3 * FP_MAX_K], lk_before[3 * FP_MAX_K], res[3 * FP_MAX_K], lk = 0;
    for (uint32_t j = 0; j < 3 * k; ++j) {   // the gaps in context order, as h2hip_fp_mul_layout reports them
        const uint32_t i = j % k, grp = j / k, last = i == k - 1;
        off[j] = grp == 0 ? sh.lay.base4 + i * sh.gap[0] : grp == 1 ? sh.lay.base5 + i * (4 + sh.gap[2]) + 4 : sh.lay.base6 + i * (8 + sh.gap[4]) + 8;
        res[j] = grp == 0 ? i : grp == 1 ? k + 1 + i : 2 * k + 1 + i;
        lk_before[j] = lk;
        lk += sh.lookups[grp == 0 ? (last ? 1 : 0) : grp == 1 ? (last ? 3 : 2) : 4];
    }
    for (size_t u = 0; u < count; ++u)
        for (uint32_t j = 0; j < 3 * k; ++j) {
            h2hip_range_check &c = checks_out[(size_t)j * count + u];
            const int r = h2hip_trace_seek(break_points_host, num_columns, units_host[u].column, units_host[u].row, off[j], &c.column, &c.row);
            if (r != H2HIP_OK) return r;
            c.a_offset = (uint64_t)u * fp_result_len(k) + res[j];
            c.b_offset = 0;
            c.lookup_slot = lookup_slots_host[u] + lk_before[j];
        }
    return H2HIP_OK;
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
    const uint32_t k = sh.k, slots = fp_unit_slots(k), cells = sh.lay.total;
    H2_REQUIRE(count <= ((uint64_t)1 << 32) / slots, "more than 2^32 slots (count * (4 num_limbs + 3)) in one call");
    H2_REQUIRE(num_columns >= 1 && num_columns < 0xFFFFFFFFu, "num_columns out of range");
    H2_REQUIRE(usable_rows <= 0xFFFFFFFFu, "usable_rows out of range");
    H2_REQUIRE(values_len <= SIZE_MAX / sizeof(Fr) && results_len <= SIZE_MAX / sizeof(Fr), "values_len / results_len is no count of field elements");
    if (break_points_host)
        for (size_t c = 0; c + 1 < num_columns; ++c) H2_REQUIRE(break_points_host[c] < usable_rows, "a break point >= usable_rows");
    H2_REQUIRE(!results_dev || results_len / fp_result_len(k) >= count, "results_len < count * (3 num_limbs + 1)");
    std::vector<ByteRange> written, reads;
    written.reserve(count + 9);
    reads.reserve(2 * count);
    for (size_t j = 0; j < count; ++j) {
        const h2hip_fp_mul &u = units_host[j];
        H2_REQUIRE(u.column < num_columns && columns_dev[u.column], "a unit's column index is out of range (or the column is NULL)");
        // the unit's whole run, gaps included, column by column, as the kernel's TraceOut walks it
        const char *left = run_byte_ranges(columns_dev, num_columns, usable_rows, break_points_host, u.column, u.row, cells, written);
        H2_REQUIRE(!left, left);
        H2_REQUIRE(u.a_offset < values_len && k < values_len - u.a_offset && u.b_offset < values_len && k < values_len - u.b_offset,
                   "a unit's operand lies outside values_len");
        reads.push_back(ByteRange{(uintptr_t)values_dev + sizeof(Fr) * u.a_offset, (uintptr_t)values_dev + sizeof(Fr) * (u.a_offset + k + 1)});
        reads.push_back(ByteRange{(uintptr_t)values_dev + sizeof(Fr) * u.b_offset, (uintptr_t)values_dev + sizeof(Fr) * (u.b_offset + k + 1)});
    }
    // two units' cells are disjoint; the results lie in none of them; no operand lies in anything written.  Address intervals, sorted and swept.
    const char *clash = byte_ranges_clash(written, {}, "two units' cells overlap (break copies and the range checks' gaps included)");
    H2_REQUIRE(!clash, clash);
    if (results_dev) written.push_back(ByteRange{(uintptr_t)results_dev, (uintptr_t)results_dev + sizeof(Fr) * fp_result_len(k) * count});
    clash = byte_ranges_clash(written, {&reads}, "the results overlap cells this call writes");
    H2_REQUIRE(!clash, clash);
    // ---- workspace: [unit table][column pointers][break points][constants], and the records
    const auto align = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t table_bytes = sizeof(h2hip_fp_mul) * count, ptr_off = align(table_bytes), ptr_bytes = sizeof(void *) * num_columns;
    const size_t bp_off = align(ptr_off + ptr_bytes), bp_bytes = break_points_host ? sizeof(uint32_t) * (num_columns - 1) : 0;
    const size_t cs_off = align(bp_off + bp_bytes), cs_bytes = sizeof(Fr) * FP_CONSTS;
    char *tabs = nullptr;
    Fr *rec = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP1, cs_off + cs_bytes, (void **)&tabs));
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP2, sizeof(Fr) * fp_record_len(k) * count, (void **)&rec));
    H2_CHK(upload_jobs(ctx, tabs, units_host, table_bytes));
    H2_CHK(upload_jobs(ctx, tabs + ptr_off, columns_dev, ptr_bytes));
    H2_CHK(upload_jobs(ctx, tabs + bp_off, break_points_host, bp_bytes));
    H2_CHK(upload_jobs(ctx, tabs + cs_off, consts, cs_bytes));
    fc.cols = (Fr *const *)(tabs + ptr_off);
    fc.bps = bp_bytes ? (const uint32_t *)(tabs + bp_off) : nullptr;
    fc.values = (const Fr *)values_dev;
    fc.consts = (const Fr *)(tabs + cs_off);
    fc.results = (Fr *)results_dev;
    fc.rec = rec;
    fc.last_col = (uint32_t)(num_columns - 1);
    const h2hip_fp_mul *units = (const h2hip_fp_mul *)tabs;
    const dim3 solve_grid((uint32_t)((count + FP_SOLVE_BLOCK - 1) / FP_SOLVE_BLOCK)), solve_block(FP_SOLVE_BLOCK);
    prof_begin(ctx, "fp_mul_solve_kernel");
    if (k == 2)
        hipLaunchKernelGGL(fp_mul_solve_kernel<2>, solve_grid, solve_block, 0, ctx->stream, fc, units, (uint32_t)count);
    else if (k == 3)
        hipLaunchKernelGGL(fp_mul_solve_kernel<3>, solve_grid, solve_block, 0, ctx->stream, fc, units, (uint32_t)count);
    else
        hipLaunchKernelGGL(fp_mul_solve_kernel<4>, solve_grid, solve_block, 0, ctx->stream, fc, units, (uint32_t)count);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    const uint64_t lanes = (uint64_t)count * slots;
    prof_begin(ctx, "fp_mul_place_kernel");
    hipLaunchKernelGGL(fp_mul_place_kernel, dim3((uint32_t)((lanes + FP_PLACE_BLOCK - 1) / FP_PLACE_BLOCK)), dim3(FP_PLACE_BLOCK), 0, ctx->stream, fc,
                       units, slots, lanes);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

}  // extern "C"
