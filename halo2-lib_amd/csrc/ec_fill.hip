// EccChip's ec_add_unequal (non-strict) and ec_double filled on the device: every gate cell the reference writes for one curve operation on
// points lying on the device — sub_no_carry / scalar_mul_no_carry / mul_no_carry, divide_unsafe (load_private of lambda and
// check_carry_mod_to_zero) and two carry_mod — except the cells of its 9 k range checks, which are left as gaps for
// h2hip_range_fill_checks_dev (halo2-ecc/src/ecc/mod.rs:153-179, :302-327, fields/mod.rs:217-238; include/h2hip.h states the cell form).
//
// Two kernels on the context's stream, their code in ec_fill.cuh as host and device code.  ec_solve_kernel: one lane per unit, templated on
// k and on the operation, does lambda's inversion mod p (division steps, the modulus a kernel argument) and the three signed floor divisions
// one after the other, each stage's cells going to the unit's record before the next stage begins.  ec_place_kernel: one lane per (unit,
// segment) writes a segment's cells through TraceOut from the record.  No LDS, no atomics, no workgroup waits for another.
#include "internal.h"
#include "ec_fill.cuh"

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
    *num_cells = sh.total;
    *num_own_cells = sh.own;
    *num_lookup_cells = sh.num_lookups;
    for (uint32_t j = 0; j < sh.ngaps; ++j) ranges[j] = sh.gaps[j];
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
    uint32_t width[EC_MAX_GAPS], group_of[EC_MAX_GAPS], gaps_in[EC_MAX_GAPS], lk_before[EC_MAX_GAPS], lk = 0;
    const uint32_t ng = ec_width_groups(sh, width, group_of, gaps_in);
    size_t start[EC_MAX_GAPS], next[EC_MAX_GAPS];
    for (uint32_t g = 0; g < ng; ++g) start[g] = g ? start[g - 1] + (size_t)gaps_in[g - 1] * count : 0;
    for (uint32_t j = 0; j < sh.ngaps; ++j) {
        lk_before[j] = lk;
        lk += sh.gap_lookups[j];
    }
    for (uint32_t g = 0; g < ng; ++g) next[g] = start[g];
    for (size_t u = 0; u < count; ++u)   // unit-major inside a width: rows and lookup slots ascend with the units
        for (uint32_t j = 0; j < sh.ngaps; ++j) {
            h2hip_range_check &c = checks_out[next[group_of[j]]++];
            const int r = h2hip_trace_seek(break_points_host, num_columns, units_host[u].column, units_host[u].row, sh.gaps[j].cell_offset, &c.column, &c.row);
            if (r != H2HIP_OK) return r;
            c.a_offset = (uint64_t)u * ec_result_len(sh.k) + sh.gaps[j].result_index;
            c.b_offset = 0;
            c.lookup_slot = lookup_slots_host[u] + lk_before[j];
        }
    return H2HIP_OK;
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
    const uint32_t k = sh.k, slots = sh.nsegs, cells = sh.total, k1 = k + 1, point = 2 * k1;
    const bool two = op == H2HIP_EC_ADD_UNEQUAL;
    H2_REQUIRE(count <= ((uint64_t)1 << 32) / slots, "more than 2^32 slots (count * the unit's segments) in one call");
    H2_REQUIRE(num_columns >= 1 && num_columns < 0xFFFFFFFFu, "num_columns out of range");
    H2_REQUIRE(usable_rows <= 0xFFFFFFFFu, "usable_rows out of range");
    H2_REQUIRE(values_len <= SIZE_MAX / sizeof(Fr) && results_len <= SIZE_MAX / sizeof(Fr), "values_len / results_len is no count of field elements");
    if (break_points_host)
        for (size_t c = 0; c + 1 < num_columns; ++c) H2_REQUIRE(break_points_host[c] < usable_rows, "a break point >= usable_rows");
    H2_REQUIRE(!results_dev || results_len / ec_result_len(k) >= count, "results_len < count * (9 num_limbs + 3)");
    std::vector<ByteRange> written, reads;
    written.reserve(count + 9);
    reads.reserve(2 * count);
    for (size_t j = 0; j < count; ++j) {
        const h2hip_ec_op &u = units_host[j];
        H2_REQUIRE(u.column < num_columns && columns_dev[u.column], "a unit's column index is out of range (or the column is NULL)");
        // the unit's whole run, gaps included, column by column, as the kernel's TraceOut walks it
        const char *left = run_byte_ranges(columns_dev, num_columns, usable_rows, break_points_host, u.column, u.row, cells, written);
        H2_REQUIRE(!left, left);
        H2_REQUIRE(u.p_offset < values_len && point - 1 < values_len - u.p_offset && (!two || (u.q_offset < values_len && point - 1 < values_len - u.q_offset)),
                   "a unit's operand lies outside values_len");
        reads.push_back(ByteRange{(uintptr_t)values_dev + sizeof(Fr) * u.p_offset, (uintptr_t)values_dev + sizeof(Fr) * (u.p_offset + point)});
        if (two) reads.push_back(ByteRange{(uintptr_t)values_dev + sizeof(Fr) * u.q_offset, (uintptr_t)values_dev + sizeof(Fr) * (u.q_offset + point)});
    }
    // two units' cells are disjoint; the results lie in none of them; no operand lies in anything written.  Address intervals, sorted and swept.
    const char *clash = byte_ranges_clash(written, {}, "two units' cells overlap (break copies and the range checks' gaps included)");
    H2_REQUIRE(!clash, clash);
    if (results_dev) written.push_back(ByteRange{(uintptr_t)results_dev, (uintptr_t)results_dev + sizeof(Fr) * ec_result_len(k) * count});
    clash = byte_ranges_clash(written, {&reads}, "the results overlap cells this call writes");
    H2_REQUIRE(!clash, clash);
    // ---- workspace: [unit table][column pointers][break points][constants][segments], and the records
    const auto align = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t table_bytes = sizeof(h2hip_ec_op) * count, ptr_off = align(table_bytes), ptr_bytes = sizeof(void *) * num_columns;
    const size_t bp_off = align(ptr_off + ptr_bytes), bp_bytes = break_points_host ? sizeof(uint32_t) * (num_columns - 1) : 0;
    const size_t cs_off = align(bp_off + bp_bytes), cs_bytes = sizeof(Fr) * EC_CONSTS;
    const size_t sg_off = align(cs_off + cs_bytes), sg_bytes = sizeof(EcSeg) * slots;
    char *tabs = nullptr;
    Fr *rec = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP1, sg_off + sg_bytes, (void **)&tabs));
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP2, sizeof(Fr) * ec_record_len(k) * count, (void **)&rec));
    H2_CHK(upload_jobs(ctx, tabs, units_host, table_bytes));
    H2_CHK(upload_jobs(ctx, tabs + ptr_off, columns_dev, ptr_bytes));
    H2_CHK(upload_jobs(ctx, tabs + bp_off, break_points_host, bp_bytes));
    H2_CHK(upload_jobs(ctx, tabs + cs_off, consts, cs_bytes));
    H2_CHK(upload_jobs(ctx, tabs + sg_off, sh.segs, sg_bytes));
    ec.cols = (Fr *const *)(tabs + ptr_off);
    ec.bps = bp_bytes ? (const uint32_t *)(tabs + bp_off) : nullptr;
    ec.values = (const Fr *)values_dev;
    ec.consts = (const Fr *)(tabs + cs_off);
    ec.segs = (const EcSeg *)(tabs + sg_off);
    ec.results = (Fr *)results_dev;
    ec.rec = rec;
    ec.last_col = (uint32_t)(num_columns - 1);
    const h2hip_ec_op *units = (const h2hip_ec_op *)tabs;
    const dim3 solve_grid((uint32_t)((count + EC_SOLVE_BLOCK - 1) / EC_SOLVE_BLOCK)), solve_block(EC_SOLVE_BLOCK);
    prof_begin(ctx, "ec_solve_kernel");
    if (k == 3 && two)
        hipLaunchKernelGGL((ec_solve_kernel<3, H2HIP_EC_ADD_UNEQUAL>), solve_grid, solve_block, 0, ctx->stream, ec, units, (uint32_t)count);
    else if (k == 3)
        hipLaunchKernelGGL((ec_solve_kernel<3, H2HIP_EC_DOUBLE>), solve_grid, solve_block, 0, ctx->stream, ec, units, (uint32_t)count);
    else if (two)
        hipLaunchKernelGGL((ec_solve_kernel<4, H2HIP_EC_ADD_UNEQUAL>), solve_grid, solve_block, 0, ctx->stream, ec, units, (uint32_t)count);
    else
        hipLaunchKernelGGL((ec_solve_kernel<4, H2HIP_EC_DOUBLE>), solve_grid, solve_block, 0, ctx->stream, ec, units, (uint32_t)count);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    const uint64_t lanes = (uint64_t)count * slots;
    prof_begin(ctx, "ec_place_kernel");
    hipLaunchKernelGGL(ec_place_kernel, dim3((uint32_t)((lanes + EC_PLACE_BLOCK - 1) / EC_PLACE_BLOCK)), dim3(EC_PLACE_BLOCK), 0, ctx->stream, ec,
                       units, slots, lanes);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

}  // extern "C"
