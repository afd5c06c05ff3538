// Range checks filled on the device: every gate cell that RangeChip::_range_check writes (halo2-base/src/gates/range/mod.rs:512-564: the limb
// decomposition as inner_product_simple's "b starts with Constant(1)" form, flex_gate/mod.rs:953-962, and the tail gate on the last limb),
// optionally behind the seven cells of check_less_than / is_less_than (:604-687), and the copies into the lookup-advice columns in the order
// LookupAnyManager::assign_raw lays the queue down (virtual_region/lookups.rs:129-156), for many cells of one width at once (include/h2hip.h
// states the cell form).
//
// One lane per (unit, slot) (the slot's code is range_fill.cuh's range_slot, host and device code): the running sums s_i are bit masks of v,
// so no slot waits for the one before it.  Lane g takes unit g / S and slot g mod S with S uniform over the call; neighbouring lanes of a unit
// write neighbouring groups of three cells.  Per lane: one fe_from_mont, bit slicing over the four 64-bit digits by comparisons, two
// fe_to_mont, the constant from the uploaded power table, 32-byte stores.  No LDS, no atomics, no workgroup waits for another.
#include "internal.h"
#include "range_fill.cuh"
#include "trace_host.h"

namespace h2 {

constexpr uint32_t RANGE_BLOCK = 256;

static_assert(sizeof(h2hip_range_check) == 32, "the unit table is uploaded as the caller laid it out");

// rc.values may point into the columns (at cells this call does not write: the host checked)
__global__ __launch_bounds__(RANGE_BLOCK) void range_fill_kernel(RangeCall rc, const h2hip_range_check *__restrict__ units, uint32_t slots, uint64_t lanes) {
    const uint64_t g = (uint64_t)blockIdx.x * RANGE_BLOCK + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t u = (uint32_t)(g / slots);
    range_slot(rc, units[u], (uint32_t)(g - (uint64_t)u * slots));
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2hip_range_check_layout(uint32_t range_bits, uint32_t lookup_bits, uint32_t flags, size_t *num_cells, size_t *num_lookup_cells, uint32_t *last_limb_offset) {
    H2_REQUIRE(num_cells && num_lookup_cells && last_limb_offset, "NULL argument");
    RangeCall rc;
    const char *bad = range_prepare(range_bits, lookup_bits, 0, flags, rc, nullptr);
    H2_REQUIRE(!bad, bad);
    const uint32_t L = rc.L, rem = rc.rem, prefix = rc.prefix;
    *num_cells = range_unit_cells(L, rem, prefix);
    *num_lookup_cells = range_unit_lookups(L, rem);
    // the last limb: l_{L-1} of the decomposition; with L = 1 the checked cell itself, which the unit writes only as the prefix's first cell
    *last_limb_offset = L >= 2 ? prefix + 1 + 3 * (L - 2) : prefix ? 0 : 0xFFFFFFFFu;
    return H2HIP_OK;
}

int h2hip_range_fill_checks_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                                void *const *lookup_columns_dev, size_t num_lookup_columns, const void *values_dev, size_t values_len, uint32_t range_bits,
                                uint32_t lookup_bits, uint32_t shift_bits, uint32_t flags, const h2hip_range_check *checks_host, size_t count) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "NULL argument");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched or uploaded
    H2_REQUIRE(checks_host && lookup_columns_dev && values_dev, "NULL argument");
    RangeCall rc;
    std::vector<Fr> pows;
    const char *bad = range_prepare(range_bits, lookup_bits, shift_bits, flags, rc, &pows);
    H2_REQUIRE(!bad, bad);
    const uint32_t L = rc.L, rem = rc.rem, prefix = rc.prefix;
    const uint32_t cells = range_unit_cells(L, rem, prefix), nlk = range_unit_lookups(L, rem), slots = range_unit_slots(L, rem);
    H2_REQUIRE(count <= ((uint64_t)1 << 32) / (L + 1), "more than 2^32 slots (count * (limbs + 1)) in one call");
    H2_REQUIRE(num_lookup_columns >= 1 && num_lookup_columns < 0xFFFFFFFFu, "num_lookup_columns out of range (no lookup column)");
    for (size_t c = 0; c < num_lookup_columns; ++c) H2_REQUIRE(lookup_columns_dev[c], "a NULL lookup column");
    H2_REQUIRE(usable_rows <= 0xFFFFFFFFu, "usable_rows out of range");
    H2_REQUIRE(values_len <= SIZE_MAX / sizeof(Fr), "values_len is no count of field elements");
    // (a unit of one limb without the prefix has no gate cell: such a call has no gate columns)
    TraceRuns gates{columns_dev, cells ? num_columns : 0, usable_rows, cells ? break_points_host : nullptr};
    if (cells) {
        H2_REQUIRE(columns_dev, "NULL argument");
        bad = gates.args_bad();
        H2_REQUIRE(!bad, bad);
    }
    const uint64_t lk_room = (uint64_t)usable_rows * num_lookup_columns;   // queue positions whose row is usable
    std::vector<ByteRange> reads;
    std::vector<uint64_t> lk_slots(count);
    gates.written.reserve(cells ? count + 8 : 0);
    reads.reserve(prefix ? 2 * count : count);
    for (size_t j = 0; j < count; ++j) {
        const h2hip_range_check &u = checks_host[j];
        if (cells) {
            bad = gates.run(u.column, u.row, cells);
            H2_REQUIRE(!bad, bad);
        }
        H2_REQUIRE(operand_range(values_dev, values_len, u.a_offset, 0, reads) && (!prefix || operand_range(values_dev, values_len, u.b_offset, 0, reads)),
                   "a unit's operand lies outside values_len");
        H2_REQUIRE(u.lookup_slot < lk_room && nlk <= lk_room - u.lookup_slot, "a unit's lookup cells leave the usable rows");
        lk_slots[j] = u.lookup_slot;
    }
    // two units' lookup cells: exact, in queue positions
    if (!std::is_sorted(lk_slots.begin(), lk_slots.end())) std::sort(lk_slots.begin(), lk_slots.end());
    for (size_t j = 1; j < count; ++j) H2_REQUIRE(lk_slots[j] - lk_slots[j - 1] >= nlk, "two units' lookup slot ranges intersect");
    // the gate cells of two units are disjoint; then no gate cell lies where a lookup cell does (a unit's positions in one lookup column are
    // one run of rows; runs of units sorted by slot ascend in every column); then no operand lies in anything written.  Address intervals,
    // sorted and swept.
    bad = byte_ranges_clash(gates.written, {}, "two units' gate cells overlap (break copies included)");
    H2_REQUIRE(!bad, bad);
    std::vector<ByteRange> written;
    written.reserve(gates.written.size() + count * (nlk < num_lookup_columns ? nlk : num_lookup_columns));
    for (size_t c = 0; c < num_lookup_columns; ++c)
        for (size_t j = 0; j < count; ++j) {
            const uint64_t p = lk_slots[j], first = p + (c + num_lookup_columns - p % num_lookup_columns) % num_lookup_columns;
            if (first >= p + nlk) continue;
            const uint64_t r0 = first / num_lookup_columns, r1 = (p + nlk - 1 - c) / num_lookup_columns;
            written.push_back(ByteRange{(uintptr_t)lookup_columns_dev[c] + sizeof(Fr) * r0, (uintptr_t)lookup_columns_dev[c] + sizeof(Fr) * (r1 + 1)});
        }
    written.insert(written.end(), gates.written.begin(), gates.written.end());
    bad = byte_ranges_clash(written, {&reads}, "a gate cell and a lookup cell of the call at one address (or two lookup columns overlap)");
    H2_REQUIRE(!bad, bad);
    // ---- tables: [unit table][gate column pointers][lookup column pointers][break points][powers]
    DevTables t;
    H2_CHK(pack_tables(ctx, {{checks_host, sizeof(h2hip_range_check) * count}, columns_table(gates), {lookup_columns_dev, sizeof(void *) * num_lookup_columns},
                             breaks_table(gates), {pows.data(), sizeof(Fr) * pows.size()}}, t));
    rc.tc = t.tc;
    rc.lk_cols = (Fr *const *)t.at[2];
    rc.values = (const Fr *)values_dev;
    rc.pows = (const Fr *)t.at[4];
    rc.num_lk_cols = (uint32_t)num_lookup_columns;
    const uint64_t lanes = (uint64_t)count * slots;
    prof_begin(ctx, "range_fill_kernel");
    hipLaunchKernelGGL(range_fill_kernel, dim3((uint32_t)((lanes + RANGE_BLOCK - 1) / RANGE_BLOCK)), dim3(RANGE_BLOCK), 0, ctx->stream, rc,
                       (const h2hip_range_check *)t.at[0], slots, lanes);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

}  // extern "C"
