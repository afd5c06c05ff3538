// tools/range_fill_time.py's host side: h2hip_range_fill_checks_dev's cells computed on ONE host thread with the library's host field
// (csrc/field.cuh's fe_from_mont / fe_to_mont as host code) and the library's own per-slot code (csrc/range_fill.cuh), into host columns, from
// values in host memory — what a caller had to do with the cells before the device fill existed, short of writing a field of its own.
// `pows` is the table the library uploads: 2^(i lb) for i < L, 2^(lb - rem), 2^shift_bits, -2^shift_bits (Montgomery).  Built by the tool
// (hipcc, host only); not part of libh2hip.
#include "../halo2-lib_amd/csrc/range_fill.cuh"

using namespace h2;

extern "C" void range_host_fill_checks(void *const *columns_host, size_t num_columns, const uint32_t *break_points, void *const *lookup_columns_host,
                                       size_t num_lookup_columns, const void *values_host, const void *pows, uint32_t range_bits, uint32_t lookup_bits,
                                       uint32_t flags, const h2hip_range_check *checks, size_t count) {
    RangeCall rc;
    if (range_prepare(range_bits, lookup_bits, 0, flags, rc, nullptr)) return;
    rc.tc = TraceCols{(Fr *const *)columns_host, break_points, num_columns ? (uint32_t)(num_columns - 1) : 0};
    rc.lk_cols = (Fr *const *)lookup_columns_host;
    rc.values = (const Fr *)values_host;
    rc.pows = (const Fr *)pows;
    rc.num_lk_cols = (uint32_t)num_lookup_columns;
    const uint32_t slots = range_unit_slots(rc.L, rc.rem);
    for (size_t j = 0; j < count; ++j)
        for (uint32_t s = 0; s < slots; ++s) range_slot(rc, checks[j], s);
}
