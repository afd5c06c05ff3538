// tools/poseidon_trace_time.py's host side: h2hip_poseidon_fill_hashes_dev's cells computed on ONE host thread with the library's host field
// (csrc/field.cuh's fe_mul / fe_add as host code) and the library's own per-unit code (csrc/poseidon_trace.cuh), into host columns, from inputs
// in host memory — what a caller had to do with the cells before the device fill existed, short of writing a field of its own.  `spec` is the
// optimised spec in the order h2hip_poseidon_set_optimized_spec stores it: start, partial, end, mds, pre_sparse_mds, sparse, then 2^64.
// Built by the tool (hipcc, host only); not part of libh2hip.
#include "../halo2-lib_amd/csrc/poseidon_trace.cuh"

using namespace h2;

extern "C" void poseidon_host_fill_hashes(void *const *columns_host, size_t num_columns, const uint32_t *break_points, const void *inputs_host, uint32_t len,
                                          const h2hip_poseidon_hash *hashes, size_t count, const void *spec, uint32_t t, uint32_t r_f, uint32_t r_p) {
    const uint32_t half = r_f / 2;
    PoseidonOptDev sp;
    sp.start = (const Fr *)spec;
    sp.partial = sp.start + (size_t)(half + 1) * t;
    sp.end = sp.partial + r_p;
    sp.mds = sp.end + (size_t)(half - 1) * t;
    sp.pre = sp.mds + (size_t)t * t;
    sp.sparse = sp.pre + (size_t)t * t;
    sp.init0 = sp.sparse + (size_t)r_p * (2 * t - 1);
    sp.half = half;
    sp.r_p = r_p;
    const TraceCols tc{(Fr *const *)columns_host, break_points, (uint32_t)(num_columns - 1)};
    for (size_t j = 0; j < count; ++j) {
        if (t == 3) trace_unit<3>(tc, (const Fr *)inputs_host, len, nullptr, nullptr, hashes[j], (uint32_t)j, sp);
        else trace_unit<5>(tc, (const Fr *)inputs_host, len, nullptr, nullptr, hashes[j], (uint32_t)j, sp);
    }
}
