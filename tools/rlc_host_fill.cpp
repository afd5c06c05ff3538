// tools/rlc_time.py's host side: h2hip_rlc_fill_chains_dev's cells computed on ONE host thread with the library's host field (csrc/ec.cuh's
// fe_mul / fe_add as host code), into host columns — what a caller of h2hip_phase_witness_fn had to do before the device fill existed, short
// of writing a field of its own.  Built by the tool (hipcc, host only); not part of libh2hip.
#include "../halo2-lib_amd/csrc/host_field.h"

using namespace h2;

extern "C" void rlc_host_fill_chains(void *const *columns_host, const void *values_host, const h2hip_rlc_chain *chains, size_t count, const void *gamma) {
    const Fr *values = (const Fr *)values_host;
    const Fr g = ld_fr(gamma);
    Fr r = Fr::zero();
    for (size_t j = 0; j < count; ++j) {
        const h2hip_rlc_chain &c = chains[j];
        Fr *col = (Fr *)columns_host[c.column] + c.row;
        const Fr *v = values + c.value_offset;
        if (c.flags & H2HIP_RLC_CARRY) {
            col[0] = r;
            for (uint32_t i = 0; i < c.len; ++i) {
                r = fe_add(fe_mul(r, g), v[i]);
                col[2 * (size_t)i + 1] = v[i];
                col[2 * (size_t)i + 2] = r;
            }
        } else {
            r = v[0];
            col[0] = r;
            for (uint32_t i = 1; i < c.len; ++i) {
                r = fe_add(fe_mul(r, g), v[i]);
                col[2 * (size_t)i - 1] = v[i];
                col[2 * (size_t)i] = r;
            }
        }
    }
}
