// tools/gate_chain_time.py's host side: h2hip_gate_fill_chains_dev's cells computed on ONE host thread with the library's host field (csrc/ec.cuh's
// fe_mul / fe_add as host code), into host columns, from operands in host memory — what a caller of h2hip_phase_witness_fn had to do with the
// running sums before the device fill existed, short of writing a field of its own.  Built by the tool (hipcc, host only); not part of libh2hip.
#include "../halo2-lib_amd/csrc/host_field.h"

using namespace h2;

extern "C" void gate_host_fill_chains(void *const *columns_host, const void *a_host, const void *b_host, const h2hip_gate_chain *chains, size_t count) {
    const Fr *a = (const Fr *)a_host, *b = (const Fr *)b_host;
    Fr s = Fr::zero();
    for (size_t j = 0; j < count; ++j) {
        const h2hip_gate_chain &c = chains[j];
        Fr *col = (Fr *)columns_host[c.column] + c.row;
        uint32_t i = 0;
        if (c.flags & H2HIP_GATE_START_A) {
            s = a[c.a_offset];
            *col++ = s;
            i = 1;
        } else if (c.flags & H2HIP_GATE_CARRY) {
            *col++ = s;
        } else if (!(c.flags & H2HIP_GATE_JOIN)) {
            s = Fr::zero();
            *col++ = s;
        }
        for (; i < c.len; ++i, col += 3) {
            const Fr av = a[c.a_offset + (uint64_t)i * c.a_stride], bv = b[c.b_offset + (uint64_t)i * c.b_stride];
            s = fe_add(s, fe_mul(av, bv));
            col[0] = av;
            col[1] = bv;
            col[2] = s;
        }
    }
}
