// The cells of one in-circuit Poseidon hash (include/h2hip.h states the form), as host and device code: poseidon_trace.hip's kernel runs
// trace_unit in one lane per unit, tools/poseidon_host_fill.cpp in a loop on one host thread.
#pragma once
#include "internal.h"
#include "trace_place.cuh"   // TraceOut: assign_witnesses' placement of a run of cells

namespace h2 {

// the optimised spec as the kernel reads it: [start (half+1) x T][partial r_p][end (half-1) x T][mds T x T][pre_sparse_mds T x T]
// [sparse r_p x (row T, col_hat T-1)][2^64]
struct PoseidonOptDev {
    const Fr *start, *partial, *end, *mds, *pre, *sparse, *init0;
    uint32_t half, r_p;
};

// x^5 + c as x_power5_with_constant writes it (state.rs:97-106): | 0 x x x2 | 0 x2 x2 x4 | c x x4 x*x4+c |
H2_HD Fr trace_sbox(TraceOut &o, const Fr &x, const Fr &c) {
    const Fr zero = Fr::zero(), x2 = fe_mul(x, x), x4 = fe_mul(x2, x2), r = fe_add(fe_mul(x, x4), c);
    o.put(zero);
    o.put(x);
    o.put(x);
    o.put(x2);
    o.put(zero);
    o.put(x2);
    o.put(x2);
    o.put(x4);
    o.put(c);
    o.put(x);
    o.put(x4);
    o.put(r);
    return r;
}
// <s, row> as inner_product_simple writes it when row does not start with Constant(1) (flex_gate/mod.rs:959-967): | 0 | s_b row_b sum | ...
template <int T>
H2_HD Fr trace_inner(TraceOut &o, const Fr (&s)[T], const Fr *__restrict__ row) {
    Fr acc = Fr::zero();
    o.put(acc);
    static_for<T>([&](auto b) {
        const Fr m = row[b];
        acc = fe_add(acc, fe_mul(s[b], m));
        o.put(s[b]);
        o.put(m);
        o.put(acc);
    });
    return acc;
}
template <int T>
H2_HD void trace_sbox_full(TraceOut &o, Fr (&s)[T], const Fr *__restrict__ c) {
    static_for<T>([&](auto k) { s[k] = trace_sbox(o, s[k], c ? c[k] : Fr::zero()); });
}
template <int T>
H2_HD void trace_mds(TraceOut &o, Fr (&s)[T], const Fr *__restrict__ m) {
    Fr n[T];
    static_for<T>([&](auto a) { n[a] = trace_inner<T>(o, s, m + a * T); });
    static_for<T>([&](auto a) { s[a] = n[a]; });
}

// PoseidonState::permutation(inputs, None) over m inputs x[0..m) (state.rs:35-83, absorb_with_pre_constants :124-161)
template <int T>
H2_HD void trace_permutation(TraceOut &o, Fr (&s)[T], const Fr *x, uint32_t x_stride, uint32_t m, const PoseidonOptDev &sp) {
    const Fr one = Fr::one();
    // add(s[0], pre[0]): | s0 pre0 1 s0+pre0 |
    {
        const Fr c = sp.start[0], r = fe_add(s[0], c);
        o.put(s[0]);
        o.put(c);
        o.put(one);
        o.put(r);
        s[0] = r;
    }
    static_for<T - 1>([&](auto i0) {
        constexpr int i = i0 + 1;
        const Fr c = sp.start[i];
        if ((uint32_t)i <= m) {   // sum([s_i, input, pre_i]): | s_i | in 1 s_i+in | pre_i 1 s_i+in+pre_i |
            const Fr in = x[(size_t)(i - 1) * x_stride], a = fe_add(s[i], in), r = fe_add(a, c);
            o.put(s[i]);
            o.put(in);
            o.put(one);
            o.put(a);
            o.put(c);
            o.put(one);
            o.put(r);
            s[i] = r;
        } else {   // add(s_i, pre_i), with the padding 1 folded into the constant of the first lane behind the inputs
            const Fr cc = (uint32_t)i == m + 1 ? fe_add(one, c) : c;
            const Fr r = fe_add(s[i], cc);
            o.put(s[i]);
            o.put(cc);
            o.put(one);
            o.put(r);
            s[i] = r;
        }
    });
    for (uint32_t r = 1; r < sp.half; ++r) {
        trace_sbox_full<T>(o, s, sp.start + r * T);
        trace_mds<T>(o, s, sp.mds);
    }
    trace_sbox_full<T>(o, s, sp.start + sp.half * T);
    trace_mds<T>(o, s, sp.pre);
    for (uint32_t r = 0; r < sp.r_p; ++r) {
        s[0] = trace_sbox(o, s[0], sp.partial[r]);
        // apply_sparse_mds (state.rs:230-250): <s, row>, then mul_add(s0, col_hat_i, s_{i+1}) = | s_{i+1} s0 col_hat_i s0*col_hat_i+s_{i+1} | on the OLD s0
        const Fr *sm = sp.sparse + (size_t)r * (2 * T - 1);
        const Fr n0 = trace_inner<T>(o, s, sm);
        static_for<T - 1>([&](auto i0) {
            constexpr int i = i0 + 1;
            const Fr h = sm[T + i - 1], n = fe_add(fe_mul(s[0], h), s[i]);
            o.put(s[i]);
            o.put(s[0]);
            o.put(h);
            o.put(n);
            s[i] = n;
        });
        s[0] = n0;
    }
    for (uint32_t r = 0; r + 1 < sp.half; ++r) {
        trace_sbox_full<T>(o, s, sp.end + r * T);
        trace_mds<T>(o, s, sp.mds);
    }
    trace_sbox_full<T>(o, s, nullptr);
    trace_mds<T>(o, s, sp.mds);
}

// one unit: fix_len_array_squeeze over `len` inputs, from PoseidonState::default or unit u's row of states_in
template <int T>
H2_HD void trace_unit(const TraceCols &tc, const Fr *inputs, uint32_t len, const Fr *states_in, Fr *states_out, const h2hip_poseidon_hash &unit, uint32_t u,
                      const PoseidonOptDev &sp) {
    constexpr uint32_t RATE = T - 1;
    TraceOut o = trace_at(tc, unit.column, unit.row);
    Fr s[T];
    s[0] = *sp.init0;
    static_for<T - 1>([&](auto k) { s[k + 1] = Fr::zero(); });
    if (unit.flags & H2HIP_POSEIDON_WITH_CONSTS) {   // PoseidonState::default's load_constant cells
        static_for<T>([&](auto k) { o.put(s[k]); });
    }
    if (states_in) {
        static_for<T>([&](auto k) { s[k] = states_in[(size_t)u * T + k]; });
    }
    const Fr *x = inputs + unit.input_offset;
    uint32_t at = 0;
    for (; at < len; at += RATE) {
        const uint32_t m = len - at < RATE ? len - at : RATE;
        trace_permutation<T>(o, s, x + (size_t)at * unit.input_stride, unit.input_stride, m, sp);
    }
    if (len % RATE == 0 && !(unit.flags & H2HIP_POSEIDON_ABSORB_ONLY)) trace_permutation<T>(o, s, x, 0, 0, sp);
    if (states_out) {
        static_for<T>([&](auto k) { states_out[(size_t)u * T + k] = s[k]; });
    }
}

}  // namespace h2
