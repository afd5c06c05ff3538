// The cells of one FpChip::mul (include/h2hip.h states the form): mul_no_carry::crt followed by carry_mod::crt with its check_carry_to_zero,
// as host and device code.  fp_mul.hip's first kernel runs fp_solve_unit in one lane per unit (the big-integer step: product, Barrett
// division, limbs, carries -> a per-unit record), its second fp_place_slot in one lane per (unit, slot); tools/fp_mul_host_fill.cpp runs both
// in a loop on one host thread.  fp_prepare is what the host derives from h2hip_fp_params once per call.
#pragma once
#include "internal.h"
#include "range_fill.cuh"   // range_low_bits, range_unit_cells / range_unit_lookups, pow2_mont
#include "trace_place.cuh"

namespace h2 {

// (a lambda's call operator is an ordinary function to the inliner: left out of line in the larger instantiations, it takes its arrays by
// address, and they leave the registers)
#define H2_INL __attribute__((always_inline))

constexpr uint32_t FP_MAX_K = 4;
constexpr uint32_t FP_P_WORDS = 11;    // p < 2^320, one word of head room for the remainder before its correction
constexpr uint32_t FP_MU_WORDS = 13;   // mu = floor(2^S / p) with S = 512 (k = 2) or 640 and p >= 2^252
constexpr uint32_t FP_CONSTS = 2 * FP_MAX_K + 4;
constexpr uint32_t FP_NUM_BITS = 254, FP_CAPACITY = 253;   // F::NUM_BITS, F::CAPACITY

// what one call's lanes share.  consts (canonical Montgomery Fr): [m_i, i < k][2^(n i), i < k][2^quot_last_limb_bits][2^rb][m_nat][-1]
struct FpCall : TraceCall {
    uint32_t n, k;
    uint32_t gap_o, gap_ol, gap_q, gap_ql, gap_c;   // cells of the range checks of o_i (the last), q_i + B (the last), -c_i + 2^rb
    uint32_t p[FP_P_WORDS], mu[FP_MU_WORDS];        // wave-uniform: the modulus and its Barrett constant, 32-bit words
};
H2_CALL_LEADS(FpCall) H2_OFFSET_IS(FpCall, n, 56) H2_OFFSET_IS(FpCall, k, 60) H2_OFFSET_IS(FpCall, gap_o, 64) H2_OFFSET_IS(FpCall, gap_ol, 68)
H2_OFFSET_IS(FpCall, gap_q, 72) H2_OFFSET_IS(FpCall, gap_ql, 76) H2_OFFSET_IS(FpCall, gap_c, 80) H2_OFFSET_IS(FpCall, p, 84) H2_OFFSET_IS(FpCall, mu, 128)
static_assert(sizeof(FpCall) == 184, "FpCall grew or shrank");
H2_HD uint32_t fp_record_len(uint32_t k) { return 5 * k + 3; }    // [q_i][o_i][-c_i][P_i][check_i] N quot_native out_native
H2_HD uint32_t fp_result_len(uint32_t k) { return 3 * k + 1; }    // [o_i] out_native [q_i + B][-c_i + 2^rb]
H2_HD uint32_t fp_unit_slots(uint32_t k) { return 4 * k + 3; }

// offsets of the segments inside a unit's run (the table in include/h2hip.h): S1_i = 3 i (i - 1) / 2 + 4 i, S2 = off2, S3_i = base3 + 3 i (i - 1) / 2
// + 10 i, S4_i = base4 + i gap_o, S5_i = base5 + i (4 + gap_q), S6_i = base6 + i (8 + gap_c), S7, S8, S9
struct FpLayout {
    uint32_t off2, base3, base4, base5, base6, off7, off8, off9, total;
};
H2_HD uint32_t fp_tri(uint32_t i) { return 3 * i * (i + 1) / 2 - 3 * i; }
H2_HD FpLayout fp_layout(uint32_t k, uint32_t gap_o, uint32_t gap_ol, uint32_t gap_q, uint32_t gap_ql, uint32_t gap_c) {
    FpLayout l;
    l.off2 = fp_tri(k) + 4 * k;
    l.base3 = l.off2 + 4;
    l.base4 = l.base3 + fp_tri(k) + 10 * k;
    l.base5 = l.base4 + (k - 1) * gap_o + gap_ol;
    l.base6 = l.base5 + (k - 1) * (4 + gap_q) + 4 + gap_ql;
    l.off7 = l.base6 + k * (8 + gap_c);
    l.off8 = l.off7 + 3 * k - 2;
    l.off9 = l.off8 + 3 * k - 2;
    l.total = l.off9 + 3;
    return l;
}

// ---- integers of N 32-bit words, every index a compile-time constant (a runtime index would move the array to scratch)
template <int I, int N>
H2_HD uint32_t mp_at(const uint32_t (&x)[N]) {
    if constexpr (I >= 0 && I < N)
        return x[I];
    else
        return 0;
}
template <int NA, int NB>
H2_HD void mp_mul(const uint32_t (&a)[NA], const uint32_t (&b)[NB], uint32_t (&r)[NA + NB]) {
    static_for<NA + NB>([&](auto j) H2_INL { r[decltype(j)::value] = 0; });
    static_for<NB>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value;
        uint32_t carry = 0;
        static_for<NA>([&](auto j0) H2_INL {
            constexpr int j = decltype(j0)::value;
            const uint64_t t = (uint64_t)a[j] * b[i] + r[i + j] + carry;
            r[i + j] = (uint32_t)t;
            carry = (uint32_t)(t >> 32);
        });
        r[i + NA] = carry;
    });
}
// words [FROM, FROM + NR) of a b, column by column (the columns below FROM only feed the carry): no array for the whole product
template <int NA, int NB, int FROM, int NR>
H2_HD void mp_mul_words(const uint32_t (&a)[NA], const uint32_t (&b)[NB], uint32_t (&r)[NR]) {
    uint64_t lo = 0;
    uint32_t hi = 0;
    static_for<FROM + NR>([&](auto c0) H2_INL {
        constexpr int c = decltype(c0)::value, j0 = c - (NA - 1) > 0 ? c - (NA - 1) : 0, j1 = c < NB - 1 ? c : NB - 1;
        static_for<(j1 - j0 + 1 > 0 ? j1 - j0 + 1 : 0)>([&](auto jj) H2_INL {
            constexpr int j = j0 + decltype(jj)::value;
            const uint64_t p = (uint64_t)a[c - j] * b[j];
            lo += p;
            hi += lo < p ? 1u : 0u;
        });
        if constexpr (c >= FROM) r[c - FROM] = (uint32_t)lo;
        lo = lo >> 32 | (uint64_t)hi << 32;
        hi = 0;
    });
}
template <int N>
H2_HD void mp_mul_low(const uint32_t (&a)[N], const uint32_t (&b)[N], uint32_t (&r)[N]) {   // a b mod 2^(32 N)
    static_for<N>([&](auto j) H2_INL { r[decltype(j)::value] = 0; });
    static_for<N>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value;
        uint32_t carry = 0;
        static_for<N - i>([&](auto j0) H2_INL {
            constexpr int j = decltype(j0)::value;
            const uint64_t t = (uint64_t)a[j] * b[i] + r[i + j] + carry;
            r[i + j] = (uint32_t)t;
            carry = (uint32_t)(t >> 32);
        });
    });
}
template <int N>
H2_HD unsigned mp_sub(const uint32_t (&a)[N], const uint32_t (&b)[N], uint32_t (&r)[N]) {   // -> the borrow
    unsigned br = 0;
    static_for<N>([&](auto j) H2_INL { r[decltype(j)::value] = subb32(a[decltype(j)::value], b[decltype(j)::value], br); });
    return br;
}
template <int N>
H2_HD void mp_neg_if(uint32_t (&x)[N], uint32_t neg) {   // two's complement negation when neg == 1
    unsigned c = neg;
    const uint32_t m = 0u - neg;
    static_for<N>([&](auto j) H2_INL { x[decltype(j)::value] = addc32(x[decltype(j)::value] ^ m, 0, c); });
}
// shifts by n bits, 64 <= n <= 127: two or three whole words, chosen by a comparison, and n mod 32 bits
template <int N>
H2_HD void mp_shr(uint32_t (&x)[N], uint32_t n) {
    const bool w3 = n >= 96;
    const uint32_t s = n & 31;
    uint32_t t[N];
    static_for<N>([&](auto j0) H2_INL {
        constexpr int j = decltype(j0)::value;
        const uint32_t lo = w3 ? mp_at<j + 3>(x) : mp_at<j + 2>(x), hi = w3 ? mp_at<j + 4>(x) : mp_at<j + 3>(x);
        t[j] = s ? (lo >> s) | (hi << (32 - s)) : lo;
    });
    static_for<N>([&](auto j) H2_INL { x[decltype(j)::value] = t[decltype(j)::value]; });
}
template <int N>
H2_HD void mp_shl(uint32_t (&x)[N], uint32_t n) {
    const bool w3 = n >= 96;
    const uint32_t s = n & 31;
    uint32_t t[N];
    static_for<N>([&](auto j0) H2_INL {
        constexpr int j = decltype(j0)::value;
        const uint32_t hi = w3 ? mp_at<j - 3>(x) : mp_at<j - 2>(x), lo = w3 ? mp_at<j - 4>(x) : mp_at<j - 3>(x);
        t[j] = s ? (hi << s) | (lo >> (32 - s)) : hi;
    });
    static_for<N>([&](auto j) H2_INL { x[decltype(j)::value] = t[decltype(j)::value]; });
}
template <int N>
H2_HD Fr mp_low_limb(const uint32_t (&x)[N], uint32_t n) {   // the low n <= 127 bits as a canonical integer
    Fr c = Fr::zero();
    static_for<4>([&](auto j) H2_INL { c.l[decltype(j)::value] = x[decltype(j)::value]; });
    return range_low_bits(c, n);
}

// (Q, O) = floor divmod of X < 2^S by p through mu = floor(2^S / p), S = 64 WA: the estimate floor(X mu / 2^S) is Q or Q - 1, so the correction
// loop runs at most once; its bound is two.  Q mod 2^(32 (WA + 1)): limbs past k are dropped anyway.
template <int WA>
H2_HD void fp_barrett(const uint32_t (&X)[2 * WA], const uint32_t (&p)[FP_P_WORDS], const uint32_t (&mu_)[FP_MU_WORDS], uint32_t (&Q)[WA + 1],
                      uint32_t (&O)[WA + 1]) {
    constexpr int WR = WA + 1;
    uint32_t pw[WR];
    static_for<WR>([&](auto j) H2_INL { pw[decltype(j)::value] = p[decltype(j)::value]; });
    {
        uint32_t mu[FP_MU_WORDS];
        static_for<(int)FP_MU_WORDS>([&](auto j) H2_INL { mu[decltype(j)::value] = mu_[decltype(j)::value]; });
        mp_mul_words<2 * WA, (int)FP_MU_WORDS, 2 * WA, WR>(X, mu, Q);
        uint32_t QP[WR], XL[WR];
        mp_mul_low<WR>(Q, pw, QP);
        static_for<WR>([&](auto j) H2_INL { XL[decltype(j)::value] = X[decltype(j)::value]; });
        mp_sub<WR>(XL, QP, O);   // < 2 p < 2^(32 WR)
    }
    static_for<2>([&](auto) H2_INL {
        uint32_t D[WR];
        const unsigned below = mp_sub<WR>(O, pw, D);
        unsigned c = below ? 0u : 1u;
        static_for<WR>([&](auto j) H2_INL {
            O[decltype(j)::value] = below ? O[decltype(j)::value] : D[decltype(j)::value];
            Q[decltype(j)::value] = addc32(Q[decltype(j)::value], 0, c);
        });
    });
}
// one step of check_carry_to_zero's chain: cw holds c_{i-1} in 288-bit two's complement and gets c_i = trunc((signed(check) + c_{i-1}) / 2^n)
// (|signed(check)| < 2^253, |c_i| < 2^190), signed() as fe_to_bigint: above (r - 1) / 2 is negative -> -c_i (Montgomery)
H2_HD Fr fp_carry_step(const Fr &check, uint32_t (&cw)[9], uint32_t n) {
    const Fr c = fe_from_mont(check);
    unsigned br = 0;
    static_for<9>([&](auto j0) H2_INL {   // 2 c >= r ?
        constexpr int j = decltype(j0)::value;
        const uint32_t two_c = (j < 8 ? c.l[j < 8 ? j : 0] << 1 : 0u) | (j > 0 ? c.l[j > 0 ? j - 1 : 0] >> 31 : 0u);
        subb32(two_c, j < 8 ? FrP::m(j < 8 ? j : 0) : 0u, br);
    });
    const bool neg = br == 0;
    uint32_t v[9];
    br = 0;
    static_for<8>([&](auto j0) H2_INL {
        constexpr int j = decltype(j0)::value;
        const uint32_t d = subb32(c.l[j], FrP::m(j), br);
        v[j] = neg ? d : c.l[j];
    });
    v[8] = neg ? 0xFFFFFFFFu : 0u;
    unsigned cy = 0;
    static_for<9>([&](auto j) H2_INL { v[decltype(j)::value] = addc32(v[decltype(j)::value], cw[decltype(j)::value], cy); });
    const uint32_t sign = v[8] >> 31;
    mp_neg_if<9>(v, sign);   // the magnitude: the division truncates toward zero
    mp_shr<9>(v, n);
    Fr cm;
    static_for<8>([&](auto j) H2_INL { cm.l[decltype(j)::value] = v[decltype(j)::value]; });
    cm = fe_to_mont(cm);
    const Fr negc = sign ? cm : fe_neg(cm);
    static_for<9>([&](auto j) H2_INL { cw[decltype(j)::value] = v[decltype(j)::value]; });
    mp_neg_if<9>(cw, sign);
    return negc;
}

// ---- the big-integer step of one unit: the record and the results entries
// A = sum (canon(a_i) mod 2^n) 2^(n i), B alike; (Q, O) = floor divmod of A B < 2^S by p (fp_barrett, S = 64 WA >= 2 n k).  q_i, o_i: the low k limbs.
template <int K>
H2_HD void fp_solve_unit(const FpCall &fc, const h2hip_fp_mul &unit, uint32_t u) {
    constexpr int WA = K == 2 ? 8 : 10, WR = WA + 1;
    static_assert(WR <= (int)FP_P_WORDS, "the modulus words cover the remainder");
    const uint32_t n = fc.n;
    const Fr *va = fc.values + unit.a_offset, *vb = fc.values + unit.b_offset, *cs = fc.consts;
    Fr a[K], b[K];
    static_for<K>([&](auto i) H2_INL {
        a[decltype(i)::value] = va[decltype(i)::value];
        b[decltype(i)::value] = vb[decltype(i)::value];
    });
    uint32_t X[2 * WA];
    {
        uint32_t A[WA], B[WA];
        static_for<WA>([&](auto j) H2_INL { A[decltype(j)::value] = B[decltype(j)::value] = 0; });
        static_for<K>([&](auto i0) H2_INL {
            constexpr int i = K - 1 - decltype(i0)::value;
            const Fr la = range_low_bits(fe_from_mont(a[i]), n), lb = range_low_bits(fe_from_mont(b[i]), n);
            mp_shl<WA>(A, n);
            mp_shl<WA>(B, n);
            static_for<4>([&](auto j) H2_INL {
                A[decltype(j)::value] |= la.l[decltype(j)::value];
                B[decltype(j)::value] |= lb.l[decltype(j)::value];
            });
        });
        mp_mul<WA, WA>(A, B, X);
    }
    uint32_t Q[WR], O[WR];
    fp_barrett<WA>(X, fc.p, fc.mu, Q, O);
    Fr *rec = fc.rec + (size_t)u * fp_record_len(K);
    Fr *res = fc.results ? fc.results + (size_t)u * fp_result_len(K) : nullptr;
    Fr q[K], o[K];
    static_for<K>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value;
        q[i] = fe_to_mont(mp_low_limb<WR>(Q, n));
        o[i] = fe_to_mont(mp_low_limb<WR>(O, n));
        mp_shr<WR>(Q, n);
        mp_shr<WR>(O, n);
        rec[i] = q[i];
        rec[K + i] = o[i];
        if (res) {
            res[i] = o[i];
            res[K + 1 + i] = fe_add(q[i], i == K - 1 ? cs[2 * K] : cs[K + 1]);
        }
    });
    // P_i, prod_i and check_i in Fr from the operand values themselves; the carries by fp_carry_step
    uint32_t cw[9];
    static_for<9>([&](auto j) H2_INL { cw[decltype(j)::value] = 0; });
    static_for<K>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value;
        Fr P = Fr::zero(), prod = Fr::zero();
        static_for<i + 1>([&](auto j0) H2_INL {
            constexpr int j = decltype(j0)::value;
            P = fe_add(P, fe_mul(a[j], b[i - j]));
            prod = fe_add(prod, fe_mul(q[j], cs[i - j]));
        });
        const Fr check = fe_add(fe_sub(prod, P), o[i]);
        rec[3 * K + i] = P;
        rec[4 * K + i] = check;
        const Fr negc = fp_carry_step(check, cw, n);
        rec[2 * K + i] = negc;
        if (res) res[2 * K + 1 + i] = fe_add(negc, cs[2 * K + 1]);
    });
    Fr qn = q[0], on = o[0];
    static_for<K - 1>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value + 1;
        qn = fe_add(qn, fe_mul(q[i], cs[K + i]));
        on = fe_add(on, fe_mul(o[i], cs[K + i]));
    });
    rec[5 * K] = fe_mul(va[K], vb[K]);
    rec[5 * K + 1] = qn;
    rec[5 * K + 2] = on;
    if (res) res[K] = on;
}

// ---- one slot of one unit: S1_i (i < k), S2 with S9, S3_i, S5_i, S6_i, S7, S8, in this order; each lane recomputes its own running sums
H2_HD void fp_place_slot(const FpCall &fc, const h2hip_fp_mul &unit, uint32_t u, uint32_t slot) {
    const uint32_t k = fc.k;
    const FpLayout lay = fp_layout(k, fc.gap_o, fc.gap_ol, fc.gap_q, fc.gap_ql, fc.gap_c);
    const Fr *va = fc.values + unit.a_offset, *vb = fc.values + unit.b_offset, *cs = fc.consts, *rec = fc.rec + (size_t)u * fp_record_len(k);
    const Fr *q = rec, *o = rec + k, *negc = rec + 2 * k, *P = rec + 3 * k, *check = rec + 4 * k;
    const Fr zero = Fr::zero(), one = Fr::one();
    TraceOut out;
    if (slot < k) {   // ip(a_0 .. a_i; b_i .. b_0)
        const uint32_t i = slot;
        out = trace_at(fc.tc, unit.column, unit.row, fp_tri(i) + 4 * i);
        Fr acc = zero;
        out.put(acc);
        for (uint32_t j = 0; j <= i; ++j) {
            const Fr x = va[j], y = vb[i - j];
            acc = fe_add(acc, fe_mul(x, y));
            out.put(x);
            out.put(y);
            out.put(acc);
        }
    } else if (slot == k) {   // 0, a_nat, b_nat, N; and the three cells behind out_native: m_nat, quot_native, N
        out = trace_at(fc.tc, unit.column, unit.row, lay.off2);
        out.put(zero);
        out.put(va[k]);
        out.put(vb[k]);
        out.put(rec[5 * k]);
        out = trace_at(fc.tc, unit.column, unit.row, lay.off9);
        out.put(cs[2 * k + 2]);
        out.put(rec[5 * k + 1]);
        out.put(rec[5 * k]);
    } else if (slot <= 2 * k) {   // ip(q_0 .. q_i; m_i .. m_0), then -1, P_i, prod_i - P_i, 1, o_i, check_i
        const uint32_t i = slot - k - 1;
        out = trace_at(fc.tc, unit.column, unit.row, lay.base3 + fp_tri(i) + 10 * i);
        Fr acc = zero;
        out.put(acc);
        for (uint32_t j = 0; j <= i; ++j) {
            const Fr x = q[j], y = cs[i - j];
            acc = fe_add(acc, fe_mul(x, y));
            out.put(x);
            out.put(y);
            out.put(acc);
        }
        out.put(cs[2 * k + 3]);
        out.put(P[i]);
        out.put(fe_sub(acc, P[i]));
        out.put(one);
        out.put(o[i]);
        out.put(check[i]);
    } else if (slot <= 3 * k) {   // q_i, B, 1, q_i + B
        const uint32_t i = slot - 2 * k - 1;
        const Fr base = i == k - 1 ? cs[2 * k] : cs[k + 1];
        out = trace_at(fc.tc, unit.column, unit.row, lay.base5 + i * (4 + fc.gap_q));
        out.put(q[i]);
        out.put(base);
        out.put(one);
        out.put(fe_add(q[i], base));
    } else if (slot <= 4 * k) {   // check_i, -c_i, 2^n, -c_{i-1}; -c_i, 2^rb, 1, -c_i + 2^rb
        const uint32_t i = slot - 3 * k - 1;
        const Fr nc = negc[i], shift = cs[2 * k + 1];
        out = trace_at(fc.tc, unit.column, unit.row, lay.base6 + i * (8 + fc.gap_c));
        out.put(check[i]);
        out.put(nc);
        out.put(cs[k + 1]);
        Fr prev = zero;
        if (i) prev = negc[i - 1];
        out.put(prev);
        out.put(nc);
        out.put(shift);
        out.put(one);
        out.put(fe_add(nc, shift));
    } else {   // evaluate_native: x_0, x_1, 2^n, s_1, ... over q, then over o
        const Fr *x = slot == 4 * k + 1 ? q : o;
        out = trace_at(fc.tc, unit.column, unit.row, slot == 4 * k + 1 ? lay.off7 : lay.off8);
        Fr acc = x[0];
        out.put(acc);
        for (uint32_t j = 1; j < k; ++j) {
            const Fr y = cs[k + j];
            acc = fe_add(acc, fe_mul(x[j], y));
            out.put(x[j]);
            out.put(y);
            out.put(acc);
        }
    }
}

// ---- what the host derives from the parameters, once per call (host only)
// what the shape of every fused unit (FpShape, EcShape, CmpShape) states of its run: the cells, those the unit writes itself, the lookup
// cells of its range checks, and the gaps those checks fill, in context order (the lookup queue order)
constexpr uint32_t UNIT_MAX_GAPS = 9 * FP_MAX_K;
struct UnitShape {
    uint32_t total, own, num_lookups, ngaps;
    h2hip_fp_mul_range gaps[UNIT_MAX_GAPS];
    uint32_t gap_lookups[UNIT_MAX_GAPS];
};
// the gaps: o_i (behind S3), q_i + B (behind its four cells), -c_i + 2^rb (behind its eight)
struct FpShape : UnitShape {
    uint32_t n, k, lb, rb, out_last_bits, quot_last_bits;
    uint32_t gap[5];       // cells of a range check of n, out_last_bits, n + 1, quot_last_bits + 1, rb + 1 bits
    FpLayout lay;
};
inline uint32_t fp_words_bits(const uint32_t *w, int nw) {
    for (int j = nw - 1; j >= 0; --j)
        if (w[j]) return 32u * j + 32u - (uint32_t)__builtin_clz(w[j]);
    return 0;
}
// nullptr when the parameters are served, else the reason.  fc (optional): n, k, the gaps, p, mu; consts (optional): FP_CONSTS entries
inline const char *fp_prepare(const h2hip_fp_params &pr, FpShape &sh, FpCall *fc, Fr *consts) {
    const uint32_t n = pr.limb_bits, k = pr.num_limbs, lb = pr.lookup_bits;
    if (pr.flags) return "flags must be 0";
    if (n < 64 || n > 127) return "limb_bits outside 64 .. 127";
    if (k < 2 || k > FP_MAX_K) return "num_limbs outside 2 .. 4";
    if (n * k > 320) return "limb_bits * num_limbs > 320";
    const uint32_t log2_ceil = k == 2 ? 1 : 2, bit_len = k == 4 ? 3 : 2;
    if (log2_ceil + 2 * n > FP_NUM_BITS - 2) return "ceil(log2 num_limbs) + 2 limb_bits > 252 (mul_no_carry's bound)";
    uint32_t p[12];
    memcpy(p, pr.modulus, 48);
    const uint32_t pbits = fp_words_bits(p, 12);
    if (pbits == 0) return "the modulus is zero";
    if (pbits <= n * (k - 1) || pbits > n * k) return "the modulus does not need exactly num_limbs limbs";
    const uint32_t quot_max_bits = n * k - 1 + FP_NUM_BITS - 1 - pbits;
    if (quot_max_bits >= n * k) return "quot_max_bits >= limb_bits * num_limbs (the modulus has fewer than 253 bits)";
    if (lb < 1 || lb > 63) return "lookup_bits outside 1 .. 63";
    // the limbs of p
    Fr m[FP_MAX_K];
    {
        uint32_t w[12];
        memcpy(w, p, 48);
        for (uint32_t i = 0; i < k; ++i) {
            Fr c = Fr::zero();
            for (int j = 0; j < 4; ++j) c.l[j] = w[j];
            c = range_low_bits(c, n);
            const bool is_one = c.l[0] == 1 && !(c.l[1] | c.l[2] | c.l[3]);
            if (is_one) return "a limb of the modulus equals 1 (inner_product_simple then writes another cell form)";
            m[i] = fe_to_mont(c);
            const uint32_t wsh = n >> 5, s = n & 31;   // w >>= n
            for (uint32_t j = 0; j < 12; ++j) {
                const uint32_t lo = j + wsh < 12 ? w[j + wsh] : 0, hi = j + wsh + 1 < 12 ? w[j + wsh + 1] : 0;
                w[j] = s ? (lo >> s) | (hi << (32 - s)) : lo;
            }
        }
    }
    sh.n = n;
    sh.k = k;
    sh.lb = lb;
    sh.out_last_bits = pbits - n * (k - 1);
    sh.quot_last_bits = quot_max_bits - n * (k - 1);
    const uint32_t a_max = log2_ceil + 2 * n, max_limb_bits = std::max(std::max(n, a_max) + 1, 2 * n + bit_len);
    sh.rb = (max_limb_bits - n + 1 + lb) / lb * lb - 1;
    const uint32_t width[5] = {n, sh.out_last_bits, n + 1, sh.quot_last_bits + 1, sh.rb + 1};
    uint32_t lookups[5];
    for (int j = 0; j < 5; ++j) {
        const uint32_t L = (width[j] + lb - 1) / lb, rem = width[j] % lb;
        if ((uint64_t)L * lb > FP_CAPACITY) return "the limbs of a range check take more than 253 bits (F::CAPACITY)";
        sh.gap[j] = range_unit_cells(L, rem, 0);
        lookups[j] = range_unit_lookups(L, rem);
    }
    sh.lay = fp_layout(k, sh.gap[0], sh.gap[1], sh.gap[2], sh.gap[3], sh.gap[4]);
    sh.total = sh.lay.total;
    sh.own = 3 * k * k + 29 * k + 3;
    sh.num_lookups = 0;
    sh.ngaps = 3 * k;
    for (uint32_t j = 0; j < 3 * k; ++j) {
        const uint32_t i = j % k, grp = j / k, w = 2 * grp + (grp < 2 && i == k - 1 ? 1 : 0);   // (the last o and the last q have a width of their own)
        const uint32_t off = grp == 0 ? sh.lay.base4 + i * sh.gap[0] : grp == 1 ? sh.lay.base5 + i * (4 + sh.gap[2]) + 4 : sh.lay.base6 + i * (8 + sh.gap[4]) + 8;
        sh.gaps[j] = h2hip_fp_mul_range{off, sh.gap[w], width[w], grp == 0 ? i : grp * k + 1 + i};
        sh.gap_lookups[j] = lookups[w];
        sh.num_lookups += lookups[w];
    }
    if (consts) {
        Fr m_nat = Fr::zero();
        for (uint32_t i = 0; i < k; ++i) {
            consts[i] = m[i];
            consts[k + i] = pow2_mont(n * i);
            m_nat = fe_add(m_nat, fe_mul(m[i], consts[k + i]));
        }
        consts[2 * k] = pow2_mont(sh.quot_last_bits);
        consts[2 * k + 1] = pow2_mont(sh.rb);
        consts[2 * k + 2] = m_nat;
        consts[2 * k + 3] = fe_neg(Fr::one());
    }
    if (fc) {
        fc->n = n;
        fc->k = k;
        fc->gap_o = sh.gap[0];
        fc->gap_ol = sh.gap[1];
        fc->gap_q = sh.gap[2];
        fc->gap_ql = sh.gap[3];
        fc->gap_c = sh.gap[4];
        for (uint32_t j = 0; j < FP_P_WORDS; ++j) fc->p[j] = p[j];   // (p < 2^320: the eleventh word is zero)
        // mu = floor(2^S / p) by shift and subtract, S = 512 (k = 2) or 640; below 2^(S - 251): 13 words
        const uint32_t S = k == 2 ? 512 : 640;
        uint32_t rem[12] = {0}, mu[21] = {0};
        for (int bit = (int)S; bit >= 0; --bit) {
            uint32_t carry = bit == (int)S ? 1u : 0u;   // the numerator's only set bit
            for (int j = 0; j < 12; ++j) {
                const uint32_t nx = rem[j] >> 31;
                rem[j] = rem[j] << 1 | carry;
                carry = nx;
            }
            uint32_t d[12];
            unsigned br = 0;
            for (int j = 0; j < 12; ++j) d[j] = subb32(rem[j], p[j], br);
            if (!br) {
                memcpy(rem, d, sizeof rem);
                mu[bit >> 5] |= 1u << (bit & 31);
            }
        }
        for (uint32_t j = 0; j < FP_MU_WORDS; ++j) fc->mu[j] = mu[j];
    }
    return nullptr;
}

// The h2hip_range_check of every gap of every unit (h2hip_fp_mul or h2hip_ec_op: column and row lead both), entry (u, j) written to
// out[index(u, j)]: its first cell by h2hip_trace_seek's walk from the unit's first cell, its value at results entry u result_len +
// result_index, its lookup cells behind those of the unit's gaps before it.  -> H2HIP_OK, or h2hip_trace_seek's refusal
template <class Unit, class Index>
inline int fp_gap_checks(const uint32_t *break_points, size_t num_columns, const UnitShape &sh, uint32_t result_len, const Unit *units,
                         const uint64_t *lookup_slots, size_t count, h2hip_range_check *out, Index index) {
    for (size_t u = 0; u < count; ++u) {
        uint64_t slot = lookup_slots[u];
        for (uint32_t j = 0; j < sh.ngaps; ++j) {
            h2hip_range_check &c = out[index(u, j)];
            const int r = h2hip_trace_seek(break_points, num_columns, units[u].column, units[u].row, sh.gaps[j].cell_offset, &c.column, &c.row);
            if (r != H2HIP_OK) return r;
            c.a_offset = (uint64_t)u * result_len + sh.gaps[j].result_index;
            c.b_offset = 0;
            c.lookup_slot = slot;
            slot += sh.gap_lookups[j];
        }
    }
    return H2HIP_OK;
}
// the *_layout functions' common out-parameters
inline void unit_layout_out(const UnitShape &sh, size_t *num_cells, size_t *num_own_cells, size_t *num_lookup_cells, h2hip_fp_mul_range *ranges) {
    *num_cells = sh.total;
    *num_own_cells = sh.own;
    *num_lookup_cells = sh.num_lookups;
    for (uint32_t j = 0; j < sh.ngaps; ++j) ranges[j] = sh.gaps[j];
}

}  // namespace h2

#undef H2_INL
