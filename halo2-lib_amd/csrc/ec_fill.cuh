// The cells of one ec_add_unequal, ec_sub_unequal (both non-strict) or ec_double of halo2-ecc (include/h2hip.h states the form), as host and device code.  A unit is
// a fixed sequence of segments (a subtraction, one limb of a no-carry product, the load of lambda, one limb of a reduction, ...) that
// ec_prepare lays out once per call from the parameters: the same table gives h2hip_ec_layout its numbers, the place kernel its slots and
// h2hip_ec_range_checks its gaps.  ec_fill.hip's first kernel runs ec_solve_unit in one lane per unit (lambda by an inversion mod p, three
// signed floor divisions by p, the Fr cells of every no-carry value -> a per-unit record and the results entries), its second ec_place_slot in
// one lane per (unit, segment); tools/ec_host_fill.cpp runs both in a loop on one host thread.
#pragma once
#include "fp_mul.cuh"   // the multiword helpers, fp_barrett, fp_carry_step, fp_prepare
#include "modinv.cuh"   // divsteps30, s9_update_fg

namespace h2 {

#define H2_INL __attribute__((always_inline))

constexpr uint32_t EC_MAX_SEGS = 80, EC_MAX_GAPS = UNIT_MAX_GAPS, EC_CONSTS = 2 * FP_MAX_K + 8, EC_REC_REGS = 14;
constexpr int EC_WA = 10;   // words of an operand integer (n k <= 318 bits) and of lambda; a no-carry value has 2 EC_WA

// a CRT value is a "register" of k + 1 Fr (k limb cells, the native cell): registers 0 .. 3 are P.x, P.y, Q.x, Q.y in values_dev, register
// 4 + j is entry j of the unit's record.  In context order:
//   ADD_UNEQUAL  dx dy lambda lambda*dx qc=that-dy lambda^2 that-P.x x3nc=that-Q.x x3 dx13=P.x-x3 lambda*dx13 y3nc=that-P.y y3
//   DOUBLE       2y 3x 3x*x lambda lambda*2y qc=that-3x*x lambda^2 2x x3nc=lambda^2-2x x3 dx=P.x-x3 lambda*dx y3nc=that-P.y y3
//   SUB_UNEQUAL  ADD_UNEQUAL's with sy = Q.y + P.y for dy and qc = lambda*dx + sy: NUM holds sy, the numerator of lambda is -sy
template <uint32_t OP>
struct EcRegs;
template <>
struct EcRegs<H2HIP_EC_ADD_UNEQUAL> {
    enum : uint32_t { DEN = 4, NUM = 5, LAM = 6, LD = 7, QC = 8, LSQ = 9, T1 = 10, X3NC = 11, X3 = 12, DX13 = 13, LDX = 14, Y3NC = 15, Y3 = 16 };
};
template <>
struct EcRegs<H2HIP_EC_SUB_UNEQUAL> : EcRegs<H2HIP_EC_ADD_UNEQUAL> {};
template <>
struct EcRegs<H2HIP_EC_DOUBLE> {
    enum : uint32_t { DEN = 4, THREE_X = 5, NUM = 6, LAM = 7, LD = 8, QC = 9, LSQ = 10, T1 = 11, X3NC = 12, X3 = 13, DX13 = 14, LDX = 15, Y3NC = 16, Y3 = 17 };
};
// behind the registers the record holds, per reduction r < 3 (the zero check of divide_unsafe, the carry_mod of x3, of y3):
// [q_i, i < k] quot_native [check_i] [-c_i]
H2_HD uint32_t ec_red_base(uint32_t k, uint32_t r) { return EC_REC_REGS * (k + 1) + r * (3 * k + 1); }
H2_HD uint32_t ec_record_len(uint32_t k) { return ec_red_base(k, 3); }
// results: x3, y3, lambda (a register each), then per reduction [q_i + B][-c_i + 2^rb_r]
H2_HD uint32_t ec_result_len(uint32_t k) { return 9 * k + 3; }
H2_HD uint32_t ec_result_red(uint32_t k, uint32_t r) { return 3 * k + 3 + 2 * k * r; }

// constants (canonical Montgomery Fr): [m_i, i < k][2^(n i), i < k][2^quot_last_limb_bits][m_nat][-1][2][3][2^rb_r, r < 3]
H2_HD uint32_t ec_c_bl(uint32_t k) { return 2 * k; }
H2_HD uint32_t ec_c_mnat(uint32_t k) { return 2 * k + 1; }
H2_HD uint32_t ec_c_neg1(uint32_t k) { return 2 * k + 2; }
H2_HD uint32_t ec_c_two(uint32_t k) { return 2 * k + 3; }
H2_HD uint32_t ec_c_rb(uint32_t k, uint32_t r) { return 2 * k + 5 + r; }

// one segment of a unit = one lane of the place kernel.  a, b: the registers read, c: the register of the result (SMUL: b is the constant's
// index, no register); i: the limb; red: the reduction
enum : uint8_t { EC_SUB, EC_SMUL, EC_MUL, EC_MULNAT, EC_LOAD, EC_ZC, EC_CM, EC_QSH, EC_CARRY, EC_EVALQ, EC_EVALO, EC_NATZ, EC_NATC, EC_ADD };
struct EcSeg {
    uint32_t off;   // of the segment's first cell in the unit's run
    uint8_t type, i, a, b, c, red, pad0, pad1;
};

// what one call's lanes share
struct EcCall : TraceCall {
    const EcSeg *segs;
    uint32_t n, k;
    uint32_t p[FP_P_WORDS], mu[FP_MU_WORDS];   // wave-uniform: the modulus and its Barrett constant, 32-bit words
    int32_t p30[9];                            // the modulus in 30-bit limbs and -p^-1 mod 2^30, for the division steps
    uint32_t neg_pinv30;
};
H2_CALL_LEADS(EcCall) H2_OFFSET_IS(EcCall, segs, 56) H2_OFFSET_IS(EcCall, n, 64) H2_OFFSET_IS(EcCall, k, 68) H2_OFFSET_IS(EcCall, p, 72)
H2_OFFSET_IS(EcCall, mu, 116) H2_OFFSET_IS(EcCall, p30, 168) H2_OFFSET_IS(EcCall, neg_pinv30, 204)
static_assert(sizeof(EcCall) == 208, "EcCall grew or shrank");

// ---- integers
template <int N>
H2_HD void mp_add(const uint32_t (&a)[N], const uint32_t (&b)[N], uint32_t (&r)[N]) {
    unsigned c = 0;
    static_for<N>([&](auto j) H2_INL { r[decltype(j)::value] = addc32(a[decltype(j)::value], b[decltype(j)::value], c); });
}
template <int N>
H2_HD uint32_t mp_absdiff(const uint32_t (&a)[N], const uint32_t (&b)[N], uint32_t (&r)[N]) {   // |a - b| -> 1 when a < b
    const uint32_t br = mp_sub<N>(a, b, r);
    mp_neg_if<N>(r, br);
    return br;
}
template <int NS, int ND>
H2_HD void mp_widen(const uint32_t (&s)[NS], uint32_t (&d)[ND]) {
    static_for<ND>([&](auto j) H2_INL { d[decltype(j)::value] = mp_at<decltype(j)::value>(s); });
}
// X = sum (canon(cell_i) mod 2^n) 2^(n i)
template <int K>
H2_HD void ec_load_int(const Fr *cells, uint32_t n, uint32_t (&X)[EC_WA]) {
    static_for<EC_WA>([&](auto j) H2_INL { X[decltype(j)::value] = 0; });
    static_for<K>([&](auto i0) H2_INL {
        constexpr int i = K - 1 - decltype(i0)::value;
        const Fr l = range_low_bits(fe_from_mont(cells[i]), n);
        mp_shl<EC_WA>(X, n);
        static_for<4>([&](auto j) H2_INL { X[decltype(j)::value] |= l.l[decltype(j)::value]; });
    });
}
// X = |V| -> the sign of V = (n1 ? -1 : 1) A B - (n2 ? -1 : 1) C, in 672-bit two's complement; |V| < 2^640 for every value a unit forms
H2_HD uint32_t ec_signed_mac(const uint32_t (&A)[EC_WA], const uint32_t (&B)[EC_WA], uint32_t n1, const uint32_t (&C)[2 * EC_WA], uint32_t n2,
                             uint32_t (&X)[2 * EC_WA]) {
    uint32_t V[2 * EC_WA + 1];
    {
        uint32_t T[2 * EC_WA];
        mp_mul<EC_WA, EC_WA>(A, B, T);
        mp_widen(T, V);
    }
    mp_neg_if<2 * EC_WA + 1>(V, n1);
    {
        uint32_t U[2 * EC_WA + 1];
        mp_widen(C, U);
        mp_neg_if<2 * EC_WA + 1>(U, n2 ^ 1u);
        mp_add<2 * EC_WA + 1>(V, U, V);
    }
    const uint32_t sign = V[2 * EC_WA] >> 31;
    mp_neg_if<2 * EC_WA + 1>(V, sign);
    mp_widen(V, X);
    return sign;
}
// (Q, O) = FLOOR divmod of V = (neg ? -X : X) by p (div_mod_floor): Qm = |Q| mod 2^352, neg its sign, 0 <= O < p
H2_HD void ec_floor_div(const EcCall &ec, const uint32_t (&X)[2 * EC_WA], uint32_t neg, uint32_t (&Qm)[EC_WA + 1], uint32_t (&O)[EC_WA + 1]) {
    fp_barrett<EC_WA>(X, ec.p, ec.mu, Qm, O);
    uint32_t any = 0;
    static_for<EC_WA + 1>([&](auto j) H2_INL { any |= O[decltype(j)::value]; });
    const uint32_t adj = neg & (any ? 1u : 0u);   // a negative value with a remainder: |Q| + 1 and p - O
    uint32_t pw[EC_WA + 1], D[EC_WA + 1];
    static_for<EC_WA + 1>([&](auto j) H2_INL { pw[decltype(j)::value] = ec.p[decltype(j)::value]; });
    mp_sub<EC_WA + 1>(pw, O, D);
    unsigned c = adj;
    static_for<EC_WA + 1>([&](auto j) H2_INL {
        O[decltype(j)::value] = adj ? D[decltype(j)::value] : O[decltype(j)::value];
        Qm[decltype(j)::value] = addc32(Qm[decltype(j)::value], 0, c);
    });
}
// (d, e) <- t * (d, e) / 2^30 mod p as modinv.cuh's s9_update_de, the modulus and -p^-1 mod 2^30 being arguments
H2_HD void ec_update_de(S9 &d, S9 &e, int32_t u, int32_t v, int32_t q, int32_t r, const int32_t (&p)[9], uint32_t neg_pinv) {
    int64_t cd = (int64_t)u * d.v[0] + (int64_t)v * e.v[0];
    int64_t ce = (int64_t)q * d.v[0] + (int64_t)r * e.v[0];
    const int32_t md = (int32_t)(((uint32_t)cd * neg_pinv) & (uint32_t)M30);
    const int32_t me = (int32_t)(((uint32_t)ce * neg_pinv) & (uint32_t)M30);
    cd += (int64_t)md * p[0];
    ce += (int64_t)me * p[0];
    cd >>= 30;
    ce >>= 30;
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        cd += (int64_t)u * d.v[i] + (int64_t)v * e.v[i] + (int64_t)md * p[i];
        ce += (int64_t)q * d.v[i] + (int64_t)r * e.v[i] + (int64_t)me * p[i];
        d.v[i - 1] = (int32_t)cd & M30;
        e.v[i - 1] = (int32_t)ce & M30;
        cd >>= 30;
        ce >>= 30;
    }
    d.v[8] = (int32_t)cd;
    e.v[8] = (int32_t)ce;
}
// x^-1 mod p for x < p, p odd and below 2^256, by modinv.cuh's division steps (25 batches of 30); 0 for an x with no inverse (the
// reference's unwrap_or_default): then f does not end at +-1
H2_HD void ec_modinv(const EcCall &ec, const uint32_t (&x)[8], uint32_t (&out)[8]) {
    S9 f, g = s9_from_limbs32<void>(x), d, e;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        f.v[i] = ec.p30[i];
        d.v[i] = 0;
        e.v[i] = 0;
    }
    e.v[0] = 1;
    int32_t delta = 1;
#pragma unroll 1
    for (int batch = 0; batch < 25; ++batch) {
        int32_t u, v, q, r;
        delta = divsteps30(delta, (uint32_t)f.v[0] | ((uint32_t)f.v[1] << 30), (uint32_t)g.v[0] | ((uint32_t)g.v[1] << 30), u, v, q, r);
        s9_update_fg(f, g, u, v, q, r);
        ec_update_de(d, e, u, v, q, r, ec.p30, ec.neg_pinv30);
    }
    const int32_t fneg = f.v[8] >> 31;   // all ones when f < 0
    int32_t not_one = f.v[0] ^ 1, not_minus_one = f.v[0] ^ M30;   // f = 1, 0, .., 0 or f = 2^30 - 1, .., 2^30 - 1, -1 (limbs 0 .. 7 lie in [0, 2^30))
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        not_one |= f.v[i];
        not_minus_one |= f.v[i] ^ (i < 8 ? M30 : -1);
    }
    const bool unit = !not_one || !not_minus_one;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {        // d <- sign(f) * d + 32 p  (positive, < 59 p)
        c += (int64_t)((d.v[i] ^ fneg) - fneg) + ((int64_t)ec.p30[i] << 5);
        d.v[i] = i < 8 ? ((int32_t)c & M30) : (int32_t)c;
        if (i < 8) c >>= 30;
    }
#pragma unroll 1
    for (int k = 5; k >= 0; --k) {       // subtract 32 p, 16 p, ..., p while the result stays non-negative
        S9 t;
        int64_t b = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            b += (int64_t)d.v[i] - ((int64_t)ec.p30[i] << k);
            t.v[i] = i < 8 ? ((int32_t)b & M30) : (int32_t)b;
            if (i < 8) b >>= 30;
        }
        const int32_t keep = t.v[8] >> 31;   // negative: keep d
#pragma unroll
        for (int i = 0; i < 9; ++i) d.v[i] = (d.v[i] & keep) | (t.v[i] & ~keep);
    }
    const uint32_t mask = unit ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int w = 0; w < 8; ++w) {        // 9 x 30 -> 8 x 32
        const int bit = 32 * w, i = bit / 30, off = bit % 30;
        uint64_t acc = (uint64_t)(uint32_t)d.v[i] >> off;
        acc |= (uint64_t)(uint32_t)d.v[i + 1] << (30 - off);
        if (i + 2 < 9) acc |= (uint64_t)(uint32_t)d.v[i + 2] << (60 - off);
        out[w] = (uint32_t)acc & mask;
    }
}

// ---- Fr cells of the no-carry values, register to register (k + 1 cells each)
template <int K>
H2_HD void ec_sub_cells(const Fr *a, const Fr *b, Fr *out) {
    static_for<K + 1>([&](auto i) H2_INL { out[decltype(i)::value] = fe_sub(a[decltype(i)::value], b[decltype(i)::value]); });
}
template <int K>
H2_HD void ec_add_cells(const Fr *a, const Fr *b, Fr *out) {
    static_for<K + 1>([&](auto i) H2_INL { out[decltype(i)::value] = fe_add(a[decltype(i)::value], b[decltype(i)::value]); });
}
template <int K>
H2_HD void ec_smul_cells(const Fr *a, const Fr &c, Fr *out) {
    static_for<K + 1>([&](auto i) H2_INL { out[decltype(i)::value] = fe_mul(a[decltype(i)::value], c); });
}
template <int K>
H2_HD void ec_mul_cells(const Fr *a, const Fr *b, Fr *out) {
    Fr x[K], y[K];
    static_for<K>([&](auto i) H2_INL {
        x[decltype(i)::value] = a[decltype(i)::value];
        y[decltype(i)::value] = b[decltype(i)::value];
    });
    const Fr nat = fe_mul(a[K], b[K]);
    static_for<K>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value;
        Fr s = Fr::zero();
        static_for<i + 1>([&](auto j0) H2_INL { s = fe_add(s, fe_mul(x[decltype(j0)::value], y[i - decltype(j0)::value])); });
        out[i] = s;
    });
    out[K] = nat;
}
H2_HD const Fr *ec_reg(const EcCall &ec, const h2hip_ec_op &unit, const Fr *rec, uint32_t r) {
    const uint32_t k1 = ec.k + 1;
    return r < 2 ? ec.values + unit.p_offset + r * k1 : r < 4 ? ec.values + unit.q_offset + (r - 2) * k1 : rec + (r - 4) * k1;
}

// the cells of reduction RED from (Q, O): q_i = the low k limbs of |Q|, negated in Fr for a negative Q (decompose_bigint); o_i alike (CM);
// check_i = prod_i - a_i (+ o_i) in Fr over the cells a_i; the carries by fp_carry_step; the natives by evaluate_native's sums
template <int K, uint32_t RED, bool CM>
H2_HD void ec_reduce_cells(const EcCall &ec, Fr *rec, Fr *res, const Fr *a, Fr *oreg, Fr *ores, uint32_t (&Qm)[EC_WA + 1], uint32_t qneg,
                           uint32_t (&O)[EC_WA + 1]) {
    const Fr *cs = ec.consts;
    const uint32_t n = ec.n;
    Fr *rr = rec + ec_red_base(K, RED);
    Fr q[K], o[K];
    static_for<K>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value;
        const Fr t = fe_to_mont(mp_low_limb<EC_WA + 1>(Qm, n)), tn = fe_neg(t);
        q[i] = qneg ? tn : t;
        mp_shr<EC_WA + 1>(Qm, n);
        rr[i] = q[i];
        if (res) res[ec_result_red(K, RED) + i] = fe_add(q[i], i == K - 1 ? cs[ec_c_bl(K)] : cs[K + 1]);
        if constexpr (CM) {
            o[i] = fe_to_mont(mp_low_limb<EC_WA + 1>(O, n));
            mp_shr<EC_WA + 1>(O, n);
            oreg[i] = o[i];
            if (res) ores[i] = o[i];
        }
    });
    uint32_t cw[9];
    static_for<9>([&](auto j) H2_INL { cw[decltype(j)::value] = 0; });
    static_for<K>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value;
        Fr prod = Fr::zero();
        static_for<i + 1>([&](auto j0) H2_INL { prod = fe_add(prod, fe_mul(q[decltype(j0)::value], cs[i - decltype(j0)::value])); });
        Fr check = fe_sub(prod, a[i]);
        if constexpr (CM) check = fe_add(check, o[i]);
        rr[K + 1 + i] = check;
        const Fr negc = fp_carry_step(check, cw, n);
        rr[2 * K + 1 + i] = negc;
        if (res) res[ec_result_red(K, RED) + K + i] = fe_add(negc, cs[ec_c_rb(K, RED)]);
    });
    Fr qn = q[0], on = Fr::zero();
    if constexpr (CM) on = o[0];
    static_for<K - 1>([&](auto i0) H2_INL {
        constexpr int i = decltype(i0)::value + 1;
        qn = fe_add(qn, fe_mul(q[i], cs[K + i]));
        if constexpr (CM) on = fe_add(on, fe_mul(o[i], cs[K + i]));
    });
    rr[K] = qn;
    if constexpr (CM) {
        oreg[K] = on;
        if (res) ores[K] = on;
    }
}

// the denominator and the numerator of lambda as integers: ADD_UNEQUAL X2 - X1 and Y2 - Y1, SUB_UNEQUAL X2 - X1 and -(Y2 + Y1) (neg_divide_unsafe:
// the zero check lambda den - num is then lambda (X2 - X1) + (Y2 + Y1)), DOUBLE 2 Y and 3 X X
template <int K, uint32_t OP>
H2_HD void ec_den_num(const EcCall &ec, const Fr *P, const Fr *Q, uint32_t (&den)[EC_WA], uint32_t &sden, uint32_t (&num)[2 * EC_WA], uint32_t &snum) {
    if constexpr (OP != H2HIP_EC_DOUBLE) {
        uint32_t A[EC_WA], B[EC_WA], D[EC_WA];
        ec_load_int<K>(P, ec.n, A);
        ec_load_int<K>(Q, ec.n, B);
        sden = mp_absdiff<EC_WA>(B, A, den);
        ec_load_int<K>(P + K + 1, ec.n, A);
        ec_load_int<K>(Q + K + 1, ec.n, B);
        if constexpr (OP == H2HIP_EC_ADD_UNEQUAL)
            snum = mp_absdiff<EC_WA>(B, A, D);
        else {
            mp_add<EC_WA>(B, A, D);   // Y2 + Y1 < 2^319 (n k <= 318)
            snum = 1;
        }
        mp_widen(D, num);
    } else {
        uint32_t A[EC_WA], T[EC_WA];
        ec_load_int<K>(P + K + 1, ec.n, A);
        mp_add<EC_WA>(A, A, den);
        ec_load_int<K>(P, ec.n, A);
        mp_add<EC_WA>(A, A, T);
        mp_add<EC_WA>(T, A, T);   // 3 X < 2^320 (n k <= 318)
        mp_mul<EC_WA, EC_WA>(T, A, num);
        sden = snum = 0;
    }
}

// ---- one unit: stage by stage, each stage's cells written to the record before the next begins (a later stage reads them back: the live
// state is one stage's)
template <int K, uint32_t OP>
H2_HD void ec_solve_unit(const EcCall &ec, const h2hip_ec_op &unit, uint32_t u) {
    using R = EcRegs<OP>;
    constexpr uint32_t K1 = K + 1;
    const uint32_t n = ec.n;
    const Fr *cs = ec.consts, *P = ec.values + unit.p_offset, *Q = nullptr;
    if constexpr (OP != H2HIP_EC_DOUBLE) Q = ec.values + unit.q_offset;   // (ignored for DOUBLE: not even formed)
    Fr *rec = ec.rec + (size_t)u * ec_record_len(K);
    Fr *res = ec.results ? ec.results + (size_t)u * ec_result_len(K) : nullptr;
    const auto reg = [&](uint32_t r) H2_INL { return rec + (r - 4) * K1; };
    // -- the cells of denominator and numerator
    if constexpr (OP == H2HIP_EC_ADD_UNEQUAL) {
        ec_sub_cells<K>(Q, P, reg(R::DEN));
        ec_sub_cells<K>(Q + K1, P + K1, reg(R::NUM));
    } else if constexpr (OP == H2HIP_EC_SUB_UNEQUAL) {
        ec_sub_cells<K>(Q, P, reg(R::DEN));
        ec_add_cells<K>(Q + K1, P + K1, reg(R::NUM));
    } else {
        ec_smul_cells<K>(P + K1, cs[ec_c_two(K)], reg(R::DEN));
        ec_smul_cells<K>(P, cs[ec_c_two(K) + 1], reg(R::THREE_X));
        ec_mul_cells<K>(reg(R::THREE_X), P, reg(R::NUM));
    }
    // -- lambda = (num mod p) (den mod p)^-1 mod p
    {
        uint32_t lam[8];
        {
            uint32_t den[EC_WA], num[2 * EC_WA], sden, snum, Qm[EC_WA + 1], O[EC_WA + 1], inv[8], nm[8];
            ec_den_num<K, OP>(ec, P, Q, den, sden, num, snum);
            ec_floor_div(ec, num, snum, Qm, O);
            static_for<8>([&](auto j) H2_INL { nm[decltype(j)::value] = O[decltype(j)::value]; });
            uint32_t X[2 * EC_WA];
            mp_widen(den, X);
            ec_floor_div(ec, X, sden, Qm, O);
            uint32_t d8[8];
            static_for<8>([&](auto j) H2_INL { d8[decltype(j)::value] = O[decltype(j)::value]; });
            ec_modinv(ec, d8, inv);
            uint32_t T[16];
            mp_mul<8, 8>(nm, inv, T);
            mp_widen(T, X);
            ec_floor_div(ec, X, 0, Qm, O);
            static_for<8>([&](auto j) H2_INL { lam[decltype(j)::value] = O[decltype(j)::value]; });
        }
        uint32_t L[EC_WA + 1];
        mp_widen(lam, L);
        Fr *lr = reg(R::LAM);
        Fr nat = Fr::zero();
        static_for<K>([&](auto i0) H2_INL {
            constexpr int i = decltype(i0)::value;
            const Fr l = fe_to_mont(mp_low_limb<EC_WA + 1>(L, n));
            mp_shr<EC_WA + 1>(L, n);
            nat = i ? fe_add(nat, fe_mul(l, cs[K + i])) : l;
            lr[i] = l;
            if (res) res[2 * K1 + i] = l;
        });
        lr[K] = nat;
        if (res) res[2 * K1 + K] = nat;
    }
    // -- divide_unsafe's constraint: lambda den - num carries to zero mod p (SUB_UNEQUAL: neg_divide_unsafe's, lambda den + sy)
    {
        ec_mul_cells<K>(reg(R::LAM), reg(R::DEN), reg(R::LD));
        if constexpr (OP == H2HIP_EC_SUB_UNEQUAL)
            ec_add_cells<K>(reg(R::LD), reg(R::NUM), reg(R::QC));
        else
            ec_sub_cells<K>(reg(R::LD), reg(R::NUM), reg(R::QC));
        uint32_t Qm[EC_WA + 1], O[EC_WA + 1], sign;
        {
            uint32_t den[EC_WA], num[2 * EC_WA], lam[EC_WA], X[2 * EC_WA], sden, snum;
            ec_den_num<K, OP>(ec, P, Q, den, sden, num, snum);
            ec_load_int<K>(reg(R::LAM), n, lam);
            sign = ec_signed_mac(lam, den, sden, num, snum, X);
            ec_floor_div(ec, X, sign, Qm, O);
        }
        ec_reduce_cells<K, 0, false>(ec, rec, res, reg(R::QC), nullptr, nullptr, Qm, sign, O);
    }
    // -- x3 = lambda^2 - x1 - x2 (- 2 x)
    {
        ec_mul_cells<K>(reg(R::LAM), reg(R::LAM), reg(R::LSQ));
        if constexpr (OP != H2HIP_EC_DOUBLE) {
            ec_sub_cells<K>(reg(R::LSQ), P, reg(R::T1));
            ec_sub_cells<K>(reg(R::T1), Q, reg(R::X3NC));
        } else {
            ec_smul_cells<K>(P, cs[ec_c_two(K)], reg(R::T1));
            ec_sub_cells<K>(reg(R::LSQ), reg(R::T1), reg(R::X3NC));
        }
        uint32_t Qm[EC_WA + 1], O[EC_WA + 1], sign;
        {
            uint32_t lam[EC_WA], A[EC_WA], B[EC_WA], C[2 * EC_WA], X[2 * EC_WA];
            ec_load_int<K>(P, n, A);
            if constexpr (OP != H2HIP_EC_DOUBLE)
                ec_load_int<K>(Q, n, B);
            else
                static_for<EC_WA>([&](auto j) H2_INL { B[decltype(j)::value] = A[decltype(j)::value]; });
            mp_add<EC_WA>(A, B, A);
            mp_widen(A, C);
            ec_load_int<K>(reg(R::LAM), n, lam);
            sign = ec_signed_mac(lam, lam, 0, C, 0, X);
            ec_floor_div(ec, X, sign, Qm, O);
        }
        ec_reduce_cells<K, 1, true>(ec, rec, res, reg(R::X3NC), reg(R::X3), res, Qm, sign, O);
    }
    // -- y3 = lambda (x1 - x3) - y1
    {
        ec_sub_cells<K>(P, reg(R::X3), reg(R::DX13));
        ec_mul_cells<K>(reg(R::LAM), reg(R::DX13), reg(R::LDX));
        ec_sub_cells<K>(reg(R::LDX), P + K1, reg(R::Y3NC));
        uint32_t Qm[EC_WA + 1], O[EC_WA + 1], sign;
        {
            uint32_t lam[EC_WA], A[EC_WA], B[EC_WA], D[EC_WA], C[2 * EC_WA], X[2 * EC_WA];
            ec_load_int<K>(P, n, A);
            ec_load_int<K>(reg(R::X3), n, B);
            const uint32_t sd = mp_absdiff<EC_WA>(A, B, D);
            ec_load_int<K>(P + K1, n, A);
            mp_widen(A, C);
            ec_load_int<K>(reg(R::LAM), n, lam);
            sign = ec_signed_mac(lam, D, sd, C, 0, X);
            ec_floor_div(ec, X, sign, Qm, O);
        }
        ec_reduce_cells<K, 2, true>(ec, rec, res, reg(R::Y3NC), reg(R::Y3), res ? res + K1 : nullptr, Qm, sign, O);
    }
}

// ---- one segment of one unit; each lane recomputes its own running sums from the record
H2_HD void ec_place_slot(const EcCall &ec, const h2hip_ec_op &unit, uint32_t u, uint32_t slot) {
    const uint32_t k = ec.k;
    const EcSeg sg = ec.segs[slot];
    const Fr *cs = ec.consts, *rec = ec.rec + (size_t)u * ec_record_len(k);
    // (registers 2 and 3, Q's, occur in ADD_UNEQUAL's and SUB_UNEQUAL's tables only; SMUL's b is no register)
    const Fr *a = ec_reg(ec, unit, rec, sg.a), *b = sg.type == EC_SMUL ? nullptr : ec_reg(ec, unit, rec, sg.b), *c = ec_reg(ec, unit, rec, sg.c);
    const Fr *rr = rec + ec_red_base(k, sg.red), *q = rr, *check = rr + k + 1, *negc = rr + 2 * k + 1;
    const Fr zero = Fr::zero(), one = Fr::one();
    const uint32_t i = sg.i;
    TraceOut out = trace_at(ec.tc, unit.column, unit.row, sg.off);
    switch (sg.type) {
    case EC_SUB:   // per cell of the registers: out = a - b, b, 1, a
        for (uint32_t j = 0; j <= k; ++j) {
            out.put(c[j]);
            out.put(b[j]);
            out.put(one);
            out.put(a[j]);
        }
        break;
    case EC_ADD:   // per cell of the registers: a, b, 1, out = a + b
        for (uint32_t j = 0; j <= k; ++j) {
            out.put(a[j]);
            out.put(b[j]);
            out.put(one);
            out.put(c[j]);
        }
        break;
    case EC_SMUL:   // 0, a, Constant, out
        for (uint32_t j = 0; j <= k; ++j) {
            out.put(zero);
            out.put(a[j]);
            out.put(cs[sg.b]);
            out.put(c[j]);
        }
        break;
    case EC_MUL: {   // ip(a_0 .. a_i; b_i .. b_0)
        Fr acc = zero;
        out.put(acc);
        for (uint32_t j = 0; j <= i; ++j) {
            const Fr x = a[j], y = b[i - j];
            acc = fe_add(acc, fe_mul(x, y));
            out.put(x);
            out.put(y);
            out.put(acc);
        }
        break;
    }
    case EC_MULNAT:
        out.put(zero);
        out.put(a[k]);
        out.put(b[k]);
        out.put(c[k]);
        break;
    case EC_LOAD:
    case EC_EVALO:
    case EC_EVALQ: {   // (LOAD: the k witness cells first) x_0, x_1, 2^n, s_1, ...
        const Fr *x = sg.type == EC_EVALQ ? q : a;
        if (sg.type == EC_LOAD)
            for (uint32_t j = 0; j < k; ++j) out.put(x[j]);
        Fr acc = x[0];
        out.put(acc);
        for (uint32_t j = 1; j < k; ++j) {
            const Fr y = cs[k + j];
            acc = fe_add(acc, fe_mul(x[j], y));
            out.put(x[j]);
            out.put(y);
            out.put(acc);
        }
        break;
    }
    case EC_ZC:
    case EC_CM: {   // ip(q_0 .. q_i; m_i .. m_0), then -1, a_i, prod_i - a_i (CM: 1, o_i, check_i)
        Fr acc = zero;
        out.put(acc);
        for (uint32_t j = 0; j <= i; ++j) {
            const Fr x = q[j], y = cs[i - j];
            acc = fe_add(acc, fe_mul(x, y));
            out.put(x);
            out.put(y);
            out.put(acc);
        }
        out.put(cs[ec_c_neg1(k)]);
        out.put(a[i]);
        out.put(fe_sub(acc, a[i]));
        if (sg.type == EC_CM) {
            out.put(one);
            out.put(b[i]);
            out.put(check[i]);
        }
        break;
    }
    case EC_QSH: {   // q_i, B, 1, q_i + B
        const Fr base = i == k - 1 ? cs[ec_c_bl(k)] : cs[k + 1];
        out.put(q[i]);
        out.put(base);
        out.put(one);
        out.put(fe_add(q[i], base));
        break;
    }
    case EC_CARRY: {   // check_i, -c_i, 2^n, -c_{i-1}; -c_i, 2^rb, 1, -c_i + 2^rb
        const Fr nc = negc[i], shift = cs[ec_c_rb(k, sg.red)];
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
        break;
    }
    case EC_NATZ:   // 0, m_nat, quot_native, a_nat
        out.put(zero);
        [[fallthrough]];
    default:        // EC_NATC: (out_native,) m_nat, quot_native, a_nat
        out.put(cs[ec_c_mnat(k)]);
        out.put(rr[k]);
        out.put(a[k]);
        break;
    }
}

// ---- what the host derives from the parameters and the operation, once per call (host only)
struct EcShape : UnitShape {
    FpShape fp;
    uint32_t op, k, nsegs;
    uint32_t rb[3], limb_bits_max[3];
    EcSeg segs[EC_MAX_SEGS];
    uint32_t out_offsets[3 * (FP_MAX_K + 1)];
};
struct EcBuilder {
    EcShape &s;
    uint32_t n, k, lb, pbits, at = 0;
    const char *bad = nullptr;
    void seg(uint8_t type, uint32_t i, uint32_t a, uint32_t b, uint32_t c, uint32_t red, uint32_t cells) {
        s.segs[s.nsegs++] = EcSeg{at, type, (uint8_t)i, (uint8_t)a, (uint8_t)b, (uint8_t)c, (uint8_t)red, 0, 0};
        at += cells;
    }
    void gap(uint32_t bits, uint32_t result) {
        const uint32_t L = (bits + lb - 1) / lb, rem = bits % lb;
        if ((uint64_t)L * lb > FP_CAPACITY) bad = "the limbs of a range check take more than 253 bits (F::CAPACITY)";
        s.gaps[s.ngaps] = h2hip_fp_mul_range{at, range_unit_cells(L, rem, 0), bits, result};
        s.gap_lookups[s.ngaps++] = range_unit_lookups(L, rem);
        at += range_unit_cells(L, rem, 0);
    }
    // each returns the max_limb_bits of its result (bigint/sub_no_carry.rs:21, add_no_carry.rs:22, scalar_mul_no_carry.rs:17, mul_no_carry.rs:34)
    uint32_t add(uint32_t a, uint32_t b, uint32_t out, uint32_t ma, uint32_t mb) {
        seg(EC_ADD, 0, a, b, out, 0, 4 * (k + 1));
        return std::max(ma, mb) + 1;
    }
    uint32_t sub(uint32_t a, uint32_t b, uint32_t out, uint32_t ma, uint32_t mb) {
        seg(EC_SUB, 0, a, b, out, 0, 4 * (k + 1));
        return std::max(ma, mb) + 1;
    }
    uint32_t smul(uint32_t a, uint32_t constant, uint32_t clog, uint32_t out, uint32_t ma) {
        seg(EC_SMUL, 0, a, constant, out, 0, 4 * (k + 1));
        return ma + clog;
    }
    uint32_t mul(uint32_t a, uint32_t b, uint32_t out, uint32_t ma, uint32_t mb) {
        const uint32_t log2_ceil = k == 2 ? 1 : 2;
        if (log2_ceil + ma + mb > FP_NUM_BITS - 2) bad = "ceil(log2 num_limbs) + max_limb_bits of both factors > 252 for a product of the operation";
        for (uint32_t i = 0; i < k; ++i) seg(EC_MUL, i, a, b, out, 0, 3 * (i + 1) + 1);
        seg(EC_MULNAT, 0, a, b, out, 0, 4);
        return log2_ceil + ma + mb;
    }
    void load(uint32_t r) {   // FpChip::load_private: the limbs, evaluate_native, the range checks
        for (uint32_t i = 0; i < k; ++i) s.out_offsets[2 * (k + 1) + i] = at + i;
        seg(EC_LOAD, 0, r, r, r, 0, k + 3 * k - 2);
        s.out_offsets[2 * (k + 1) + k] = at - 1;
        for (uint32_t i = 0; i < k; ++i) gap(i == k - 1 ? pbits - n * (k - 1) : n, 2 * (k + 1) + i);
    }
    // o == 0: check_carry_mod_to_zero, else carry_mod into register o, entry x of the results (0: x3, 1: y3)
    void reduce(uint32_t red, uint32_t a, uint32_t o, uint32_t x, uint32_t ma) {
        const uint32_t bit_len = k == 4 ? 3 : 2, cm = o ? 1 : 0;
        const uint32_t mlb = cm ? std::max(std::max(n, ma) + 1, 2 * n + bit_len) : std::max(ma, 2 * n + bit_len);
        s.limb_bits_max[red] = mlb;
        s.rb[red] = (mlb - n + 1 + lb) / lb * lb - 1;
        for (uint32_t i = 0; i < k; ++i) {
            seg(cm ? EC_CM : EC_ZC, i, a, o ? o : a, a, red, 3 * (i + 1) + 1 + (cm ? 6 : 3));
            if (cm) s.out_offsets[x * (k + 1) + i] = at - 2;
        }
        if (cm)
            for (uint32_t i = 0; i < k; ++i) gap(i == k - 1 ? s.fp.out_last_bits : n, x * (k + 1) + i);
        for (uint32_t i = 0; i < k; ++i) {
            seg(EC_QSH, i, a, a, a, red, 4);
            gap((i == k - 1 ? s.fp.quot_last_bits : n) + 1, ec_result_red(k, red) + i);
        }
        for (uint32_t i = 0; i < k; ++i) {
            seg(EC_CARRY, i, a, a, a, red, 8);
            gap(s.rb[red] + 1, ec_result_red(k, red) + k + i);
        }
        seg(EC_EVALQ, 0, a, a, a, red, 3 * k - 2);
        if (cm) {
            seg(EC_EVALO, 0, o, o, o, red, 3 * k - 2);
            s.out_offsets[x * (k + 1) + k] = at - 1;
            seg(EC_NATC, 0, a, a, a, red, 3);
        } else
            seg(EC_NATZ, 0, a, a, a, red, 4);
    }
};
// nullptr when the parameters and the operation are served, else the reason.  ec, consts (EC_CONSTS entries): optional
inline const char *ec_prepare(const h2hip_fp_params &pr, uint32_t op, EcShape &sh, EcCall *ec, Fr *consts) {
    if (op != H2HIP_EC_ADD_UNEQUAL && op != H2HIP_EC_DOUBLE && op != H2HIP_EC_SUB_UNEQUAL) return "unknown op";
    FpCall fc;
    Fr fcs[FP_CONSTS];
    const char *bad = fp_prepare(pr, sh.fp, &fc, fcs);
    if (bad) return bad;
    const uint32_t n = sh.fp.n, k = sh.fp.k, pbits = fp_words_bits(fc.p, FP_P_WORDS);
    if (k < 3) return "num_limbs outside 3 .. 4";
    if (pbits > 256) return "the modulus has more than 256 bits (lambda's inversion)";
    if (!(fc.p[0] & 1)) return "the modulus is even (lambda's inversion)";
    if (n * k > 318) return "limb_bits * num_limbs > 318 (3 x^2 passes 2^640)";
    sh.op = op;
    sh.k = k;
    sh.nsegs = sh.ngaps = 0;
    EcBuilder b{sh, n, k, sh.fp.lb, pbits};
    if (op != H2HIP_EC_DOUBLE) {   // ecc/mod.rs:153-179, fields/mod.rs:217-238; SUB_UNEQUAL: ecc/mod.rs:219-246, fields/mod.rs:256-277
        using R = EcRegs<H2HIP_EC_ADD_UNEQUAL>;
        const bool sub = op == H2HIP_EC_SUB_UNEQUAL;
        const uint32_t dx = b.sub(2, 0, R::DEN, n, n), dy = sub ? b.add(3, 1, R::NUM, n, n) : b.sub(3, 1, R::NUM, n, n);
        b.load(R::LAM);
        const uint32_t ld = b.mul(R::LAM, R::DEN, R::LD, n, dx), qc = sub ? b.add(R::LD, R::NUM, R::QC, ld, dy) : b.sub(R::LD, R::NUM, R::QC, ld, dy);
        b.reduce(0, R::QC, 0, 0, qc);
        const uint32_t lsq = b.mul(R::LAM, R::LAM, R::LSQ, n, n), t1 = b.sub(R::LSQ, 0, R::T1, lsq, n), x3nc = b.sub(R::T1, 2, R::X3NC, t1, n);
        b.reduce(1, R::X3NC, R::X3, 0, x3nc);
        const uint32_t dx13 = b.sub(0, R::X3, R::DX13, n, n), ldx = b.mul(R::LAM, R::DX13, R::LDX, n, dx13), y3nc = b.sub(R::LDX, 1, R::Y3NC, ldx, n);
        b.reduce(2, R::Y3NC, R::Y3, 1, y3nc);
    } else {   // ecc/mod.rs:302-327
        using R = EcRegs<H2HIP_EC_DOUBLE>;
        const uint32_t two_y = b.smul(1, ec_c_two(k), 1, R::DEN, n), three_x = b.smul(0, ec_c_two(k) + 1, 2, R::THREE_X, n);
        const uint32_t num = b.mul(R::THREE_X, 0, R::NUM, three_x, n);
        b.load(R::LAM);
        const uint32_t ld = b.mul(R::LAM, R::DEN, R::LD, n, two_y), qc = b.sub(R::LD, R::NUM, R::QC, ld, num);
        b.reduce(0, R::QC, 0, 0, qc);
        const uint32_t lsq = b.mul(R::LAM, R::LAM, R::LSQ, n, n), two_x = b.smul(0, ec_c_two(k), 1, R::T1, n), x3nc = b.sub(R::LSQ, R::T1, R::X3NC, lsq, two_x);
        b.reduce(1, R::X3NC, R::X3, 0, x3nc);
        const uint32_t dx = b.sub(0, R::X3, R::DX13, n, n), ldx = b.mul(R::LAM, R::DX13, R::LDX, n, dx), y3nc = b.sub(R::LDX, 1, R::Y3NC, ldx, n);
        b.reduce(2, R::Y3NC, R::Y3, 1, y3nc);
    }
    if (b.bad) return b.bad;
    sh.total = b.at;
    sh.own = sh.total;
    sh.num_lookups = 0;
    for (uint32_t j = 0; j < sh.ngaps; ++j) {
        sh.own -= sh.gaps[j].num_cells;
        sh.num_lookups += sh.gap_lookups[j];
    }
    if (consts) {
        for (uint32_t i = 0; i < 2 * k; ++i) consts[i] = fcs[i];
        consts[ec_c_bl(k)] = fcs[2 * k];
        consts[ec_c_mnat(k)] = fcs[2 * k + 2];
        consts[ec_c_neg1(k)] = fcs[2 * k + 3];
        consts[ec_c_two(k)] = fe_add(Fr::one(), Fr::one());
        consts[ec_c_two(k) + 1] = fe_add(consts[ec_c_two(k)], Fr::one());
        for (uint32_t r = 0; r < 3; ++r) consts[ec_c_rb(k, r)] = pow2_mont(sh.rb[r]);
    }
    if (ec) {
        ec->n = n;
        ec->k = k;
        for (uint32_t j = 0; j < FP_P_WORDS; ++j) ec->p[j] = fc.p[j];
        for (uint32_t j = 0; j < FP_MU_WORDS; ++j) ec->mu[j] = fc.mu[j];
        for (int i = 0; i < 9; ++i) {
            const int bit = 30 * i, w = bit >> 5, off = bit & 31;
            const uint64_t lo = fc.p[w], hi = fc.p[w + 1];
            ec->p30[i] = (int32_t)((((hi << 32) | lo) >> off) & (uint64_t)M30);
        }
        uint32_t x = fc.p[0];   // p^-1 mod 2^32 by Newton's iteration (p is odd: p p = 1 mod 8)
        for (int it = 0; it < 5; ++it) x *= 2u - fc.p[0] * x;
        ec->neg_pinv30 = (0u - x) & (uint32_t)M30;
    }
    return nullptr;
}
// the distinct widths of the gaps in the order of their first appearance: h2hip_ec_range_checks' groups -> their number
inline uint32_t ec_width_groups(const EcShape &sh, uint32_t (&width)[EC_MAX_GAPS], uint32_t (&group_of)[EC_MAX_GAPS], uint32_t (&gaps_in)[EC_MAX_GAPS]) {
    uint32_t ng = 0;
    for (uint32_t j = 0; j < sh.ngaps; ++j) {
        uint32_t g = 0;
        while (g < ng && width[g] != sh.gaps[j].range_bits) ++g;
        if (g == ng) {
            width[ng] = sh.gaps[j].range_bits;
            gaps_in[ng++] = 0;
        }
        group_of[j] = g;
        ++gaps_in[g];
    }
    return ng;
}

#undef H2_INL

}  // namespace h2
