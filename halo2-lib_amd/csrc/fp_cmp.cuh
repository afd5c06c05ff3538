// The cells of FpChip's comparisons (include/h2hip.h states the form): enforce_less_than_p of one or both operands and big_is_equal::assign of
// the two, as host and device code.  fp_cmp.hip's first kernel runs cmp_solve_unit in one lane per unit (the s_i, the limbs l_i the range
// checks end in, the borrow chain, the differences and the partial products -> a per-unit record and the results entries), its second
// cmp_place_slot in one lane per (unit, segment), each is_zero segment inverting its own cell; tools/ec_host_fill.cpp runs both in a loop on
// one host thread.  cmp_prepare is what the host derives from h2hip_fp_params and the mask once per call.
#pragma once
#include "fp_mul.cuh"   // fp_prepare, FpShape, the gaps' struct; range_fill.cuh's decomposition with it

namespace h2 {

constexpr uint32_t CMP_MAX_SEGS = 5 * FP_MAX_K, CMP_MAX_GAPS = 2 * FP_MAX_K, CMP_CONSTS = FP_MAX_K + 2;

// one segment of a unit = one lane of the place kernel.  e: the enforced operand (0: a, 1: b), i: the limb
//   CMP_LT   (i >= 1: p_i, borrow_{i-1}, 1, t_i;) s_i, t_i, 1, a_i + 2^pad, -2^pad, 1, a_i                  [fp.rs:123-142, range/mod.rs:662-680]
//   CMP_ISZ  z, l_i, inv, 1, 0, l_i, z, 0 behind the gap of s_i's range check                               [flex_gate/mod.rs:789-809]
//   CMP_EQ   a_i - b_i, b_i, 1, a_i; is_zero of the difference; (i >= 1: 0, eq_i, partial_{i-1}, partial_i)  [big_is_equal.rs]
enum : uint8_t { CMP_LT, CMP_ISZ, CMP_EQ };
struct CmpSeg {
    uint32_t off;   // of the segment's first cell in the unit's run
    uint8_t type, i, e, pad0;
};

// the record of a unit: per enforced operand e [s_i][l_i][borrow_i] at 3 k e, then [a_i - b_i][eq_i][partial_i] at 6 k
H2_HD uint32_t cmp_record_len(uint32_t k) { return 9 * k; }
// results: per enforced operand, in order, s_0 .. s_{k-1} and the final borrow; for EQUAL the equality cell's value
H2_HD uint32_t cmp_result_len(uint32_t k, uint32_t op) {
    return (k + 1) * ((op & H2HIP_FP_CMP_REDUCE_A ? 1 : 0) + (op & H2HIP_FP_CMP_REDUCE_B ? 1 : 0)) + (op & H2HIP_FP_CMP_EQUAL ? 1 : 0);
}

// what one call's lanes share.  consts (canonical Montgomery Fr): [m_i, i < k][2^pad][-2^pad]
struct CmpCall : TraceCall {
    const CmpSeg *segs;
    uint32_t k, op, pad, lb;
};
H2_CALL_LEADS(CmpCall) H2_OFFSET_IS(CmpCall, segs, 56) H2_OFFSET_IS(CmpCall, k, 64) H2_OFFSET_IS(CmpCall, op, 68) H2_OFFSET_IS(CmpCall, pad, 72)
H2_OFFSET_IS(CmpCall, lb, 76)
static_assert(sizeof(CmpCall) == 80, "CmpCall grew or shrank");

// c ? a : b word by word (a ?: over two Fr objects selects between their addresses and sends both to scratch)
H2_HD Fr cmp_select(bool c, const Fr &a, const Fr &b) {
    Fr r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.l[j] = c ? a.l[j] : b.l[j];
    return r;
}
// is_zero's witnesses: z = [x == 0]
H2_HD Fr cmp_flag(const Fr &x) { return cmp_select(x == Fr::zero(), Fr::one(), Fr::zero()); }

// ---- one unit: no inversion here (each is_zero segment's lane does its own)
H2_HD void cmp_solve_unit(const CmpCall &cc, const h2hip_fp_mul &unit, uint32_t u) {
    const uint32_t k = cc.k;
    const Fr *cs = cc.consts;
    Fr *rec = cc.rec + (size_t)u * cmp_record_len(k);
    Fr *res = cc.results ? cc.results + (size_t)u * cmp_result_len(k, cc.op) : nullptr;
    uint32_t at = 0;
    for (uint32_t e = 0; e < 2; ++e) {
        if (!(cc.op & (e ? H2HIP_FP_CMP_REDUCE_B : H2HIP_FP_CMP_REDUCE_A))) continue;
        const Fr *x = cc.values + (e ? unit.b_offset : unit.a_offset);
        Fr *r = rec + 3 * k * e, borrow = Fr::zero();
        for (uint32_t i = 0; i < k; ++i) {
            // s_i = a_i + 2^pad - t_i in Fr over the cells; l_i = the limb the range check of s_i at pad + lb bits ends in (range_slot's)
            const Fr t = i ? fe_add(cs[i], borrow) : cs[0], s = fe_sub(fe_add(x[i], cs[k]), t);
            const Fr l = range_from_u64(range_bits_at(fe_from_mont(s), cc.pad, cc.lb));
            borrow = cmp_flag(l);
            r[i] = s;
            r[k + i] = l;
            r[2 * k + i] = borrow;
            if (res) res[at + i] = s;
        }
        if (res) res[at + k] = borrow;
        at += k + 1;
    }
    if (cc.op & H2HIP_FP_CMP_EQUAL) {
        const Fr *a = cc.values + unit.a_offset, *b = cc.values + unit.b_offset;
        Fr *r = rec + 6 * k, partial = Fr::one();
        for (uint32_t i = 0; i < k; ++i) {
            const Fr d = fe_sub(a[i], b[i]), eq = cmp_flag(d);
            partial = i ? fe_mul(eq, partial) : eq;
            r[i] = d;
            r[k + i] = eq;
            r[2 * k + i] = partial;
        }
        if (res) res[at] = partial;
    }
}

// ---- one segment of one unit.  is_zero(x): z, x, inv, 1, 0, x, z, 0 with inv = x^-1 in Fr, 1 for x = 0 (one inversion per lane)
H2_HD void cmp_place_slot(const CmpCall &cc, const h2hip_fp_mul &unit, uint32_t u, uint32_t slot) {
    const uint32_t k = cc.k;
    const CmpSeg sg = cc.segs[slot];
    const Fr *cs = cc.consts, *rec = cc.rec + (size_t)u * cmp_record_len(k);
    const Fr zero = Fr::zero(), one = Fr::one();
    const uint32_t i = sg.i;
    TraceOut out = trace_at(cc.tc, unit.column, unit.row, sg.off);
    if (sg.type == CMP_LT) {
        const Fr *r = rec + 3 * k * sg.e;
        const Fr a = cc.values[(sg.e ? unit.b_offset : unit.a_offset) + i];
        Fr t = cs[0];
        if (i) {   // gate.add(Constant(p_i), borrow)
            const Fr borrow = r[2 * k + i - 1];
            t = fe_add(cs[i], borrow);
            out.put(cs[i]);
            out.put(borrow);
            out.put(one);
            out.put(t);
        }
        out.put(r[i]);
        out.put(t);
        out.put(one);
        out.put(fe_add(a, cs[k]));
        out.put(cs[k + 1]);
        out.put(one);
        out.put(a);
        return;
    }
    const bool eq = sg.type == CMP_EQ;
    const Fr *r = rec + 6 * k;
    const Fr x = eq ? r[i] : rec[3 * k * sg.e + k + i];
    if (eq) {   // gate.sub(a_i, b_i)
        out.put(x);
        out.put(cc.values[unit.b_offset + i]);
        out.put(one);
        out.put(cc.values[unit.a_offset + i]);
    }
    const bool is_zero = x == zero;
    const Fr z = cmp_select(is_zero, one, zero), inv = cmp_select(is_zero, one, fe_inv(x));   // (fe_inv(0) = 0, not used)
    out.put(z);
    out.put(x);
    out.put(inv);
    out.put(one);
    out.put(zero);
    out.put(x);
    out.put(z);
    out.put(zero);
    if (eq && i) {   // gate.and(eq_i, partial) = mul
        out.put(zero);
        out.put(r[k + i]);
        out.put(r[2 * k + i - 1]);
        out.put(r[2 * k + i]);
    }
}

// ---- what the host derives from the parameters and the mask, once per call (host only)
struct CmpShape : UnitShape {
    FpShape fp;
    uint32_t op, k, pad, width, nsegs, gap_cells, gap_lookups_each;
    CmpSeg segs[CMP_MAX_SEGS];
    uint32_t out_offsets[3];
};
// nullptr when the parameters and the mask are served, else the reason.  cc, consts (CMP_CONSTS entries): optional
inline const char *cmp_prepare(const h2hip_fp_params &pr, uint32_t op, CmpShape &sh, CmpCall *cc, Fr *consts) {
    if (op == 0 || op > 7) return "op is no mask of H2HIP_FP_CMP_REDUCE_A, _REDUCE_B, _EQUAL (1 .. 7)";
    Fr fcs[FP_CONSTS];
    const char *bad = fp_prepare(pr, sh.fp, nullptr, fcs);
    if (bad) return bad;
    const uint32_t n = sh.fp.n, k = sh.fp.k, lb = sh.fp.lb;
    const uint32_t pad = (n + lb - 1) / lb * lb, width = pad + lb, L = width / lb;
    if (width > FP_CAPACITY) return "padded limb_bits + lookup_bits > 253 (is_less_than's bound, F::CAPACITY)";
    sh.op = op;
    sh.k = k;
    sh.pad = pad;
    sh.width = width;
    sh.gap_cells = range_unit_cells(L, 0, 0);
    sh.gap_lookups_each = range_unit_lookups(L, 0);
    sh.nsegs = sh.ngaps = 0;
    sh.out_offsets[0] = sh.out_offsets[1] = sh.out_offsets[2] = 0xFFFFFFFFu;
    uint32_t at = 0, res = 0;
    auto seg = [&](uint8_t type, uint32_t i, uint32_t e, uint32_t cells) {
        sh.segs[sh.nsegs++] = CmpSeg{at, type, (uint8_t)i, (uint8_t)e, 0};
        at += cells;
    };
    for (uint32_t e = 0; e < 2; ++e) {
        if (!(op & (e ? H2HIP_FP_CMP_REDUCE_B : H2HIP_FP_CMP_REDUCE_A))) continue;
        for (uint32_t i = 0; i < k; ++i) {
            seg(CMP_LT, i, e, i ? 11 : 7);
            sh.gaps[sh.ngaps] = h2hip_fp_mul_range{at, sh.gap_cells, width, res + i};
            sh.gap_lookups[sh.ngaps++] = sh.gap_lookups_each;
            at += sh.gap_cells;
            seg(CMP_ISZ, i, e, 8);
        }
        sh.out_offsets[e] = at - 2;   // is_zero returns its seventh cell
        res += k + 1;
    }
    if (op & H2HIP_FP_CMP_EQUAL) {
        for (uint32_t i = 0; i < k; ++i) seg(CMP_EQ, i, 0, i ? 16 : 12);
        sh.out_offsets[2] = at - 1;   // (k >= 2) the product of the last and
    }
    sh.total = at;
    sh.own = at - sh.ngaps * sh.gap_cells;
    sh.num_lookups = sh.ngaps * sh.gap_lookups_each;
    if (consts) {
        for (uint32_t i = 0; i < k; ++i) consts[i] = fcs[i];
        consts[k] = pow2_mont(pad);
        consts[k + 1] = fe_neg(consts[k]);
    }
    if (cc) {
        cc->k = k;
        cc->op = op;
        cc->pad = pad;
        cc->lb = lb;
    }
    return nullptr;
}

}  // namespace h2
