// The cells of EccChip's point selections and of GateChip::num_to_bits (include/h2hip.h states the form), as host and device code:
// ec_select (select::crt twice: one 8-cell GateChip::select per limb and native cell), ec_select_from_bits (bits_to_indicator, then
// select_by_indicator::crt twice) and the bit decomposition of a scalar.  ec_select.hip's first kernel runs sel_solve_unit in one lane per
// unit (the indicator levels, the chains' sums in front of every piece, the selected point -> a per-unit record and the results entries), its
// second sel_place_slot in one lane per (unit, segment); its third runs bits_slot in one lane per (unit, bit).  tools/ec_select_host_fill.cpp
// runs all three in loops on one host thread.  sel_prepare is what the host derives from h2hip_fp_params, the op and the window once per call.
#pragma once
#include "fp_mul.cuh"   // fp_prepare (the limb bases 2^(n i)); range_fill.cuh's limb extraction and trace_place.cuh with it

namespace h2 {

constexpr uint32_t SEL_MAX_WINDOW = 8;
constexpr uint32_t SEL_PIECE = 2;   // entries of a select_by_indicator chain per lane of the place kernel (6 cells, 7 for a chain's first piece)
constexpr uint32_t BITS_MAX = 254;  // F::NUM_BITS

// what one call's lanes share.  consts (canonical Montgomery Fr): fp_prepare's table, of which [k + i] = 2^(n i) is read
struct SelCall : TraceCall {
    uint32_t k, op, w;
    uint32_t m, pieces, chains;   // op 1: 2^w table points; pieces per chain; chains per coordinate (k, and the native's where m <= k)
};
H2_CALL_LEADS(SelCall) H2_OFFSET_IS(SelCall, k, 56) H2_OFFSET_IS(SelCall, op, 60) H2_OFFSET_IS(SelCall, w, 64) H2_OFFSET_IS(SelCall, m, 68)
H2_OFFSET_IS(SelCall, pieces, 72) H2_OFFSET_IS(SelCall, chains, 76)
static_assert(sizeof(SelCall) == 80, "SelCall grew or shrank");

// cells of a unit.  op 0: 8 per cell of the point.  op 1: bits_to_indicator, then per coordinate k chains and the native
H2_HD uint32_t sel_indicator_cells(uint32_t w) { return (8u << w) - 12; }
H2_HD uint32_t sel_chain_cells(uint32_t m) { return 3 * m + 1; }
H2_HD uint32_t sel_coord_cells(uint32_t k, uint32_t m) { return k * sel_chain_cells(m) + (m > k ? 3 * k - 2 : sel_chain_cells(m)); }
H2_HD uint32_t sel_unit_cells(uint32_t k, uint32_t op, uint32_t w) {
    return op == H2HIP_EC_SELECT ? 16 * (k + 1) : sel_indicator_cells(w) + 2 * sel_coord_cells(k, 1u << w);
}
H2_HD uint32_t sel_result_len(uint32_t k) { return 2 * (k + 1); }
// the record of a unit.  op 0: the selected point.  op 1: [the indicator levels as a heap: entry t's children are 2 t + 2 and 2 t + 3, the
// last level (entry v the indicator of v) from m - 2][per coordinate and chain, the sum in front of each piece][the selected point]
H2_HD uint32_t sel_record_len(const SelCall &sc) {
    return sc.op == H2HIP_EC_SELECT ? sel_result_len(sc.k) : 2 * sc.m - 2 + 2 * sc.chains * sc.pieces + sel_result_len(sc.k);
}
// lanes of the place kernel per unit.  op 1: the indicator's first four cells, its 2^w - 2 nodes, the pieces, evaluate_native where m > k
H2_HD uint32_t sel_coord_slots(const SelCall &sc) { return sc.chains * sc.pieces + (sc.m > sc.k ? 1 : 0); }
H2_HD uint32_t sel_unit_slots(const SelCall &sc) { return sc.op == H2HIP_EC_SELECT ? sel_result_len(sc.k) : sc.m - 1 + 2 * sel_coord_slots(sc); }

// a cell read word by word (a struct copy from memory that is only stored again stays a memcpy through a private slot, and alloca promotion
// moves that slot to LDS)
H2_HD Fr sel_load(const Fr &x) {
    Fr r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.l[j] = x.l[j];
    return r;
}

// ---- one unit
H2_HD void sel_solve_unit(const SelCall &sc, const h2hip_ec_select &unit, uint32_t u) {
    const uint32_t k = sc.k, pt = sel_result_len(k);
    Fr *rec = sc.rec + (size_t)u * sel_record_len(sc);
    Fr *res = sc.results ? sc.results + (size_t)u * pt : nullptr;
    if (sc.op == H2HIP_EC_SELECT) {   // out = (a - b) sel + b over the cell values
        const Fr *a = sc.values + unit.p_offset, *b = sc.values + unit.q_offset;
        const Fr sel = sc.values[unit.sel_offset];
        for (uint32_t j = 0; j < pt; ++j) {
            const Fr y = b[j], out = fe_add(fe_mul(fe_sub(a[j], y), sel), y);
            rec[j] = out;
            if (res) res[j] = out;
        }
        return;
    }
    const uint32_t w = sc.w, m = sc.m;
    const Fr *bits = sc.values + unit.sel_offset, *table = sc.values + unit.p_offset;
    // bits_to_indicator: level 0 = (1 - b_{w-1}, b_{w-1}); entry t of level idx - 1 gives ((1 - bit) ind, bit ind) with bit = b_{w-1-idx}
    const Fr top = bits[w - 1];
    rec[0] = fe_sub(Fr::one(), top);
    rec[1] = top;
    for (uint32_t t = 0; t + 2 < m; ++t) {
        const uint32_t idx = 31u - (uint32_t)__builtin_clz(t + 2);
        const Fr ind = rec[t], prod = fe_mul(ind, bits[w - 1 - idx]);
        rec[2 * t + 2] = fe_sub(ind, prod);
        rec[2 * t + 3] = prod;
    }
    // select_by_indicator in its arithmetic form: s_i = s_{i-1} + a_i ind_i
    const Fr *ind = rec + (m - 2);
    Fr *pre = rec + (2 * m - 2), *out = pre + 2 * sc.chains * sc.pieces;
    for (uint32_t c = 0; c < 2; ++c) {
        for (uint32_t j = 0; j < sc.chains; ++j) {
            const Fr *a = table + c * (k + 1) + j;
            Fr s = Fr::zero();
            for (uint32_t i = 0; i < m; ++i) {
                if (i % SEL_PIECE == 0) pre[(c * sc.chains + j) * sc.pieces + i / SEL_PIECE] = s;
                s = fe_add(s, fe_mul(a[(size_t)i * pt], ind[i]));
            }
            out[c * (k + 1) + j] = s;
        }
        if (m > k) {   // evaluate_native over the k output limbs
            Fr nat = out[c * (k + 1)];
            for (uint32_t j = 1; j < k; ++j) nat = fe_add(nat, fe_mul(out[c * (k + 1) + j], sc.consts[k + j]));
            out[c * (k + 1) + k] = nat;
        }
    }
    if (res)
        for (uint32_t j = 0; j < pt; ++j) res[j] = out[j];
}

// ---- one segment of one unit
H2_HD void sel_place_slot(const SelCall &sc, const h2hip_ec_select &unit, uint32_t u, uint32_t slot) {
    const uint32_t k = sc.k;
    const Fr *rec = sc.rec + (size_t)u * sel_record_len(sc);
    const Fr zero = Fr::zero(), one = Fr::one();
    if (sc.op == H2HIP_EC_SELECT) {   // a - b, 1, b, a, b, sel, a - b, out
        const Fr a = sc.values[unit.p_offset + slot], b = sc.values[unit.q_offset + slot], d = fe_sub(a, b);
        TraceOut out = trace_at(sc.tc, unit.column, unit.row, 8 * slot);
        out.put(d);
        out.put(one);
        out.put(b);
        out.put(a);
        out.put(b);
        out.put(sc.values[unit.sel_offset]);
        out.put(d);
        out.put(rec[slot]);
        return;
    }
    const uint32_t w = sc.w, m = sc.m;
    const Fr *bits = sc.values + unit.sel_offset;
    if (slot == 0) {   // 1 - b_{w-1}, b_{w-1}, 1, 1
        TraceOut out = trace_at(sc.tc, unit.column, unit.row);
        out.put(rec[0]);
        out.put(rec[1]);
        out.put(one);
        out.put(one);
        return;
    }
    if (slot < m - 1) {   // node t: (1 - bit) ind, ind, bit, ind; 0, ind, bit, ind bit
        const uint32_t t = slot - 1, idx = 31u - (uint32_t)__builtin_clz(t + 2);
        const Fr ind = sel_load(rec[t]), bit = sel_load(bits[w - 1 - idx]);
        TraceOut out = trace_at(sc.tc, unit.column, unit.row, 4 + 8 * t);
        out.put(rec[2 * t + 2]);
        out.put(ind);
        out.put(bit);
        out.put(ind);
        out.put(zero);
        out.put(ind);
        out.put(bit);
        out.put(rec[2 * t + 3]);
        return;
    }
    const uint32_t per = sel_coord_slots(sc), r = slot - (m - 1), c = r / per, r2 = r - c * per, pt = sel_result_len(k);
    const uint32_t base = sel_indicator_cells(w) + c * sel_coord_cells(k, m);
    const Fr *pre = rec + (2 * m - 2), *res = pre + 2 * sc.chains * sc.pieces + c * (k + 1);
    if (r2 == sc.chains * sc.pieces) {   // (m > k) evaluate_native: o_0, o_1, 2^n, s_1, ...
        TraceOut out = trace_at(sc.tc, unit.column, unit.row, base + k * sel_chain_cells(m));
        Fr acc = res[0];
        out.put(acc);
        for (uint32_t j = 1; j < k; ++j) {
            const Fr x = res[j], y = sc.consts[k + j];
            acc = fe_add(acc, fe_mul(x, y));
            out.put(x);
            out.put(y);
            out.put(acc);
        }
        return;
    }
    // a piece of a chain: (0,) a_i, ind_i, s_i for SEL_PIECE entries from i0
    const uint32_t j = r2 / sc.pieces, q = r2 - j * sc.pieces, i0 = q * SEL_PIECE, i1 = i0 + SEL_PIECE < m ? i0 + SEL_PIECE : m;
    const Fr *a = sc.values + unit.p_offset + c * (k + 1) + j, *ind = rec + (m - 2);
    TraceOut out = trace_at(sc.tc, unit.column, unit.row, base + j * sel_chain_cells(m) + (q ? 1 + 3 * i0 : 0));
    Fr s = pre[(c * sc.chains + j) * sc.pieces + q];
    if (!q) out.put(zero);
    for (uint32_t i = i0; i < i1; ++i) {
        const Fr x = a[(size_t)i * pt], y = ind[i];
        s = fe_add(s, fe_mul(x, y));
        out.put(x);
        out.put(y);
        out.put(s);
    }
}

// ---- GateChip::num_to_bits: bit i of one unit.  l_0 | l_i, 2^i, s_i from cell 1 + 3 (i - 1) | then assert_bit per bit: 0, l_i, l_i, l_i
struct BitsCall {
    TraceCols tc;
    const Fr *values;
    Fr *results;
    uint32_t nb;
};
H2_HD uint32_t bits_unit_cells(uint32_t nb) { return 7 * nb - 2; }
// 2^i in Montgomery form, i <= 253 (the word is chosen by comparisons: a dynamic index into r.l would put the element into scratch)
H2_HD Fr bits_pow2(uint32_t i) {
    Fr r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.l[j] = (i >> 5) == (uint32_t)j ? 1u << (i & 31) : 0u;
    return fe_to_mont(r);
}
H2_HD void bits_slot(const BitsCall &bc, const h2hip_bits_unit &unit, uint32_t u, uint32_t i) {
    const uint32_t nb = bc.nb;
    const Fr c = fe_from_mont(bc.values[unit.a_offset]);
    const Fr l = range_from_u64(range_bits_at(c, i, 1));
    TraceOut out = trace_at(bc.tc, unit.column, unit.row, i ? 1 + 3 * (i - 1) : 0);
    out.put(l);
    if (i) {
        out.put(bits_pow2(i));
        out.put(fe_to_mont(range_low_bits(c, i + 1)));   // (i + 1 = 254: c itself, below r)
    }
    out = trace_at(bc.tc, unit.column, unit.row, 3 * nb - 2 + 4 * i);
    out.put(Fr::zero());
    out.put(l);
    out.put(l);
    out.put(l);
    if (bc.results) bc.results[(size_t)u * nb + i] = l;
}

// ---- what the host derives from the parameters, the op and the window, once per call (host only)
struct SelShape {
    uint32_t k, total;
    uint32_t out_offsets[2 * (FP_MAX_K + 1)];
};
// nullptr when the call is served, else the reason.  sc, consts (FP_CONSTS entries): optional
inline const char *sel_prepare(const h2hip_fp_params &pr, uint32_t op, uint32_t window_bits, SelShape &sh, SelCall *sc, Fr *consts) {
    if (op != H2HIP_EC_SELECT && op != H2HIP_EC_SELECT_FROM_BITS) return "unknown op";
    if (op == H2HIP_EC_SELECT && window_bits) return "window_bits must be 0 for H2HIP_EC_SELECT";
    if (op == H2HIP_EC_SELECT_FROM_BITS && (window_bits < 1 || window_bits > SEL_MAX_WINDOW)) return "window_bits outside 1 .. 8";
    if (pr.num_limbs < 3) return "num_limbs < 3 (a point of the curve operations has 3 or 4 limbs)";   // (fp_prepare refuses k = 2 for other reasons)
    FpShape fp;
    Fr fcs[FP_CONSTS];
    const char *bad = fp_prepare(pr, fp, nullptr, fcs);
    if (bad) return bad;
    const uint32_t k = fp.k, w = window_bits, m = 1u << w;
    sh.k = k;
    sh.total = sel_unit_cells(k, op, w);
    for (uint32_t c = 0; c < 2; ++c)
        for (uint32_t j = 0; j <= k; ++j) {
            uint32_t &off = sh.out_offsets[c * (k + 1) + j];
            if (op == H2HIP_EC_SELECT)
                off = 8 * (c * (k + 1) + j) + 7;
            else {
                const uint32_t base = sel_indicator_cells(w) + c * sel_coord_cells(k, m);
                off = j == k && m > k ? base + k * sel_chain_cells(m) + 3 * k - 3 : base + j * sel_chain_cells(m) + 3 * m;
            }
        }
    if (consts)
        for (uint32_t i = 0; i < FP_CONSTS; ++i) consts[i] = i < 2 * k + 4 ? fcs[i] : Fr::zero();
    if (sc) {
        sc->k = k;
        sc->op = op;
        sc->w = w;
        sc->m = m;
        sc->pieces = (m + SEL_PIECE - 1) / SEL_PIECE;
        sc->chains = m > k ? k : k + 1;
    }
    return nullptr;
}

}  // namespace h2
