// The cells of one range check (include/h2hip.h states the form), slot by slot, as host and device code: range_fill.hip's kernel runs
// range_slot in one lane per (unit, slot), tools/range_host_fill.cpp in a loop on one host thread.
#pragma once
#include "internal.h"
#include "trace_place.cuh"   // TraceOut: assign_witnesses' placement of a run of cells

namespace h2 {

constexpr uint32_t RANGE_PREFIX = 7;       // the cells of check_less_than / is_less_than in front of the range check
constexpr uint32_t RANGE_CAPACITY = 253;   // F::CAPACITY: 2^253 < r

// what one call's lanes share.  pows: [2^(i lb), i < L][2^(lb - rem)][2^shift_bits][-2^shift_bits], canonical Montgomery Fr
struct RangeCall {
    TraceCols tc;
    Fr *const *lk_cols;
    const Fr *values, *pows;
    uint32_t num_lk_cols, L, lb, rem, prefix;   // prefix: RANGE_PREFIX with H2HIP_RANGE_LESS_THAN, else 0
};

// cells of one unit: the prefix, l_0 l_1 2^lb s_1 ... (3 L - 2, only for L >= 2), the tail gate (4, only for rem >= 1)
H2_HD uint32_t range_decomp_cells(uint32_t L) { return L >= 2 ? 3 * L - 2 : 0; }
H2_HD uint32_t range_unit_cells(uint32_t L, uint32_t rem, uint32_t prefix) { return prefix + range_decomp_cells(L) + (rem ? 4 : 0); }
H2_HD uint32_t range_unit_lookups(uint32_t L, uint32_t rem) { return L + (rem > 1 ? 1 : 0); }
H2_HD uint32_t range_unit_slots(uint32_t L, uint32_t rem) { return L + (rem ? 1 : 0); }

// bits [lo, lo + nb) of the canonical integer c, nb <= 63, lo + nb <= 256: the 64-bit digit and its neighbour are chosen by comparisons
// over the four digits (a dynamic index into c.l would put the element into scratch)
H2_HD uint64_t range_bits_at(const Fr &c, uint32_t lo, uint32_t nb) {
    const uint64_t d0 = c.l[0] | (uint64_t)c.l[1] << 32, d1 = c.l[2] | (uint64_t)c.l[3] << 32, d2 = c.l[4] | (uint64_t)c.l[5] << 32,
                   d3 = c.l[6] | (uint64_t)c.l[7] << 32;
    const uint32_t q = lo >> 6, sh = lo & 63;
    const uint64_t a = q == 0 ? d0 : q == 1 ? d1 : q == 2 ? d2 : d3, b = q == 0 ? d1 : q == 1 ? d2 : q == 2 ? d3 : 0;
    const uint64_t v = sh ? (a >> sh) | (b << (64 - sh)) : a;
    return v & (((uint64_t)1 << nb) - 1);
}
// the low nb bits of c, nb <= 253 (below r: already canonical)
H2_HD Fr range_low_bits(const Fr &c, uint32_t nb) {
    Fr r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t base = 32u * j;
        const uint32_t mask = nb >= base + 32 ? 0xFFFFFFFFu : nb <= base ? 0u : (1u << (nb - base)) - 1u;
        r.l[j] = c.l[j] & mask;
    }
    return r;
}
H2_HD Fr range_from_u64(uint64_t x) {
    Fr r = Fr::zero();
    r.l[0] = (uint32_t)x;
    r.l[1] = (uint32_t)(x >> 32);
    return fe_to_mont(r);
}

// lookup cell j of the unit: queue position p = lookup_slot + j lies in column p mod num_lk_cols at row p / num_lk_cols (assign_raw, lookups.rs:129-156)
H2_HD void range_lookup_put(const RangeCall &rc, const h2hip_range_check &unit, uint32_t j, const Fr &v) {
    const uint64_t p = unit.lookup_slot + j;
    rc.lk_cols[p % rc.num_lk_cols][p / rc.num_lk_cols] = v;
}

// slot `slot` of one unit: 0 = the prefix, l_0 and its lookup copy (v's when L = 1); 1 <= i < L = l_i, 2^(i lb), s_i and l_i's lookup copy;
// L = the tail gate on the last limb (on v itself when L = 1) and, for rem > 1, the product's lookup copy
H2_HD void range_slot(const RangeCall &rc, const h2hip_range_check &unit, uint32_t slot) {
    const uint32_t L = rc.L, lb = rc.lb;
    Fr v = rc.values[unit.a_offset], a = v, b = v, shifted = v;
    if (rc.prefix) {   // | a + 2^shift - b | b | 1 | a + 2^shift | -2^shift | 1 | a |: v is the first cell
        b = rc.values[unit.b_offset];
        shifted = fe_add(a, rc.pows[L + 1]);
        v = fe_sub(shifted, b);
    }
    if (slot == 0) {
        Fr l0 = v;
        if (L >= 2) l0 = range_from_u64(range_bits_at(fe_from_mont(v), 0, lb));
        if (rc.prefix || L >= 2) {
            TraceOut o = trace_at(rc.tc, unit.column, unit.row);
            if (rc.prefix) {
                const Fr one = Fr::one();
                o.put(v);
                o.put(b);
                o.put(one);
                o.put(shifted);
                o.put(rc.pows[L + 2]);
                o.put(one);
                o.put(a);
            }
            if (L >= 2) o.put(l0);
        }
        range_lookup_put(rc, unit, 0, l0);
    } else if (slot < L) {
        const Fr c = fe_from_mont(v);
        const Fr li = range_from_u64(range_bits_at(c, slot * lb, lb)), si = fe_to_mont(range_low_bits(c, (slot + 1) * lb));
        TraceOut o = trace_at(rc.tc, unit.column, unit.row, rc.prefix + 1 + 3 * (slot - 1));
        o.put(li);
        o.put(rc.pows[slot]);
        o.put(si);
        range_lookup_put(rc, unit, slot, li);
    } else {   // rem >= 1
        const Fr x = L >= 2 ? range_from_u64(range_bits_at(fe_from_mont(v), (L - 1) * lb, lb)) : v;
        TraceOut o = trace_at(rc.tc, unit.column, unit.row, rc.prefix + range_decomp_cells(L));
        o.put(Fr::zero());
        o.put(x);
        if (rc.rem == 1) {   // assert_bit: | 0 | x | x | x |
            o.put(x);
            o.put(x);
        } else {             // mul: | 0 | x | 2^(lb - rem) | x 2^(lb - rem) |
            const Fr m = rc.pows[L], prod = fe_mul(x, m);
            o.put(m);
            o.put(prod);
            range_lookup_put(rc, unit, L, prod);
        }
    }
}

// ---- what the host derives from the parameters, once per call (host only)
inline Fr pow2_mont(uint32_t e) {   // e <= RANGE_CAPACITY
    Fr r = Fr::zero();
    r.l[e >> 5] = 1u << (e & 31);
    return fe_to_mont(r);
}
// nullptr when the parameters are served, else the reason.  rc: L, lb, rem, prefix; pows (optional): the table, and rc.pows points at it (a
// device call uploads it and points rc.pows at the copy)
inline const char *range_prepare(uint32_t range_bits, uint32_t lookup_bits, uint32_t shift_bits, uint32_t flags, RangeCall &rc, std::vector<Fr> *pows) {
    if (flags & ~(uint32_t)H2HIP_RANGE_LESS_THAN) return "unknown flags";
    if (range_bits == 0) return "range_bits == 0 (a constant check, not a range check)";
    if (lookup_bits < 1 || lookup_bits > 63) return "lookup_bits outside 1 .. 63";
    if (((uint64_t)range_bits + lookup_bits - 1) / lookup_bits * lookup_bits > RANGE_CAPACITY) return "the limbs take more than 253 bits (F::CAPACITY)";
    if ((flags & H2HIP_RANGE_LESS_THAN) && shift_bits > RANGE_CAPACITY) return "shift_bits above 253 (F::CAPACITY)";
    const uint32_t L = (range_bits + lookup_bits - 1) / lookup_bits, rem = range_bits % lookup_bits;
    rc.L = L;
    rc.lb = lookup_bits;
    rc.rem = rem;
    rc.prefix = (flags & H2HIP_RANGE_LESS_THAN) ? RANGE_PREFIX : 0;
    if (pows) {
        pows->resize(L + 3);
        for (uint32_t i = 0; i < L; ++i) (*pows)[i] = pow2_mont(i * lookup_bits);
        (*pows)[L] = pow2_mont(rem ? lookup_bits - rem : 0);
        (*pows)[L + 1] = pow2_mont(rc.prefix ? shift_bits : 0);
        (*pows)[L + 2] = fe_neg((*pows)[L + 1]);
        rc.pows = pows->data();
    }
    return nullptr;
}

}  // namespace h2
