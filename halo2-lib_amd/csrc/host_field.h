// Small host-side helpers over Fr / Fq shared by the prover (plonk_internal.h) and the verifier (verifier.hip): canonical bytes, ordering,
// Fr::from_uniform_bytes.
#pragma once
#include "internal.h"

namespace h2 {

static inline Fr fr_from_canonical_u64x4(const uint64_t v[4]) {
    Fr a;
    memcpy(a.l, v, 32);
    return fe_to_mont(a);
}
static inline Fr fr_from_u64(uint64_t v) {
    uint64_t w[4] = {v, 0, 0, 0};
    return fr_from_canonical_u64x4(w);
}
// canonical little-endian bytes (to_repr)
static inline void fr_repr(const Fr &a, uint8_t out[32]) {
    Fr c = fe_from_mont(a);
    memcpy(out, c.l, 32);
}
static inline void fq_repr(const Fq &a, uint8_t out[32]) {
    Fq c = fe_from_mont(a);
    memcpy(out, c.l, 32);
}
// numeric order of the canonical values (Ord for Fr compares to_repr from the most significant byte)
static inline int fr_cmp(const Fr &a, const Fr &b) {
    Fr x = fe_from_mont(a), y = fe_from_mont(b);
    for (int i = 7; i >= 0; --i)
        if (x.l[i] != y.l[i]) return x.l[i] < y.l[i] ? -1 : 1;
    return 0;
}
// Fr::from_uniform_bytes: 512-bit little-endian integer mod r = d0 + d1 * 2^256
static inline Fr fr_from_uniform_bytes(const uint8_t b[64]) {
    Fr d0, d1;
    memcpy(d0.l, b, 32);
    memcpy(d1.l, b + 32, 32);
    const Fr r2 = Fr::r2(), r3 = fe_mul(r2, r2);
    return fe_add(fe_mul(d0, r2), fe_mul(d1, r3));
}

}  // namespace h2
