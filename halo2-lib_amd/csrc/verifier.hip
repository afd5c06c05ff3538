// verify_proof for halo2-base circuits — the check the reference runs after every proof it creates
// (halo2-base/src/utils/testing.rs:64-88: verify_proof::<KZGCommitmentScheme<Bn256>, VerifierSHPLONK<_>, Challenge255<_>, Blake2bRead<_, _, _>,
// SingleStrategy<_>>).  Host code (the reference verifies on the CPU as well): Blake2b transcript replay, the quotient identity rebuilt from the
// openings, SHPLONK's folded opening and ONE pairing check e(h2, s*g2) == e(right, g2).  [UPSTREAM-RECALL for the protocol order, like
// plonk_prove.hip.]  The pairing is the plain ate pairing f_{t-1,Q}(P)^((q^12-1)/r) over the tower Fq2 = Fq[u]/(u^2+1), Fq6 = Fq2[v]/(v^3 - (9+u)),
// Fq12 = Fq6[w]/(w^2 - v) — any non-degenerate pairing decides e(L, sQ) == e(R, Q), which is all a KZG verifier needs.
#include <mutex>
#include <algorithm>
#include <map>
#include <vector>

#include "blake2b.h"
#include "shplonk_sets.h"
#include "transcript.h"
#include "verifier_internal.h"

namespace h2 {
namespace verifier {

// ---------------------------------------------------------------------------------------------- tower arithmetic (host)
struct F2 {
    Fq c0, c1;
};
static F2 f2_zero() { return {Fq::zero(), Fq::zero()}; }
static F2 f2_one() { return {Fq::one(), Fq::zero()}; }
static bool f2_eq(const F2 &a, const F2 &b) { return a.c0 == b.c0 && a.c1 == b.c1; }
static bool f2_is_zero(const F2 &a) { return a.c0.is_zero() && a.c1.is_zero(); }
static F2 f2_add(const F2 &a, const F2 &b) { return {fe_add(a.c0, b.c0), fe_add(a.c1, b.c1)}; }
static F2 f2_sub(const F2 &a, const F2 &b) { return {fe_sub(a.c0, b.c0), fe_sub(a.c1, b.c1)}; }
static F2 f2_neg(const F2 &a) { return {fe_neg(a.c0), fe_neg(a.c1)}; }
static F2 f2_mul(const F2 &a, const F2 &b) {
    Fq t0 = fe_mul(a.c0, b.c0), t1 = fe_mul(a.c1, b.c1);
    return {fe_sub(t0, t1), fe_sub(fe_sub(fe_mul(fe_add(a.c0, a.c1), fe_add(b.c0, b.c1)), t0), t1)};
}
static F2 f2_sqr(const F2 &a) { return {fe_mul(fe_add(a.c0, a.c1), fe_sub(a.c0, a.c1)), fe_dbl(fe_mul(a.c0, a.c1))}; }
static F2 f2_scal(const F2 &a, const Fq &k) { return {fe_mul(a.c0, k), fe_mul(a.c1, k)}; }
static F2 f2_inv(const F2 &a) {
    Fq d = fe_inv(fe_add(fe_sqr(a.c0), fe_sqr(a.c1)));
    return {fe_mul(a.c0, d), fe_neg(fe_mul(a.c1, d))};
}
static Fq fq_small(uint32_t v) {
    Fq a = Fq::zero();
    a.l[0] = v;
    return fe_to_mont(a);
}
static F2 f2_mul_xi(const F2 &a) {   // * (9 + u)
    const Fq nine = fq_small(9);
    return {fe_sub(fe_mul(a.c0, nine), a.c1), fe_add(a.c0, fe_mul(a.c1, nine))};
}
struct F6 {
    F2 c0, c1, c2;
};
static F6 f6_zero() { return {f2_zero(), f2_zero(), f2_zero()}; }
static F6 f6_one() { return {f2_one(), f2_zero(), f2_zero()}; }
static F6 f6_add(const F6 &a, const F6 &b) { return {f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
static F6 f6_sub(const F6 &a, const F6 &b) { return {f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
static F6 f6_neg(const F6 &a) { return {f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
static F6 f6_mul(const F6 &a, const F6 &b) {
    F2 t0 = f2_mul(a.c0, b.c0), t1 = f2_mul(a.c1, b.c1), t2 = f2_mul(a.c2, b.c2);
    F6 r;
    r.c0 = f2_add(t0, f2_mul_xi(f2_sub(f2_sub(f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), t1), t2)));
    r.c1 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), t0), t1), f2_mul_xi(t2));
    r.c2 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), t0), t2), t1);
    return r;
}
static F6 f6_mul_v(const F6 &a) { return {f2_mul_xi(a.c2), a.c0, a.c1}; }
static F6 f6_inv(const F6 &a) {
    F2 c0 = f2_sub(f2_sqr(a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
    F2 c1 = f2_sub(f2_mul_xi(f2_sqr(a.c2)), f2_mul(a.c0, a.c1));
    F2 c2 = f2_sub(f2_sqr(a.c1), f2_mul(a.c0, a.c2));
    F2 t = f2_inv(f2_add(f2_mul(a.c0, c0), f2_mul_xi(f2_add(f2_mul(a.c2, c1), f2_mul(a.c1, c2)))));
    return {f2_mul(c0, t), f2_mul(c1, t), f2_mul(c2, t)};
}
struct F12 {
    F6 c0, c1;
};
static F12 f12_one() { return {f6_one(), f6_zero()}; }
static F12 f12_mul(const F12 &a, const F12 &b) {
    F6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    return {f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1)};
}
static F12 f12_inv(const F12 &a) {
    F6 t = f6_inv(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return {f6_mul(a.c0, t), f6_neg(f6_mul(a.c1, t))};
}
static bool f12_is_one(const F12 &a) {
    const F12 o = f12_one();
    return f2_eq(a.c0.c0, o.c0.c0) && f2_is_zero(a.c0.c1) && f2_is_zero(a.c0.c2) && f2_is_zero(a.c1.c0) && f2_is_zero(a.c1.c1) && f2_is_zero(a.c1.c2);
}

// ---------------------------------------------------------------------------------------------- G2 (affine over Fq2) and the ate pairing
struct G2A {
    F2 x, y;
    bool inf;
};
static G2A g2_add(const G2A &A, const G2A &B) {
    if (A.inf) return B;
    if (B.inf) return A;
    F2 lam;
    if (f2_eq(A.x, B.x)) {
        if (f2_is_zero(f2_add(A.y, B.y))) return {f2_zero(), f2_zero(), true};
        F2 x2 = f2_sqr(A.x);
        lam = f2_mul(f2_add(f2_add(x2, x2), x2), f2_inv(f2_add(A.y, A.y)));
    } else {
        lam = f2_mul(f2_sub(B.y, A.y), f2_inv(f2_sub(B.x, A.x)));
    }
    F2 x3 = f2_sub(f2_sub(f2_sqr(lam), A.x), B.x);
    return {x3, f2_sub(f2_mul(lam, f2_sub(A.x, x3)), A.y), false};
}
static bool g2_on_curve(const G2A &Q) {
    if (Q.inf) return true;
    F2 b = f2_mul({fq_small(3), Fq::zero()}, f2_inv({fq_small(9), Fq::one()}));   // 3 / (9 + u): the D-twist's constant
    return f2_eq(f2_sqr(Q.y), f2_add(f2_mul(f2_sqr(Q.x), Q.x), b));
}
// Q in the order-r subgroup G2 of the twist?  The twist's group has a large cofactor (2q - r), so "on the twist" is not enough: EIP-197
// rejects such points, and the pairing of one is not what the protocol's equations mean.  [r]Q by double-and-add in JACOBIAN
// coordinates over F_q2 (a = 0: dbl-2009-l, madd-2007-bl) — no field inversion anywhere (the affine ladder paid ~380 F_q2
// inversions, tens of milliseconds, per G2 input and call) — and the points a verifier passes again and again (the SRS's g2 and s_g2) are
// remembered: a point that passed once is recognised by its bytes.
struct G2J {
    F2 x, y, z;   // z = 0: the identity
};
static G2J g2j_dbl(const G2J &P) {
    if (f2_is_zero(P.z)) return P;
    const F2 A = f2_sqr(P.x), B = f2_sqr(P.y), C = f2_sqr(B);
    F2 D = f2_sub(f2_sub(f2_sqr(f2_add(P.x, B)), A), C);
    D = f2_add(D, D);
    const F2 E = f2_add(f2_add(A, A), A), F = f2_sqr(E);
    G2J R;
    R.x = f2_sub(F, f2_add(D, D));
    F2 C8 = f2_add(C, C);
    C8 = f2_add(C8, C8);
    C8 = f2_add(C8, C8);
    R.y = f2_sub(f2_mul(E, f2_sub(D, R.x)), C8);
    const F2 yz = f2_mul(P.y, P.z);
    R.z = f2_add(yz, yz);
    return R;
}
static G2J g2j_madd(const G2J &P, const G2A &Q) {   // Q affine, not the identity
    if (f2_is_zero(P.z)) return {Q.x, Q.y, f2_one()};
    const F2 Z1Z1 = f2_sqr(P.z), U2 = f2_mul(Q.x, Z1Z1), S2 = f2_mul(f2_mul(Q.y, P.z), Z1Z1);
    const F2 H = f2_sub(U2, P.x);
    F2 r = f2_sub(S2, P.y);
    if (f2_is_zero(H)) return f2_is_zero(r) ? g2j_dbl(P) : G2J{f2_one(), f2_one(), f2_zero()};
    r = f2_add(r, r);
    const F2 HH = f2_sqr(H);
    F2 I = f2_add(HH, HH);
    I = f2_add(I, I);
    const F2 J = f2_mul(H, I), V = f2_mul(P.x, I);
    G2J R;
    R.x = f2_sub(f2_sub(f2_sqr(r), J), f2_add(V, V));
    const F2 YJ = f2_mul(P.y, J);
    R.y = f2_sub(f2_mul(r, f2_sub(V, R.x)), f2_add(YJ, YJ));
    R.z = f2_sub(f2_sub(f2_sqr(f2_add(P.z, H)), Z1Z1), HH);
    return R;
}
static bool g2_in_subgroup(const G2A &Q) {
    if (Q.inf) return true;
    static std::mutex mu;
    static G2A seen[8];
    static int seen_n = 0, seen_next = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (int i = 0; i < seen_n; ++i)
            if (f2_eq(seen[i].x, Q.x) && f2_eq(seen[i].y, Q.y)) return true;
    }
    G2J acc = {f2_one(), f2_one(), f2_zero()};
    for (int bit = 253; bit >= 0; --bit) {
        acc = g2j_dbl(acc);
        if ((FrP::m(bit >> 5) >> (bit & 31)) & 1u) acc = g2j_madd(acc, Q);
    }
    const bool ok = f2_is_zero(acc.z);
    if (ok) {
        std::lock_guard<std::mutex> lk(mu);
        seen[seen_next] = Q;
        seen_next = (seen_next + 1) % 8;
        if (seen_n < 8) ++seen_n;
    }
    return ok;
}
// line through T with twist-slope lam, evaluated at the G1 point (xP, yP) after untwisting: yP - lam*xP*w + (lam*xT - yT)*w^3
static F12 line_eval(const G2A &T, const F2 &lam, const Fq &xP, const Fq &yP) {
    F12 l;
    l.c0 = {{yP, Fq::zero()}, f2_zero(), f2_zero()};
    l.c1 = {f2_neg(f2_scal(lam, xP)), f2_sub(f2_mul(lam, T.x), T.y), f2_zero()};
    return l;
}
static const uint64_t ATE_LOOP[2] = {0xf83e9682e87cfd46ULL, 0x6f4d8248eeb859fbULL};   // t - 1 = 6x^2, x = 4965661367192848881
static F12 miller_loop(const G1Affine &P, const G2A &Q) {
    if (P.is_identity() || Q.inf) return f12_one();
    F12 f = f12_one();
    G2A T = Q;
    for (int bit = 125; bit >= 0; --bit) {   // 127 bits: the top one starts T = Q
        F2 x2 = f2_sqr(T.x);
        F2 lam = f2_mul(f2_add(f2_add(x2, x2), x2), f2_inv(f2_add(T.y, T.y)));
        f = f12_mul(f12_mul(f, f), line_eval(T, lam, P.x, P.y));
        T = g2_add(T, T);
        if ((ATE_LOOP[bit >> 6] >> (bit & 63)) & 1) {
            if (f2_eq(T.x, Q.x)) {   // T = -Q: only at the very end of a loop over a multiple of the order
                T = g2_add(T, Q);
                continue;
            }
            lam = f2_mul(f2_sub(Q.y, T.y), f2_inv(f2_sub(Q.x, T.x)));
            f = f12_mul(f, line_eval(T, lam, P.x, P.y));
            T = g2_add(T, Q);
        }
    }
    return f;
}
// (q^6 + 1) / r, little-endian 64-bit words: the part of the final exponent left after f -> conj(f) / f  (= f^(q^6 - 1))
static const uint64_t HARD_EXP[20] = {
    0x5250a54036e3f812ULL, 0xa5635f1596789051ULL, 0xd1138bf54d5bd1d4ULL, 0xa8ce2533be36c7a2ULL,
    0x94f69f6b84e09bf6ULL, 0x42ad1f5e50ef3644ULL, 0x0fcc420e48c3454cULL, 0x758e4408ecc9952cULL,
    0xc901bf1887c6042cULL, 0xa733cd65b14bb3b5ULL, 0xdf6d76bdcf51b0d8ULL, 0xca64c0fd82eb59e1ULL,
    0x1d2e5726e39276a1ULL, 0xc2d1ea74a391cae9ULL, 0x07409206c82d647eULL, 0x051c6d1aa5afdd17ULL,
    0xb37f601919667af5ULL, 0x150e578c5084015bULL, 0xfbdea556c23998e4ULL, 0x000fd14cc52f5b83ULL};
static F12 final_exponentiation(const F12 &f) {
    F12 conj = {f.c0, f6_neg(f.c1)};
    F12 g = f12_mul(conj, f12_inv(f));
    F12 r = f12_one();
    bool started = false;
    for (int bit = 20 * 64 - 1; bit >= 0; --bit) {
        if (started) r = f12_mul(r, r);
        if ((HARD_EXP[bit >> 6] >> (bit & 63)) & 1) {
            r = started ? f12_mul(r, g) : g;
            started = true;
        }
    }
    return r;
}

// ---------------------------------------------------------------------------------------------- G1 on the host
static XYZZ g1_scalar_mul(const G1Affine &p, const Fr &k_mont) {
    XYZZ acc = XYZZ::identity();
    if (p.is_identity()) return acc;
    const Fr k = fe_from_mont(k_mont);
    bool started = false;
    for (int bit = 255; bit >= 0; --bit) {
        if (started) acc = xyzz_double(acc);
        if ((k.l[bit >> 5] >> (bit & 31)) & 1u) {
            xyzz_add_affine(acc, p.x, p.y);
            started = true;
        }
    }
    return acc;
}
static bool g1_on_curve_host(const G1Affine &p) {   // y^2 == x^3 + 3
    return fe_mul(p.y, p.y) == fe_add(fe_mul(fe_mul(p.x, p.x), p.x), fq_small(3));
}
static G1Affine g1_neg(const G1Affine &p) {
    G1Affine r = p;
    if (!p.is_identity()) r.y = fe_neg(p.y);
    return r;
}

// ---------------------------------------------------------------------------------------------- transcript (Blake2bRead)
struct Reader final : TranscriptReader {
    Blake2b st;
    const uint8_t *p;
    size_t len, pos = 0;
    const DecodedPoints *pre;   // the points already decompressed, in reading order (the batch verifier), or nullptr
    size_t pre_pos = 0;
    Reader(const uint8_t *proof, size_t n, const DecodedPoints *decoded = nullptr) : st(64, "Halo2-Transcript"), p(proof), len(n), pre(decoded) {}
    void common_point(const G1Affine &r) {
        uint8_t b[65];
        b[0] = 0x01;
        Fq cx = fe_from_mont(r.x), cy = fe_from_mont(r.y);
        memcpy(b + 1, cx.l, 32);
        memcpy(b + 33, cy.l, 32);
        st.update(b, 65);
    }
    void common_scalar(const Fr &s) override {
        uint8_t b[33];
        b[0] = 0x02;
        fr_repr(s, b + 1);
        st.update(b, 33);
    }
    Fr read_scalar() override {
        Fr c = Fr::zero();
        if (pos + 32 > len) {
            ok = false;
            return c;
        }
        memcpy(c.l, p + pos, 32);
        pos += 32;
        if (!canonical(c)) {
            ok = false;
            return Fr::zero();
        }
        Fr m = fe_to_mont(c);
        common_scalar(m);
        return m;
    }
    G1Affine read_point() override {
        G1Affine r;
        r.x = Fq::zero();
        r.y = Fq::zero();
        if (pos + 32 > len) {
            ok = false;
            return r;
        }
        if (pre) {   // status 1 is the identity, which a prover cannot have written; 2 is what the host path below rejects
            pos += 32;
            if (pre_pos >= pre->n || pre->status[pre_pos] != 0) {
                ok = false;
                ++pre_pos;
                return r;
            }
            r = pre->pts[pre_pos++];
            common_point(r);
            return r;
        }
        Fq x;
        memcpy(x.l, p + pos, 32);
        pos += 32;
        const uint32_t top = x.l[7] >> 24;
        const bool inf = (top >> INF_BIT) & 1u, sign = (top >> SIGN_BIT) & 1u;
        x.l[7] &= ~(((1u << SIGN_BIT) | (1u << INF_BIT)) << 24);
        if (inf || !canonical(x)) {   // a prover cannot have written the identity (Blake2bWrite refuses it)
            ok = false;
            return r;
        }
        const Fq xm = fe_to_mont(x);
        const Fq y2 = fe_add(fe_mul(fe_sqr(xm), xm), fq_small(3));
        uint32_t e[8];   // (q + 1) / 4
        {
            uint64_t carry = 1;
            uint32_t t[8];
            for (int j = 0; j < 8; ++j) {
                uint64_t v = (uint64_t)FqP::m(j) + carry;
                t[j] = (uint32_t)v;
                carry = v >> 32;
            }
            for (int j = 0; j < 8; ++j) e[j] = (t[j] >> 2) | (j < 7 ? t[j + 1] << 30 : 0u);
        }
        Fq y = fe_pow(y2, e);
        if (!(fe_sqr(y) == y2)) {
            ok = false;
            return r;
        }
        if ((fe_from_mont(y).l[0] & 1u) != (sign ? 1u : 0u)) y = fe_neg(y);
        r.x = xm;
        r.y = y;
        common_point(r);
        return r;
    }
    Fr squeeze_challenge() override {
        uint8_t z = 0x00, d[64];
        st.update(&z, 1);
        st.digest(d);
        return fr_from_uniform_bytes(d);
    }
    bool exhausted() const override { return pos == len; }   // trailing bytes make a proof malformed
};

}  // namespace verifier
}  // namespace h2

using namespace h2;
using namespace h2::verifier;

namespace {

// value at u of the polynomial of degree < m through (points[i], evals[i])
Fr interpolate_at(const std::vector<Fr> &points, const std::vector<Fr> &evals, const Fr &u) {
    Fr acc = Fr::zero();
    for (size_t j = 0; j < points.size(); ++j) {
        Fr num = Fr::one(), den = Fr::one();
        for (size_t i = 0; i < points.size(); ++i) {
            if (i == j) continue;
            num = fe_mul(num, fe_sub(u, points[i]));
            den = fe_mul(den, fe_sub(points[j], points[i]));
        }
        acc = fe_add(acc, fe_mul(evals[j], fe_mul(num, fe_inv(den))));
    }
    return acc;
}
F2 load_f2(const uint8_t *p) {
    F2 r;
    memcpy(r.c0.l, p, 32);
    memcpy(r.c1.l, p + 32, 32);
    return r;
}

}  // namespace

namespace h2 {
namespace verifier {

int check_key(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens) {
    H2_REQUIRE(sh.perm_columns.empty() || vk.permutation_commitments, "NULL argument");
    H2_REQUIRE(sh.p.num_instance == 0 || (instances_host && instance_lens), "NULL argument");
    G2A Q2 = {load_f2((const uint8_t *)vk.g2), load_f2((const uint8_t *)vk.g2 + 64), false},
        SQ2 = {load_f2((const uint8_t *)vk.s_g2), load_f2((const uint8_t *)vk.s_g2 + 64), false};
    H2_REQUIRE(g2_on_curve(Q2) && g2_on_curve(SQ2), "g2 / s_g2 are not points of the twist");
    return H2HIP_OK;
}

// The prover writes num_commitments() points and num_evals() scalars.  (The advice commitments of a multi-phase proof come phase by phase,
// but every advice column belongs to exactly one phase, so they are num_advice_total words in either order.)
size_t proof_words(const plonk::Shape &sh, std::vector<uint32_t> *point_words) {
    const size_t head = sh.num_commitments() - 2, evals = sh.num_evals();   // head: every commitment up to the h pieces
    if (point_words) {
        point_words->clear();
        for (size_t i = 0; i < head; ++i) point_words->push_back((uint32_t)i);
        point_words->push_back((uint32_t)(head + evals));       // h1
        point_words->push_back((uint32_t)(head + evals + 1));   // h2
    }
    return head + evals + 2;
}

// derive: the transcript replay, the quotient identity rebuilt from the openings, SHPLONK's folded opening as a list of (commitment, scalar)
int derive(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens, const uint8_t *proof, size_t proof_len,
           const DecodedPoints *pre, Derived *out, int *well_formed) {
    Reader tr(proof, proof_len, pre);
    return derive(sh, vk, instances_host, instance_lens, tr, out, well_formed);
}
int derive(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens, TranscriptReader &tr, Derived *out,
           int *well_formed) {
    *well_formed = 0;
    const uint32_t k = sh.k, n = sh.n, bf = sh.blinding_factors, chunk = sh.chunk_len;
    const uint32_t num_instance = sh.p.num_instance, num_lookups = (uint32_t)sh.lookups.size(), num_perm_columns = (uint32_t)sh.perm_columns.size();
    std::vector<G1Affine> fixed_comm(sh.num_fixed_total), perm_comm(num_perm_columns);
    memcpy(fixed_comm.data(), vk.fixed_commitments, sizeof(G1Affine) * fixed_comm.size());
    if (!perm_comm.empty()) memcpy(perm_comm.data(), vk.permutation_commitments, sizeof(G1Affine) * perm_comm.size());
    Fr repr;
    memcpy(&repr, vk.transcript_repr, sizeof(Fr));
    Fr omega = fr_from_canonical_u64x4(plonk::ROOT_OF_UNITY);
    for (uint32_t i = k; i < 28; ++i) omega = fe_sqr(omega);
    const Fr delta = fr_from_canonical_u64x4(plonk::DELTA), one = Fr::one();

    tr.common_scalar(repr);
    std::vector<std::vector<Fr>> inst(num_instance);
    for (uint32_t i = 0; i < num_instance; ++i) {
        if (instance_lens[i] > sh.usable_rows) return H2HIP_OK;   // InstanceTooLarge: rejected
        inst[i].resize(instance_lens[i]);
        if (instance_lens[i]) memcpy(inst[i].data(), instances_host[i], sizeof(Fr) * instance_lens[i]);
        for (const Fr &v : inst[i]) tr.common_scalar(v);
    }
    std::vector<G1Affine> advice_comm(sh.num_advice_total);
    std::vector<Fr> challenges;
    if (!sh.phased) {   // (also a one-phase key of the multi-phase configuration, whose phase_cols[0] is every column in index order)
        for (auto &c : advice_comm) c = tr.read_point();
    } else {   // phase by phase, each followed by its challenges (only the RLC gates query one, challenge 0)
        for (size_t ph = 0; ph < sh.phase_cols.size(); ++ph) {
            for (int c : sh.phase_cols[ph]) advice_comm[c] = tr.read_point();
            for (uint32_t i = 0; i < sh.phase_challenges[ph]; ++i) challenges.push_back(tr.squeeze_challenge());
        }
    }
    if (sh.num_rlc && challenges.empty()) return H2HIP_OK;   // (Shape::init_rlc requires the challenge)
    const Fr theta = tr.squeeze_challenge();
    std::vector<G1Affine> lk_a_comm(num_lookups), lk_s_comm(num_lookups), lk_z_comm(num_lookups), permz_comm(sh.num_perm_sets);
    for (uint32_t i = 0; i < num_lookups; ++i) {
        lk_a_comm[i] = tr.read_point();
        lk_s_comm[i] = tr.read_point();
    }
    const Fr beta = tr.squeeze_challenge(), gamma = tr.squeeze_challenge();
    for (auto &c : permz_comm) c = tr.read_point();
    for (auto &c : lk_z_comm) c = tr.read_point();
    const G1Affine random_comm = tr.read_point();
    const Fr y = tr.squeeze_challenge();
    std::vector<G1Affine> h_comm(sh.quotient_pieces);
    for (auto &c : h_comm) c = tr.read_point();
    const Fr x = tr.squeeze_challenge();
    // evaluations, in the prover's order
    const auto &adv_q = sh.advice_queries;
    std::vector<Fr> adv_ev(adv_q.size());
    for (auto &e : adv_ev) e = tr.read_scalar();
    std::map<std::pair<int, int>, Fr> adv_at_q;
    for (size_t i = 0; i < adv_q.size(); ++i) adv_at_q[adv_q[i]] = adv_ev[i];
    std::vector<Fr> fixed_ev(sh.num_fixed_total, Fr::zero());
    for (const auto &q : sh.fixed_queries) fixed_ev[q.first] = tr.read_scalar();   // (every fixed column is queried at the current row)
    const Fr random_eval = tr.read_scalar();
    std::vector<Fr> sigma_ev(num_perm_columns);
    for (auto &e : sigma_ev) e = tr.read_scalar();
    struct PermEv {
        Fr e0, e1, e2;
    };
    std::vector<PermEv> perm_ev(sh.num_perm_sets);
    for (uint32_t si = 0; si < sh.num_perm_sets; ++si) {
        perm_ev[si].e0 = tr.read_scalar();
        perm_ev[si].e1 = tr.read_scalar();
        perm_ev[si].e2 = si + 1 != sh.num_perm_sets ? tr.read_scalar() : Fr::zero();
    }
    struct LkEv {
        Fr pe, pne, ae, aie, se;
    };
    std::vector<LkEv> lk_ev(num_lookups);
    for (auto &l : lk_ev) {
        l.pe = tr.read_scalar();
        l.pne = tr.read_scalar();
        l.ae = tr.read_scalar();
        l.aie = tr.read_scalar();
        l.se = tr.read_scalar();
    }
    if (tr.err != H2HIP_OK) return tr.err;   // the caller's transcript failed
    if (!tr.ok) return H2HIP_OK;   // malformed proof
    // ---- the quotient identity at x
    const Fr xn = fe_pow_u64(x, n);
    auto rot = [&](int r) -> Fr {
        int64_t rr = ((int64_t)r % (int64_t)n + (int64_t)n) % (int64_t)n;
        return fe_mul(x, fe_pow_u64(omega, (uint64_t)rr));
    };
    auto l_i = [&](int r) -> Fr {   // l_r(x) = (x^n - 1) * omega^r / (n * (x - omega^r))
        int64_t rr = ((int64_t)r % (int64_t)n + (int64_t)n) % (int64_t)n;
        Fr wi = fe_pow_u64(omega, (uint64_t)rr);
        return fe_mul(fe_mul(fe_sub(xn, one), wi), fe_inv(fe_mul(fr_from_u64(n), fe_sub(x, wi))));
    };
    if (fe_sub(xn, one).is_zero()) return H2HIP_OK;   // x on the domain: negligible; reject rather than divide by zero
    std::vector<Fr> inst_ev(num_instance, Fr::zero());
    {   // l_j(x) for every instance row j, with ONE inversion (Montgomery's trick) for all the denominators n * (x - omega^j)
        size_t rows = 0;
        for (const auto &col : inst) rows = std::max(rows, col.size());
        std::vector<Fr> lj(rows), den(rows), pre_prod(rows);
        Fr wi = one, run = one;
        for (size_t j = 0; j < rows; ++j) {
            lj[j] = fe_mul(fe_sub(xn, one), wi);
            den[j] = fe_mul(fr_from_u64(n), fe_sub(x, wi));
            pre_prod[j] = run;
            run = fe_mul(run, den[j]);
            wi = fe_mul(wi, omega);
        }
        Fr inv = rows ? fe_inv(run) : one;
        for (size_t j = rows; j-- > 0;) {
            lj[j] = fe_mul(lj[j], fe_mul(inv, pre_prod[j]));
            inv = fe_mul(inv, den[j]);
        }
        for (uint32_t c = 0; c < num_instance; ++c)
            for (size_t j = 0; j < inst[c].size(); ++j) inst_ev[c] = fe_add(inst_ev[c], fe_mul(inst[c][j], lj[j]));
    }
    const Fr l_last = l_i(-(int)(bf + 1)), l_0 = l_i(0);
    Fr l_blind = Fr::zero();
    for (uint32_t r = 1; r <= bf; ++r) l_blind = fe_add(l_blind, l_i(-(int)(bf + 1) + (int)r));
    const Fr active = fe_sub(fe_sub(one, l_last), l_blind);
    auto adv_at = [&](int col, int r) -> Fr { return adv_at_q[{col, r}]; };
    auto col_eval = [&](const plonk::ColumnRef &c) -> Fr { return c.kind == 0 ? fixed_ev[c.index] : c.kind == 1 ? adv_at(c.index, 0) : inst_ev[c.index]; };
    auto compress = [&](const std::vector<plonk::ColumnProduct> &exprs) -> Fr {
        Fr acc = Fr::zero();
        for (const plonk::ColumnProduct &e : exprs) {
            Fr t = one;
            for (size_t i = 0; i < e.size(); ++i) t = i ? fe_mul(t, col_eval(e[i])) : col_eval(e[i]);
            acc = fe_add(fe_mul(acc, theta), t);
        }
        return acc;
    };
    Fr expected = Fr::zero();
    auto fold = [&](const Fr &term) { expected = fe_add(fe_mul(expected, y), term); };
    for (const auto &g : sh.gates()) {
        const int a = g.second;
        fold(fe_mul(fixed_ev[g.first], fe_sub(fe_add(adv_at(a, 0), fe_mul(adv_at(a, 1), adv_at(a, 2))), adv_at(a, 3))));
    }
    for (const auto &g : sh.rlc_gates()) {
        const int a = g.second;
        fold(fe_mul(fixed_ev[g.first], fe_sub(fe_add(fe_mul(adv_at(a, 0), challenges[0]), adv_at(a, 1)), adv_at(a, 2))));
    }
    if (sh.num_perm_sets) {
        fold(fe_mul(l_0, fe_sub(one, perm_ev[0].e0)));
        const Fr zl = perm_ev[sh.num_perm_sets - 1].e0;
        fold(fe_mul(l_last, fe_sub(fe_sqr(zl), zl)));
        for (uint32_t si = 1; si < sh.num_perm_sets; ++si) fold(fe_mul(l_0, fe_sub(perm_ev[si].e0, perm_ev[si - 1].e2)));
        for (uint32_t si = 0; si < sh.num_perm_sets; ++si) {
            const uint32_t c0 = si * chunk, c1 = std::min<uint32_t>(c0 + chunk, num_perm_columns);
            Fr left = perm_ev[si].e1, right = perm_ev[si].e0;
            Fr cur = fe_mul(fe_mul(beta, x), fe_pow_u64(delta, c0));
            for (uint32_t c = c0; c < c1; ++c) left = fe_mul(left, fe_add(fe_add(col_eval(sh.perm_columns[c]), fe_mul(beta, sigma_ev[c])), gamma));
            for (uint32_t c = c0; c < c1; ++c) {
                right = fe_mul(right, fe_add(fe_add(col_eval(sh.perm_columns[c]), cur), gamma));
                cur = fe_mul(cur, delta);
            }
            fold(fe_mul(active, fe_sub(left, right)));
        }
    }
    for (uint32_t li = 0; li < num_lookups; ++li) {
        const LkEv &l = lk_ev[li];
        std::vector<plonk::ColumnProduct> lk_in, lk_tab;
        sh.lookup_exprs(li, lk_in, lk_tab);
        const Fr inp = compress(lk_in), tab = compress(lk_tab);
        fold(fe_mul(l_0, fe_sub(one, l.pe)));
        fold(fe_mul(l_last, fe_sub(fe_sqr(l.pe), l.pe)));
        fold(fe_mul(active, fe_sub(fe_mul(fe_mul(l.pne, fe_add(l.ae, beta)), fe_add(l.se, gamma)), fe_mul(fe_mul(l.pe, fe_add(inp, beta)), fe_add(tab, gamma)))));
        fold(fe_mul(l_0, fe_sub(l.ae, l.se)));
        fold(fe_mul(active, fe_mul(fe_sub(l.ae, l.se), fe_sub(l.ae, l.aie))));
    }
    const Fr expected_h = fe_mul(expected, fe_inv(fe_sub(xn, one)));
    // ---- commitments and queries in the prover's order
    struct CommRef {
        int vk_slot;   // as Term::vk_slot; -2: the h commitment, which enters the list piece by piece
        G1Affine p;
    };
    std::vector<CommRef> comm;
    auto add_comm = [&](const G1Affine &c, int vk_slot = -1) -> int {
        comm.push_back({vk_slot, c});
        return (int)comm.size() - 1;
    };
    std::vector<plonk::Query> queries;
    std::vector<int> adv_key(sh.num_advice_total);
    for (uint32_t c = 0; c < sh.num_advice_total; ++c) adv_key[c] = add_comm(advice_comm[c]);
    for (size_t i = 0; i < adv_q.size(); ++i) queries.push_back({adv_key[adv_q[i].first], rot(adv_q[i].second), adv_ev[i]});
    const Fr x_next = rot(1), x_last = rot(-(int)(bf + 1)), x_inv = rot(-1);
    {
        std::vector<plonk::Query> tail;
        for (uint32_t si = 0; si < sh.num_perm_sets; ++si) {
            int key = add_comm(permz_comm[si]);
            queries.push_back({key, x, perm_ev[si].e0});
            queries.push_back({key, x_next, perm_ev[si].e1});
            if (si + 1 != sh.num_perm_sets) tail.push_back({key, x_last, perm_ev[si].e2});
        }
        for (size_t t = tail.size(); t-- > 0;) queries.push_back(tail[t]);
    }
    for (uint32_t li = 0; li < num_lookups; ++li) {
        int kz = add_comm(lk_z_comm[li]), ka = add_comm(lk_a_comm[li]), ks = add_comm(lk_s_comm[li]);
        const LkEv &l = lk_ev[li];
        queries.push_back({kz, x, l.pe});
        queries.push_back({ka, x, l.ae});
        queries.push_back({ks, x, l.se});
        queries.push_back({ka, x_inv, l.aie});
        queries.push_back({kz, x_next, l.pne});
    }
    for (const auto &q : sh.fixed_queries) queries.push_back({add_comm(fixed_comm[q.first], q.first), x, fixed_ev[q.first]});
    for (uint32_t j = 0; j < num_perm_columns; ++j) queries.push_back({add_comm(perm_comm[j], (int)(sh.num_fixed_total + j)), x, sigma_ev[j]});
    // h commitment = sum_i xn^i H_i: no point arithmetic here, the pieces enter the list with scalar * xn^i
    G1Affine h_placeholder;
    h_placeholder.x = Fq::zero();
    h_placeholder.y = Fq::zero();
    queries.push_back({add_comm(h_placeholder, -2), x, expected_h});
    queries.push_back({add_comm(random_comm), x, random_eval});
    // ---- VerifierSHPLONK
    // the grouping the prover ran.  It returns no sets beyond 64 distinct points; a verifier opens at seven at most (x and its rotations
    // -1, 1, 2, 3 and last), so an empty result is a rejection, never an index out of range below
    std::vector<plonk::RotationSet> sets;
    std::vector<Fr> super_points;
    plonk::construct_intermediate_sets(queries, sets, super_points);
    if (sets.empty()) return H2HIP_OK;
    const Fr y2 = tr.squeeze_challenge(), v = tr.squeeze_challenge();
    const G1Affine h1 = tr.read_point();
    const Fr u = tr.squeeze_challenge();
    const G1Affine h2 = tr.read_point();
    if (tr.err != H2HIP_OK) return tr.err;
    if (!tr.ok || !tr.exhausted()) return H2HIP_OK;   // malformed or trailing bytes
    out->terms.clear();
    Fr r_outer = Fr::zero(), z_0 = Fr::zero(), z_0_diff_inv = Fr::zero(), vpow = one;
    for (size_t i = 0; i < sets.size(); ++i) {
        Fr z_diff = one;
        for (const Fr &p : super_points) {
            bool in_set = false;
            for (const Fr &sp : sets[i].points) in_set |= fr_cmp(sp, p) == 0;
            if (!in_set) z_diff = fe_mul(z_diff, fe_sub(u, p));
        }
        if (i == 0) {
            z_0 = one;
            for (const Fr &p : sets[i].points) z_0 = fe_mul(z_0, fe_sub(u, p));
            if (z_diff.is_zero()) return H2HIP_OK;
            z_0_diff_inv = fe_inv(z_diff);
            z_diff = one;
        } else {
            z_diff = fe_mul(z_diff, z_0_diff_inv);
        }
        const Fr scale = fe_mul(vpow, z_diff);
        Fr r_inner = Fr::zero(), ypow = one;
        for (size_t j = 0; j < sets[i].polys.size(); ++j) {
            r_inner = fe_add(r_inner, fe_mul(ypow, interpolate_at(sets[i].points, sets[i].evals[j], u)));
            const CommRef &c = comm[sets[i].polys[j]];
            Fr s = fe_mul(scale, ypow);
            if (c.vk_slot == -2) {
                for (const G1Affine &piece : h_comm) {
                    out->terms.push_back({-1, piece, s});
                    s = fe_mul(s, xn);
                }
            } else {
                out->terms.push_back({c.vk_slot, c.p, s});
            }
            ypow = fe_mul(ypow, y2);
        }
        r_outer = fe_add(r_outer, fe_mul(scale, r_inner));
        vpow = fe_mul(vpow, v);
    }
    out->g0_scalar = fe_neg(r_outer);
    out->terms.push_back({-1, h1, fe_neg(z_0)});
    out->terms.push_back({-1, h2, u});
    out->w = h2;
    *well_formed = 1;
    return H2HIP_OK;
}

// finish, one proof: the scalar multiplications by double-and-add on the host ...
G1Affine outer_on_host(const VKey &vk, const Derived &d) {
    G1Affine g0;
    memcpy(&g0, vk.g1, sizeof(G1Affine));
    XYZZ outer = g1_scalar_mul(g0, d.g0_scalar);
    for (const Term &t : d.terms) {
        XYZZ m = g1_scalar_mul(t.p, t.s);
        xyzz_add(outer, m);
    }
    return xyzz_to_affine(outer);
}
// ... and DualMSM::check: e(left, s*g2) * e(-outer, g2) == 1
int pairing_verdict(const VKey &vk, const G1Affine &left, const G1Affine &outer, int *accepted) {
    G2A Q2 = {load_f2((const uint8_t *)vk.g2), load_f2((const uint8_t *)vk.g2 + 64), false},
        SQ2 = {load_f2((const uint8_t *)vk.s_g2), load_f2((const uint8_t *)vk.s_g2 + 64), false};
    F12 f = f12_mul(miller_loop(left, SQ2), miller_loop(g1_neg(outer), Q2));
    *accepted = f12_is_one(final_exponentiation(f)) ? 1 : 0;
    return H2HIP_OK;
}

// derive over any reader, then the finish on the host; acc_out (optional) receives (W', outer), the pair the pairing decides
static int verify_over(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens, TranscriptReader &tr,
                       int *accepted, void *acc_out) {
    *accepted = 0;
    H2_CHK(check_key(sh, vk, instances_host, instance_lens));
    Derived d;
    int well_formed = 0;
    H2_CHK(derive(sh, vk, instances_host, instance_lens, tr, &d, &well_formed));
    if (!well_formed) return H2HIP_OK;   // a malformed proof is a rejection
    const G1Affine outer = outer_on_host(vk, d);
    if (acc_out) {
        memcpy(acc_out, &d.w, sizeof(G1Affine));
        memcpy((uint8_t *)acc_out + sizeof(G1Affine), &outer, sizeof(G1Affine));
    }
    return pairing_verdict(vk, d.w, outer, accepted);
}
int verify_one(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens, const uint8_t *proof, size_t proof_len,
               int *accepted) {
    Reader tr(proof, proof_len);
    return verify_over(sh, vk, instances_host, instance_lens, tr, accepted, nullptr);
}
// what the four h2hip_plonk_verify_proof* entries run behind their argument checks
static int verify_kind(int kind, const void *params, const VKey &vk, const void *const *instances_host, const size_t *instance_lens, const uint8_t *proof,
                       size_t proof_len, int *accepted) {
    *accepted = 0;
    plonk::Shape sh;
    H2_CHK(plonk::shape_of_kind(kind, params, sh));
    return verify_one(sh, vk, instances_host, instance_lens, proof, proof_len, accepted);
}

}  // namespace verifier
}  // namespace h2

extern "C" {

// verify_proof + VerifierSHPLONK + SingleStrategy for a BaseConfig circuit.  fixed_commitments / permutation_commitments: the verifying key
// (h2hip_plonk_pk_commitments), transcript_repr: the key's hash into the transcript, g1: params.g[0] (the G1 generator of the SRS), g2 / s_g2:
// 128 bytes each as SerdeFormat::RawBytes stores them (x.c0, x.c1, y.c0, y.c1 Montgomery limbs).  *accepted = 1 iff the proof verifies; a
// malformed proof is a rejection (accepted = 0, return H2HIP_OK); H2HIP_ERR_INVALID is reserved for bad arguments.
int h2hip_plonk_verify_proof(const h2hip_base_circuit_params *params, const void *fixed_commitments, const void *permutation_commitments,
                             const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, const void *const *instances_host,
                             const size_t *instance_lens, const uint8_t *proof, size_t proof_len, int *accepted) {
    H2_REQUIRE(params && fixed_commitments && transcript_repr && g1 && g2 && s_g2 && proof && accepted, "NULL argument");
    return verify_kind(H2HIP_CIRCUIT_BASE, params, {fixed_commitments, permutation_commitments, transcript_repr, g1, g2, s_g2}, instances_host, instance_lens, proof,
                       proof_len, accepted);
}

// the same for the dynamic-lookup configuration (include/h2hip.h states its layout): the lookups' compressed input and table evaluations are
// Horner sums in theta of the advice / fixed openings at x
int h2hip_plonk_verify_proof_dyn(const h2hip_dyn_circuit_params *params, const void *fixed_commitments, const void *permutation_commitments,
                                 const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, const uint8_t *proof, size_t proof_len,
                                 int *accepted) {
    H2_REQUIRE(params && fixed_commitments && transcript_repr && g1 && g2 && s_g2 && proof && accepted, "NULL argument");
    return verify_kind(H2HIP_CIRCUIT_DYN, params, {fixed_commitments, permutation_commitments, transcript_repr, g1, g2, s_g2}, nullptr, nullptr, proof,
                       proof_len, accepted);
}

// the same for the multi-phase configuration (include/h2hip.h states its layout): the advice commitments are read phase by phase, each phase's
// challenges squeezed after them; one used phase without challenges is h2hip_plonk_verify_proof of that phase's BaseCircuitParams
int h2hip_plonk_verify_proof_phased(const h2hip_phased_circuit_params *params, const void *fixed_commitments, const void *permutation_commitments,
                                    const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, const void *const *instances_host,
                                    const size_t *instance_lens, const uint8_t *proof, size_t proof_len, int *accepted) {
    H2_REQUIRE(params && fixed_commitments && transcript_repr && g1 && g2 && s_g2 && proof && accepted, "NULL argument");
    return verify_kind(H2HIP_CIRCUIT_PHASED, params, {fixed_commitments, permutation_commitments, transcript_repr, g1, g2, s_g2}, instances_host, instance_lens, proof,
                       proof_len, accepted);
}

// the same for the RLC configuration (include/h2hip.h states its layout): as the multi-phase verifier, with challenge 0 of the replay in the
// RLC gates' terms of the quotient identity
int h2hip_plonk_verify_proof_rlc(const h2hip_rlc_circuit_params *params, const void *fixed_commitments, const void *permutation_commitments,
                                 const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, const void *const *instances_host,
                                 const size_t *instance_lens, const uint8_t *proof, size_t proof_len, int *accepted) {
    H2_REQUIRE(params && fixed_commitments && transcript_repr && g1 && g2 && s_g2 && proof && accepted, "NULL argument");
    return verify_kind(H2HIP_CIRCUIT_RLC, params, {fixed_commitments, permutation_commitments, transcript_repr, g1, g2, s_g2}, instances_host, instance_lens, proof,
                       proof_len, accepted);
}

// verify_proof over the caller's transcript (include/h2hip.h): derive over the callback reader, the scalar multiplications on the host, one
// pairing; acc_out receives (W', outer), the pair the pairing decides
int h2hip_plonk_verify_proof_transcript(int kind, const void *params, const void *fixed_commitments, const void *permutation_commitments,
                                        const void *transcript_repr, const void *g1, const void *g2, const void *s_g2,
                                        const void *const *instances_host, const size_t *instance_lens, const h2hip_transcript *t, int *accepted,
                                        void *acc_out) {
    H2_REQUIRE(params && fixed_commitments && transcript_repr && g1 && g2 && s_g2 && t && accepted, "NULL argument");
    *accepted = 0;
    if (acc_out) memset(acc_out, 0, 2 * sizeof(G1Affine));
    H2_REQUIRE(t->common_scalar && t->read_point && t->read_scalar && t->squeeze_challenge,
               "h2hip_plonk_verify_proof_transcript: the transcript lacks common_scalar, read_point, read_scalar or squeeze_challenge");
    H2_REQUIRE(kind == H2HIP_CIRCUIT_BASE || kind == H2HIP_CIRCUIT_DYN || kind == H2HIP_CIRCUIT_PHASED || kind == H2HIP_CIRCUIT_RLC,
               "unknown circuit kind (H2HIP_CIRCUIT_BASE / _DYN / _PHASED / _RLC)");
    plonk::Shape sh;
    H2_CHK(plonk::shape_of_kind(kind, params, sh));
    CallbackReader tr(t);
    return verify_over(sh, {fixed_commitments, permutation_commitments, transcript_repr, g1, g2, s_g2}, instances_host, instance_lens, tr, accepted, acc_out);
}

// e(P_0, Q_0) * ... * e(P_{n-1}, Q_{n-1}) == 1 — the "final CPU-side pairing" of the north star as an entry of its own (the verifier above ends in
// the two-pair instance of it).  g1: n x 64 B Montgomery G1Affine (identity = all-zero), g2: n x 128 B RawBytes (x.c0, x.c1, y.c0, y.c1), identity = all-zero.
int h2hip_pairing_check(const void *g1_points, const void *g2_points, size_t n, int *is_one) {
    H2_REQUIRE(is_one && (n == 0 || (g1_points && g2_points)), "null argument");
    *is_one = 0;
    F12 f = f12_one();
    for (size_t i = 0; i < n; ++i) {
        G1Affine P;
        memcpy(&P, (const uint8_t *)g1_points + 64 * i, 64);
        const uint8_t *q = (const uint8_t *)g2_points + 128 * i;
        G2A Q = {load_f2(q), load_f2(q + 64), false};
        Q.inf = f2_is_zero(Q.x) && f2_is_zero(Q.y);
        H2_REQUIRE(canonical(P.x) && canonical(P.y) && (P.is_identity() || g1_on_curve_host(P)), "a G1 point is not on the curve");
        H2_REQUIRE(canonical(Q.x.c0) && canonical(Q.x.c1) && canonical(Q.y.c0) && canonical(Q.y.c1), "a G2 coordinate is not a canonical field element");
        H2_REQUIRE(g2_on_curve(Q), "a G2 point is not on the twist");
        H2_REQUIRE(g2_in_subgroup(Q), "a G2 point is not in the order-r subgroup");
        f = f12_mul(f, miller_loop(P, Q));
    }
    *is_one = f12_is_one(final_exponentiation(f)) ? 1 : 0;
    return H2HIP_OK;
}

// BLAKE2b (RFC 7693), unkeyed, with an optional 16-byte personalisation: the transcript's hash (blake2b.h) as an entry of its own, so that it can
// be pinned against the RFC's vectors and an independent implementation.  personal16: 16 bytes or NULL.
int h2hip_blake2b(const void *personal16, unsigned digest_len, const void *msg, size_t len, void *out) {
    H2_REQUIRE(out && digest_len >= 1 && digest_len <= 64 && (len == 0 || msg), "bad argument");
    uint8_t pers[16] = {0};
    if (personal16) memcpy(pers, personal16, 16);
    h2::Blake2b h = h2::Blake2b::with_personal16(digest_len, pers);
    h.update(msg, len);
    uint8_t d[64];
    h.digest(d);
    memcpy(out, d, digest_len);
    return H2HIP_OK;
}

}  // extern "C"
