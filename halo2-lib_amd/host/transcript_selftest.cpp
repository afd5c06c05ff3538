// A caller-owned transcript through the C++ host mirror: a Blake2b transcript implemented HERE, natively, behind
// plonk::create_proof_with_transcript / plonk::verify_proof_with_transcript — it keeps the absorbed bytes and calls h2hip_blake2b on every
// squeeze — proves selftest.cpp's small circuit.  In Blake2bWrite's encoding the bytes must be the built-in entry's (and what
// `selftest <k> --dump-proof` prints); in an encoding of its own (points uncompressed) the library's verifier accepts the proof through the
// native reader and hands out its accumulator; a transcript that throws aborts the proof and leaves the key usable.
// usage: transcript_selftest [k] [--dump-proof | --time]    (links against libh2hip.so — or, in CPU tests, the emulated build)
// --time: host clock around whole proofs (advice resident on the device, libh2hip's seeded ChaCha generator), median of 7 after two warm-up
// proofs: the built-in entry next to the same proof through the native transcript's callbacks.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>

#include "halo2_proofs.hpp"

using namespace halo2_proofs;

// ---- 4 x u64 Montgomery arithmetic for either modulus (the host mirror itself only carries F_r)
struct Mont {
    uint64_t mod[4], ninv, r2[4];   // ninv = -mod^-1 mod 2^64, r2 = 2^512 mod `mod`
    explicit Mont(const uint64_t m[4]) {
        memcpy(mod, m, 32);
        uint64_t inv = 1;
        for (int i = 0; i < 6; ++i) inv *= 2 - mod[0] * inv;   // Newton: doubles the correct bits
        ninv = 0 - inv;
        uint64_t v[4] = {1, 0, 0, 0};
        for (int i = 0; i < 512; ++i) dbl(v);
        memcpy(r2, v, 32);
    }
    bool geq(const uint64_t a[4]) const {
        for (int i = 3; i >= 0; --i)
            if (a[i] != mod[i]) return a[i] > mod[i];
        return true;
    }
    void sub_mod(uint64_t a[4]) const {
        unsigned __int128 br = 0;
        for (int i = 0; i < 4; ++i) {
            unsigned __int128 d = (unsigned __int128)a[i] - mod[i] - br;
            a[i] = (uint64_t)d;
            br = (d >> 64) & 1;
        }
    }
    void dbl(uint64_t a[4]) const {   // a < mod < 2^254: no carry out
        for (int i = 3; i >= 0; --i) a[i] = (a[i] << 1) | (i ? a[i - 1] >> 63 : 0);
        if (geq(a)) sub_mod(a);
    }
    void mul(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) const {   // a * b / 2^256 mod `mod`, for a < 2^256 and b < mod
        typedef unsigned __int128 u128;
        uint64_t t[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 4; ++i) {
            u128 c = 0;
            for (int j = 0; j < 4; ++j) {
                c += (u128)a[j] * b[i] + t[j];
                t[j] = (uint64_t)c;
                c >>= 64;
            }
            c += t[4];
            t[4] = (uint64_t)c;
            t[5] = (uint64_t)(c >> 64);
            const uint64_t m = t[0] * ninv;
            c = ((u128)m * mod[0] + t[0]) >> 64;
            for (int j = 1; j < 4; ++j) {
                c += (u128)m * mod[j] + t[j];
                t[j - 1] = (uint64_t)c;
                c >>= 64;
            }
            c += t[4];
            t[3] = (uint64_t)c;
            t[4] = t[5] + (uint64_t)(c >> 64);
        }
        uint64_t r[4] = {t[0], t[1], t[2], t[3]};
        if (t[4] || geq(r)) sub_mod(r);
        memcpy(out, r, 32);
    }
    void to_canonical(const uint64_t a[4], uint64_t out[4]) const {
        const uint64_t one[4] = {1, 0, 0, 0};
        mul(a, one, out);
    }
    void to_mont(const uint64_t a[4], uint64_t out[4]) const { mul(a, r2, out); }
    bool canonical(const uint64_t a[4]) const { return !geq(a); }
};
static const uint64_t Q_MOD[4] = {0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
static const Mont FQ(Q_MOD), FR(host_fr::MOD);

// ---- Blake2bWrite / Blake2bRead + Challenge255, natively: every absorbed byte is kept, a squeeze hashes all of them
struct NativeBlake2b : plonk::Transcript {
    bool compress;                 // true: Blake2bWrite's encoding (32-byte compressed points); false: points as 64 bytes (x, y)
    std::vector<uint8_t> absorbed, proof;
    size_t pos = 0;                // reading position in `proof`
    size_t points_written = 0, fail_at_point = 0;   // fail_at_point != 0: that write_point throws
    explicit NativeBlake2b(bool compress_) : compress(compress_) {}
    void common_point(const G1Affine &p) override {
        uint64_t x[4], y[4];
        FQ.to_canonical(p.x.l, x);
        FQ.to_canonical(p.y.l, y);
        absorbed.push_back(0x01);
        absorbed.insert(absorbed.end(), (const uint8_t *)x, (const uint8_t *)x + 32);
        absorbed.insert(absorbed.end(), (const uint8_t *)y, (const uint8_t *)y + 32);
    }
    void common_scalar(const Fr &s) override {
        uint64_t c[4];
        FR.to_canonical(s.l, c);
        absorbed.push_back(0x02);
        absorbed.insert(absorbed.end(), (const uint8_t *)c, (const uint8_t *)c + 32);
    }
    void write_point(const G1Affine &p) override {
        if (++points_written == fail_at_point) throw std::runtime_error("the caller's transcript gave up");
        common_point(p);
        uint64_t x[4], y[4];
        FQ.to_canonical(p.x.l, x);
        FQ.to_canonical(p.y.l, y);
        uint8_t b[64];
        memcpy(b, x, 32);
        memcpy(b + 32, y, 32);
        if (compress) {
            b[31] |= (uint8_t)((b[32] & 1) << 6);   // sign(y) in bit 6 of the top byte
            proof.insert(proof.end(), b, b + 32);
        } else {
            proof.insert(proof.end(), b, b + 64);
        }
    }
    void write_scalar(const Fr &s) override {
        common_scalar(s);
        uint64_t c[4];
        FR.to_canonical(s.l, c);
        proof.insert(proof.end(), (const uint8_t *)c, (const uint8_t *)c + 32);
    }
    G1Affine read_point() override {   // the uncompressed encoding only (no square root on this side)
        if (compress || pos + 64 > proof.size()) throw std::runtime_error("read_point");
        uint64_t x[4], y[4];
        memcpy(x, proof.data() + pos, 32);
        memcpy(y, proof.data() + pos + 32, 32);
        pos += 64;
        if (!FQ.canonical(x) || !FQ.canonical(y)) throw std::runtime_error("read_point: not canonical");
        G1Affine p;
        FQ.to_mont(x, p.x.l);
        FQ.to_mont(y, p.y.l);
        common_point(p);   // (the library checks the curve equation)
        return p;
    }
    Fr read_scalar() override {
        if (pos + 32 > proof.size()) throw std::runtime_error("read_scalar");
        uint64_t c[4];
        memcpy(c, proof.data() + pos, 32);
        pos += 32;
        if (!FR.canonical(c)) throw std::runtime_error("read_scalar: not canonical");
        Fr s;
        FR.to_mont(c, s.l);
        common_scalar(s);
        return s;
    }
    Fr squeeze_challenge() override {
        absorbed.push_back(0x00);
        uint64_t d[8];
        check(h2hip_blake2b("Halo2-Transcript", 64, absorbed.data(), absorbed.size(), d));
        // Fr::from_uniform_bytes: the 512-bit little-endian integer mod r = lo + hi * 2^256
        uint64_t lo[4], hi[4], hi2[4];
        FR.to_mont(d, lo);
        FR.to_mont(d + 4, hi);
        FR.to_mont(hi, hi2);
        Fr a, b;
        memcpy(a.l, lo, 32);
        memcpy(b.l, hi2, 32);
        return host_fr::add(a, b);
    }
};

// ---- selftest.cpp's small circuit (its prove_small_circuit, with the same seeds): 1 advice column with the lookup behind q_lookup
static uint64_t sm(uint64_t &s) {
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static Fr draw_fr(uint64_t &s) {
    uint64_t c[4] = {sm(s), sm(s), sm(s), sm(s) >> 4};
    return host_fr::from_canonical(c);
}
struct StreamRng {
    uint64_t state;
    void operator()(Fr *out, size_t n) {
        for (size_t i = 0; i < n; ++i) out[i] = draw_fr(state);
    }
};
struct SmallCircuit {
    h2hip_base_circuit_params bp;
    h2hip_plonk_shape sh;
    std::vector<std::vector<Fr>> fixed, advice;
    std::vector<uint32_t> copies;
    Fr toxic, repr;
    SmallCircuit(uint32_t k, uint64_t circuit_seed) {
        const uint32_t lb = k - 2;
        bp = {k, 1, 1, 1, 0, (int32_t)lb};
        check(h2hip_plonk_shape_of(&bp, &sh));
        const size_t n = (size_t)1 << k, m = sh.usable_rows / 4;
        const Fr zero = {{0, 0, 0, 0}}, one = host_fr::R1;
        fixed.assign(sh.num_fixed_total, std::vector<Fr>(n, zero));
        advice.assign(1, std::vector<Fr>(n, zero));
        for (size_t i = 0; i < ((size_t)1 << lb); ++i) fixed[sh.table_col][i] = host_fr::from_u64(i);
        uint64_t s = circuit_seed;
        for (size_t j = 0; j < m; ++j) {
            Fr a = (j % 3 == 0) ? host_fr::from_u64(sm(s) & (((uint64_t)1 << lb) - 1)) : draw_fr(s);
            Fr b = draw_fr(s), c = draw_fr(s);
            if (j == 1) b = advice[0][1];
            advice[0][4 * j] = a;
            advice[0][4 * j + 1] = b;
            advice[0][4 * j + 2] = c;
            advice[0][4 * j + 3] = host_fr::add(a, host_fr::mul(b, c));
            fixed[sh.first_q_enable_col][4 * j] = one;
            if (j % 3 == 0) fixed[sh.q_lookup_col][4 * j] = one;
        }
        copies = {1, 1, 1, 5};
        for (uint32_t t = 0; t < 8 && t < m; ++t) {
            fixed[sh.first_constant_col][t] = advice[0][4 * t + 2];
            copies.insert(copies.end(), {0u, t, 1u, 4 * t + 2});
        }
        toxic = host_fr::from_u64(0x5eed5eed5eedULL);
        repr = host_fr::from_u64(0x1234567890abcdefULL);
    }
};

template <class F>
static double median_ms(F prove) {
    for (int i = 0; i < 2; ++i) prove();
    std::vector<double> ms;
    for (int i = 0; i < 7; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        prove();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    return ms[3];
}
static void time_proofs(Backend &be, const plonk::ProvingKey &pk, const SmallCircuit &circ, uint32_t k) {
    const size_t bytes = sizeof(Fr) << k;
    void *d_adv = nullptr;
    check(h2hip_malloc(be.raw(), bytes, &d_adv));
    check(h2hip_upload(be.raw(), d_adv, circ.advice[0].data(), bytes));
    const void *adv[1] = {d_adv};
    uint8_t seed[32];
    h2hip_rng_seed_from_u64(0, seed);
    std::vector<uint8_t> proof(32 * (size_t)(pk.shape().num_commitments + pk.shape().num_evals)), via_callbacks;
    const double builtin = median_ms([&] {
        h2hip_chacha_rng rng;
        h2hip_chacha_rng_init(&rng, seed, 12);
        size_t len = 0;
        check(h2hip_plonk_create_proof(be.raw(), pk.raw(), adv, 1, nullptr, nullptr, h2hip_chacha_rng_fill, &rng, proof.data(), proof.size(), &len, nullptr));
    });
    const double native = median_ms([&] {
        h2hip_chacha_rng rng;
        h2hip_chacha_rng_init(&rng, seed, 12);
        NativeBlake2b t(true);
        plonk::detail::TranscriptBridge bridge{&t, nullptr};
        const h2hip_transcript cb = bridge.callbacks();
        check(h2hip_plonk_create_proof_transcript(be.raw(), pk.raw(), adv, 1, nullptr, nullptr, h2hip_chacha_rng_fill, &rng, nullptr, &cb, nullptr));
        via_callbacks.swap(t.proof);
    });
    check(h2hip_free(be.raw(), d_adv));
    if (via_callbacks != proof) throw Error(-1, "--time: the two entries' bytes differ");
    printf("{\"k\": %u, \"builtin_ms\": %.3f, \"native_transcript_ms\": %.3f}\n", k, builtin, native);
}

int main(int argc, char **argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 10;
    const bool dump = argc > 2 && std::string(argv[2]) == "--dump-proof";
    try {
        Backend be(0);
        SmallCircuit circ(k, 99);
        poly::kzg::ParamsKZG params = poly::kzg::ParamsKZG::setup(be, k, circ.toxic, k >= 10);
        plonk::ProvingKey pk(be, circ.bp, params, circ.fixed, circ.copies);
        pk.set_transcript_repr(circ.repr);
        if (argc > 2 && std::string(argv[2]) == "--time") {
            time_proofs(be, pk, circ, k);
            return 0;
        }
        NativeBlake2b t1(true);
        {
            StreamRng rng{7};
            plonk::create_proof_with_transcript(be, pk, circ.advice, {}, rng, t1);
        }
        if (dump) {
            for (uint8_t c : t1.proof) printf("%02x", c);
            printf("\n");
            return 0;
        }
        StreamRng rng_b{7};
        const std::vector<uint8_t> builtin = plonk::create_proof(be, pk, circ.advice, {}, rng_b);
        if (t1.proof != builtin) throw Error(-1, "the native Blake2b transcript's bytes differ from the built-in entry's");
        std::vector<G1Affine> g = params.get_g().download();
        uint8_t g2[128], s_g2[128];
        poly::kzg::ParamsKZG::g2_pair(be, circ.toxic, g2, s_g2);
        if (!plonk::verify_proof(pk, circ.bp, circ.repr, g[0], g2, s_g2, {}, t1.proof)) throw Error(-1, "the built-in verifier rejects the proof");
        // an encoding of the caller's own: the library never sees the bytes
        NativeBlake2b t2(false);
        StreamRng rng_c{7};
        plonk::create_proof_with_transcript(be, pk, circ.advice, {}, rng_c, t2);
        if (t2.proof.size() <= builtin.size()) throw Error(-1, "uncompressed points take 64 bytes");
        if (plonk::verify_proof(pk, circ.bp, circ.repr, g[0], g2, s_g2, {}, t2.proof)) throw Error(-1, "the built-in verifier accepted another encoding");
        G1Affine acc[2];
        NativeBlake2b r2(false);
        r2.proof = t2.proof;
        if (!plonk::verify_proof_with_transcript(pk, circ.bp, circ.repr, g[0], g2, s_g2, {}, r2, acc) || r2.pos != r2.proof.size())
            throw Error(-1, "verify_proof_with_transcript rejects the proof");
        {   // the accumulator: e(W', s_g2) * e(-outer, g2) == 1
            G1Affine pts[2] = {acc[0], acc[1]};
            memcpy(pts[1].y.l, Q_MOD, 32);
            unsigned __int128 br = 0;
            for (int i = 0; i < 4; ++i) {
                unsigned __int128 d = (unsigned __int128)pts[1].y.l[i] - acc[1].y.l[i] - br;
                pts[1].y.l[i] = (uint64_t)d;
                br = (d >> 64) & 1;
            }
            uint8_t g2s[256];
            memcpy(g2s, s_g2, 128);
            memcpy(g2s + 128, g2, 128);
            int one = 0;
            check(h2hip_pairing_check(pts, g2s, 2, &one));
            if (!one) throw Error(-1, "the accumulator does not satisfy the pairing equation");
        }
        NativeBlake2b r3(false);
        r3.proof = t2.proof;
        r3.proof[r3.proof.size() - 130] ^= 1;   // the last evaluation
        if (plonk::verify_proof_with_transcript(pk, circ.bp, circ.repr, g[0], g2, s_g2, {}, r3)) throw Error(-1, "a changed evaluation was accepted");
        // a transcript that throws: the exception comes back, the error names the call, the key proves the same bytes afterwards
        NativeBlake2b t3(true);
        t3.fail_at_point = 4;
        bool thrown = false;
        try {
            StreamRng rng_d{7};
            plonk::create_proof_with_transcript(be, pk, circ.advice, {}, rng_d, t3);
        } catch (const std::runtime_error &e) {
            thrown = std::string(e.what()) == "the caller's transcript gave up" && std::string(h2hip_last_error()).find("write_point #4 ") != std::string::npos;
        }
        if (!thrown) throw Error(-1, "the transcript's exception did not come back (or the error does not name write_point #4)");
        StreamRng rng_e{7};
        if (plonk::create_proof(be, pk, circ.advice, {}, rng_e) != builtin) throw Error(-1, "the key did not survive an aborted proof");
        printf("transcript selftest OK (k=%u)\n", k);
        return 0;
    } catch (const Error &e) {
        fprintf(stderr, "transcript selftest FAILED: %s (code %d)\n", e.what(), e.code);
        return 1;
    }
}
