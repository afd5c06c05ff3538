// Poseidon permutation batches.
#include "internal.h"
#include "fr29.cuh"
#include "fq29.cuh"
#include "quad29.cuh"

namespace h2 {

// ------------------------------------------------------------------ K8: Poseidon permutation batches
// One lane per instance, textbook rounds (ARK, x^5, MDS) with the caller's spec — algebraically equal to
// halo2-base's optimised PoseidonState::permutation (reference halo2-base/src/poseidon/hasher/state.rs:35-83,
// absorb rule :124-160: inputs added to s[1..], a padding 1 after the last input when fewer than RATE).
// One lane per permutation, state in the unsaturated R' = 2^261 domain for the whole permutation (converted on entry and
// exit: 2T of the ~400 products): the S-box is two squarings and a product on lazy sums, and an MDS row is ONE dual...
// T-fold product with a single Montgomery reduction (f29_dot) instead of T products and T reductions.  rc / mds arrive
// pre-converted (R' form, packed 8 x 32 bit) from h2hip_poseidon_set_spec.
// The round loop: ARK, x^5 (every lane in the full rounds, lane 0 in the partial ones), MDS.  In: s[k] N, value < 2.2 r (a permutation's output
// plus one absorbed element); after ARK lazy, < 3.2 r, limbs <= 2^30; x^5 N, < 1.03 r; an MDS row sum_b X_a*X_b <= 5 * 1.01 * 3.2 -> < 1.1 r.
// It is TEXT, expanded once in poseidon_permute_kernel and once in poseidon_permute_state (below, which everything else calls): with the
// kernel calling the function, the compiler emits a different t = 3 kernel (1.5 % more multiplier instructions) and
// h2hip_poseidon_permute_batch_dev measured 2.5 % slower at 2^20 states and 10 - 14 % slower on the lone waves of narrow batches (MI355X, three
// alternating runs each).  Expanded in place, the kernel's code is byte for byte what it was before the body was shared.
#define H2_POSEIDON_ROUNDS(T, s, rc, mds, r_f, r_p) \
    const uint32_t half = r_f / 2; \
    for (uint32_t r = 0; r < r_f + r_p; ++r) { \
        const bool full = r < half || r >= half + r_p; \
_Pragma("unroll") \
        for (int k = 0; k < T; ++k) { \
            Fr29 v = f29_add(s[k], f29_split<R29P>(rc[r * T + k])); \
            if (full || k == 0) { \
                Fr29 v2 = f29_sqr(v); \
                v = f29_mul(f29_sqr(v2), v); \
            } else { \
                v = f29_norm(v); \
            } \
            s[k] = v; \
        } \
        Fr29 o[T]; \
_Pragma("unroll") \
        for (int a = 0; a < T; ++a) { \
            Fr29 row[T]; \
_Pragma("unroll") \
            for (int b = 0; b < T; ++b) row[b] = f29_split<R29P>(mds[a * T + b]); \
            o[a] = f29_dot<T>(row, s); \
        } \
_Pragma("unroll") \
        for (int k = 0; k < T; ++k) s[k] = o[k]; \
    }
// The permutation of a state held by ONE lane (the sponge, the wide tree levels).  In: s N, value < 2.2 r.  Out: N, < 1.1 r.
template <int T>
__device__ __forceinline__ void poseidon_permute_state(Fr29 (&s)[T], const Fr *__restrict__ rc, const Fr *__restrict__ mds, uint32_t r_f, uint32_t r_p) {
    H2_POSEIDON_ROUNDS(T, s, rc, mds, r_f, r_p)
}

template <int T>
__global__ __launch_bounds__(256) void poseidon_permute_kernel(Fr *__restrict__ states, const Fr *__restrict__ inputs, uint32_t num_inputs,
                                                               size_t n, const Fr *__restrict__ rc, const Fr *__restrict__ mds, uint32_t r_f,
                                                               uint32_t r_p) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr29 s[T];
#pragma unroll
    for (int k = 0; k < T; ++k) s[k] = fr29_from_sat(states[i * T + k]);
#pragma unroll
    for (int k = 0; k < T - 1; ++k) {
        if ((uint32_t)k < num_inputs) s[k + 1] = f29_norm(f29_add(s[k + 1], fr29_from_sat(inputs[i * num_inputs + k])));
        else if ((uint32_t)k == num_inputs) s[k + 1] = f29_norm(f29_add(s[k + 1], Fr29::one()));
    }
    H2_POSEIDON_ROUNDS(T, s, rc, mds, r_f, r_p)
#pragma unroll
    for (int k = 0; k < T; ++k) states[i * T + k] = fr29_to_sat(s[k]);
}

// ------------------------------------------------------------------ K8: the sponge H (PoseidonHasher::hash_fix_len_array / hash_var_len_array)
// H(m): s = [2^64, 0, ..], absorb m in chunks of RATE = T - 1 (a short chunk gets the padding 1 behind it), one more permutation of the
// empty chunk when len is a multiple of RATE, digest = s[1] — that is len / RATE + 1 permutations.  The spec buffer (set_spec) is
// [rc][mds][2^64], all in R' = 2^261 form.
struct PoseidonSpecDev {
    const Fr *rc, *mds, *init0;
    uint32_t r_f, r_p;
};
template <int T>
__device__ __forceinline__ void poseidon_init_state(Fr29 (&s)[T], const PoseidonSpecDev &sp) {
    s[0] = f29_split<R29P>(*sp.init0);
#pragma unroll
    for (int k = 1; k < T; ++k) s[k] = Fr29::zero();
}
// One lane per message; the state never leaves the lane's registers.  The lanes of a wave may hold different lengths: the block loop runs to
// the wave's longest message (one wave vote per block); a shorter lane keeps its digest aside when its own message ends.  A length above max_len is clamped and counted.
template <int T>
__global__ __launch_bounds__(256) void poseidon_hash_kernel(Fr *__restrict__ digests, const Fr *__restrict__ inputs, size_t max_len,
                                                            const uint32_t *__restrict__ lens, size_t n, PoseidonSpecDev sp, uint32_t *bad) {
    constexpr uint32_t RATE = T - 1;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    size_t len = 0;
    if (live) {
        len = max_len;
        if (lens) {
            const uint32_t l = lens[i];
            if (l > max_len) atomicAdd(bad, 1u);
            else len = l;
        }
    }
    const size_t nperm = live ? len / RATE + 1 : 0;
    const Fr *row = inputs + i * max_len;
    Fr29 s[T];
    poseidon_init_state<T>(s, sp);
    Fr29 digest = Fr29::zero();
    for (size_t b = 0; __any(b < nperm ? 1 : 0); ++b) {
        const size_t at = b * RATE;
        // branch-free absorb: element at + k of the message, the padding 1 right behind its end, nothing after that (or once b >= nperm)
#pragma unroll
        for (uint32_t k = 0; k < RATE; ++k) {
            const size_t idx = at + k;
            const bool data = b < nperm && idx < len, pad = b < nperm && idx == len;
            const Fr29 x = fr29_from_sat(*(data ? row + idx : sp.init0));   // (always a readable address)
            const Fr29 one = Fr29::one();
            Fr29 add;
#pragma unroll
            for (int i = 0; i < 9; ++i) add.l[i] = data ? x.l[i] : pad ? one.l[i] : 0u;
            s[k + 1] = f29_norm(f29_add(s[k + 1], add));
        }
        poseidon_permute_state<T>(s, sp.rc, sp.mds, sp.r_f, sp.r_p);   // (a lane whose message has ended keeps permuting: only its digest is kept)
        if (b + 1 == nperm) digest = s[1];
    }
    if (live) digests[i] = fr29_to_sat(digest);
}

// ------------------------------------------------------------------ K8: Merkle trees, node j = H([node 2j, node 2j+1])
// H of a pair: T = 3 absorbs the pair as one full chunk and permutes the empty chunk after it (two permutations), T = 5 absorbs it as a
// short chunk with the padding 1 at s[3] (one permutation).
template <int T>
__device__ __forceinline__ Fr29 poseidon_hash_pair_lane(const Fr29 &a, const Fr29 &b, const PoseidonSpecDev &sp) {
    Fr29 s[T];
    poseidon_init_state<T>(s, sp);
    s[1] = a;
    s[2] = b;
    if (T > 3) s[3] = Fr29::one();
    poseidon_permute_state<T>(s, sp.rc, sp.mds, sp.r_f, sp.r_p);
    if (T == 3) {
        s[1] = f29_norm(f29_add(s[1], Fr29::one()));
        poseidon_permute_state<T>(s, sp.rc, sp.mds, sp.r_f, sp.r_p);
    }
    return s[1];
}
// Wide levels: one lane per node of the level [w, 2w); the two children are adjacent (one 64-byte read).
template <int T>
__global__ __launch_bounds__(256) void poseidon_tree_level_kernel(Fr *__restrict__ nodes, size_t w, PoseidonSpecDev sp) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w) return;
    const size_t j = w + i;
    nodes[j] = fr29_to_sat(poseidon_hash_pair_lane<T>(fr29_from_sat(nodes[2 * j]), fr29_from_sat(nodes[2 * j + 1]), sp));
}

// Narrow levels: a level with fewer nodes than the machine has lanes costs a whole permutation's time however few nodes it has, and that time
// is the lane's own multiplier work.  So ONE state is spread over a group of G lanes — lane g holds s[g] — the way quad29.cuh spreads a
// point: a round is then one S-box (three products) and ONE MDS row (one f29_dot) per lane instead of T of each.  T = 3 uses a quad and
// fetches the other lanes' values with DPP quad_perm moves; T = 5 does not fit a quad and uses eight lanes with wave shuffles (45 per round
// against ~1300 multiplier instructions).  Lanes g >= T of a group mirror lane T - 1 (same loads, same bounds) and store nothing.
template <int T>
struct PoseidonGroup {
    static constexpr uint32_t G = T == 3 ? 4 : 8;
};
template <int T, int B>
__device__ __forceinline__ Fr29 poseidon_group_get(const Fr29 &v, uint32_t lane) {   // the value lane B of this lane's group holds
    constexpr uint32_t G = PoseidonGroup<T>::G;
    Fr29 r;
#ifdef H2_HIPEMU
    hipemu_shfl_words<9>(r.l, v.l, (lane & ~(G - 1)) | (uint32_t)B);   // CPU emulation: one rendezvous for nine limbs
#else
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        if (T == 3) r.l[i] = quad_perm_u32<(T == 3 ? B : 0) * 0x55>(v.l[i], lane);
        else r.l[i] = (uint32_t)__shfl((int)v.l[i], (int)((lane & ~(G - 1)) | (uint32_t)B));
    }
#endif
    return r;
}
// s: this lane's element (k = min(g, T - 1)), N, < 2.2 r; row: this lane's MDS row.  Called wave-uniformly.
template <int T>
__device__ __forceinline__ Fr29 poseidon_permute_group(Fr29 s, uint32_t k, uint32_t lane, const Fr29 (&row)[T], const PoseidonSpecDev &sp) {
    const uint32_t half = sp.r_f / 2;
    for (uint32_t r = 0; r < sp.r_f + sp.r_p; ++r) {
        const bool full = r < half || r >= half + sp.r_p;
        const Fr29 v = f29_add(s, f29_split<R29P>(sp.rc[r * T + k]));   // lazy: value < 3.2 r, limbs <= 2^30
        const Fr29 v5 = f29_mul(f29_sqr(f29_sqr(v)), v);                  // every lane (lane 0 needs it in every round): N, < 1.03 r
        const Fr29 lin = f29_norm(v);
        const bool sbox = full || k == 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) s.l[i] = sbox ? v5.l[i] : lin.l[i];
        Fr29 all[T];
        all[0] = poseidon_group_get<T, 0>(s, lane);
        all[1] = poseidon_group_get<T, 1>(s, lane);
        all[2] = poseidon_group_get<T, 2>(s, lane);
        if (T > 3) {
            all[T - 2] = poseidon_group_get<T, T - 2>(s, lane);
            all[T - 1] = poseidon_group_get<T, T - 1>(s, lane);
        }
        s = f29_dot<T>(row, all);   // < 1.1 r
    }
    return s;
}
// node j = H([node 2j, node 2j+1]) on a group; c = the child this lane loads (lane 1: the left one, lane 2: the right one; every lane holds a
// valid one).  Returns the digest in lane 1 of the group (R' form).
template <int T>
__device__ __forceinline__ Fr29 poseidon_hash_pair_group(const Fr &c, uint32_t k, uint32_t lane, const Fr29 (&row)[T], const PoseidonSpecDev &sp) {
    const Fr29 cv = fr29_from_sat(c), init0 = f29_split<R29P>(*sp.init0), one = Fr29::one(), zero = Fr29::zero();
    Fr29 s;
#pragma unroll
    for (int i = 0; i < 9; ++i) s.l[i] = k == 0 ? init0.l[i] : k <= 2 ? cv.l[i] : (T > 3 && k == 3) ? one.l[i] : zero.l[i];
    s = poseidon_permute_group<T>(s, k, lane, row, sp);
    if (T == 3) {
        const Fr29 p = f29_norm(f29_add(s, one));
#pragma unroll
        for (int i = 0; i < 9; ++i) s.l[i] = k == 1 ? p.l[i] : s.l[i];
        s = poseidon_permute_group<T>(s, k, lane, row, sp);
    }
    return s;
}
template <int T>
__device__ __forceinline__ void poseidon_group_row(Fr29 (&row)[T], uint32_t k, const PoseidonSpecDev &sp) {
#pragma unroll
    for (int b = 0; b < T; ++b) row[b] = f29_split<R29P>(sp.mds[k * T + b]);
}
// Middle levels: one group per node of the level [w, 2w), one launch per level.  Whole groups past the level's end redo its last node (the
// cross-lane moves need every lane) and store nothing.
template <int T>
__global__ __launch_bounds__(256) void poseidon_tree_group_kernel(Fr *__restrict__ nodes, size_t w, PoseidonSpecDev sp) {
    constexpr uint32_t G = PoseidonGroup<T>::G;
    const uint32_t lane = threadIdx.x & 63u, g = threadIdx.x & (G - 1), k = g < T ? g : T - 1;
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const size_t j = w + (i < w ? i : w - 1);
    Fr29 row[T];
    poseidon_group_row<T>(row, k, sp);
    const Fr29 d = poseidon_hash_pair_group<T>(nodes[2 * j + (k == 2 ? 1 : 0)], k, lane, row, sp);
    const Fr out = fr29_to_sat(d);
    if (i < w && g == 1) nodes[j] = out;
}
// The top of the tree: every level from w0 <= POSEIDON_TOP_WIDTH<T> nodes down to the root in ONE launch of one workgroup, one group per
// node, the levels' nodes handed down through LDS (heap layout, like the array itself).
template <int T>
__global__ __launch_bounds__(256) void poseidon_tree_top_kernel(Fr *__restrict__ nodes, uint32_t w0, PoseidonSpecDev sp) {
    constexpr uint32_t G = PoseidonGroup<T>::G, W = 256 / G;
    __shared__ Fr heap[2 * W];
    const uint32_t lane = threadIdx.x & 63u, g = threadIdx.x & (G - 1), k = g < T ? g : T - 1, i = threadIdx.x / G;
    Fr29 row[T];
    poseidon_group_row<T>(row, k, sp);
    for (uint32_t w = w0; w >= 1; w >>= 1) {
        const uint32_t j = w + (i < w ? i : w - 1), c = 2 * j + (k == 2 ? 1 : 0);
        const Fr child = w == w0 ? nodes[c] : heap[c];
        const Fr29 d = poseidon_hash_pair_group<T>(child, k, lane, row, sp);
        const Fr out = fr29_to_sat(d);
        if (i < w && g == 1) {
            heap[j] = out;
            nodes[j] = out;
        }
        __syncthreads();
    }
}
// Switch-over widths (nodes per level), measured on MI355X — DESIGN.md §3 "Poseidon hashing" has the table.  A level of up to
// POSEIDON_GROUP_MAX_WIDTH<T> nodes runs one group per node, wider levels one lane per node.  t = 3: at 2^14 nodes the quads fill every SIMD
// with one wave and a level costs 0.31 ms against 0.55 ms one lane per node; at 2^15 the two forms tie, at 2^16 the groups lose 0.5 ms.
// t = 5: a group's round is 2.9 times shorter than a lane's, so groups still win at 2^15 nodes (four waves per SIMD: 0.66 against 0.78 ms)
// and lose from 2^16 on.  The last levels, from 256 / G nodes (one workgroup of groups) down to the root, share one launch.
template <int T>
constexpr size_t POSEIDON_GROUP_MAX_WIDTH = T == 3 ? (size_t)1 << 14 : (size_t)1 << 15;
template <int T>
constexpr uint32_t POSEIDON_TOP_WIDTH = 256 / PoseidonGroup<T>::G;

template <int T>
static void poseidon_tree_launch(h2hip_ctx *ctx, Fr *nodes, uint32_t log_leaves, const PoseidonSpecDev &sp) {
    constexpr uint32_t G = PoseidonGroup<T>::G;
    for (uint32_t lv = log_leaves; lv-- > 0;) {
        const size_t w = (size_t)1 << lv;
        if (w <= POSEIDON_TOP_WIDTH<T>) {
            prof_begin(ctx, "poseidon_tree_top_kernel");
            hipLaunchKernelGGL(poseidon_tree_top_kernel<T>, dim3(1), dim3(256), 0, ctx->stream, nodes, (uint32_t)w, sp);
            prof_end(ctx);
            return;
        }
        if (w <= POSEIDON_GROUP_MAX_WIDTH<T>) {
            prof_begin(ctx, "poseidon_tree_group_kernel");
            hipLaunchKernelGGL(poseidon_tree_group_kernel<T>, dim3((uint32_t)((w * G + 255) / 256)), dim3(256), 0, ctx->stream, nodes, w, sp);
        } else {
            prof_begin(ctx, "poseidon_tree_level_kernel");
            hipLaunchKernelGGL(poseidon_tree_level_kernel<T>, dim3((uint32_t)((w + 255) / 256)), dim3(256), 0, ctx->stream, nodes, w, sp);
        }
        prof_end(ctx);
    }
}

// ------------------------------------------------------------------ the spec from (t, r_f, r_p) alone (host)
// The Poseidon paper's parameter generation (Grassi et al., "Poseidon: A New Hash Function for Zero-Knowledge Proof Systems", appendix F /
// the authors' generate_parameters_grain script): an 80-bit Grain LFSR seeded with the instance's description, 160 discarded clocks, output
// bits taken in pairs (the second bit of a pair counts when the first is 1).  Round constants are 254-bit draws with rejection of values >= r;
// the Cauchy MDS matrix 1 / (x_i + y_j) takes its x and y as draws reduced mod r, the first such matrix (pse-poseidon's "secure MDS 0").
struct PoseidonGrain {
    uint8_t st[80];
    uint32_t at = 0;   // st is a ring: bit i of the register is st[(at + i) % 80]
    PoseidonGrain(uint32_t t, uint32_t r_f, uint32_t r_p) {
        uint32_t n = 0;
        auto push = [&](uint32_t v, uint32_t width) {
            for (uint32_t i = 0; i < width; ++i) st[n++] = (v >> (width - 1 - i)) & 1u;
        };
        push(1, 2);      // a prime field
        push(0, 4);      // S-box x^alpha
        push(254, 12);   // bits of r
        push(t, 12);
        push(r_f, 10);
        push(r_p, 10);
        while (n < 80) st[n++] = 1;
        for (int i = 0; i < 160; ++i) clock();
    }
    uint32_t bit_at(uint32_t i) const { return st[(at + i) % 80]; }
    uint32_t clock() {
        const uint32_t nb = bit_at(62) ^ bit_at(51) ^ bit_at(38) ^ bit_at(23) ^ bit_at(13) ^ bit_at(0);
        st[at] = (uint8_t)nb;   // the slot of the bit shifted out becomes the new last bit
        at = (at + 1) % 80;
        return nb;
    }
    uint32_t next_bit() {
        for (;;) {
            const uint32_t a = clock(), b = clock();
            if (a) return b;
        }
    }
    void raw254(uint32_t (&v)[8]) {   // 254 bits, most significant first
        for (int i = 0; i < 8; ++i) v[i] = 0;
        for (int i = 253; i >= 0; --i) v[i >> 5] |= next_bit() << (i & 31);
    }
};
static bool poseidon_lt_r(const uint32_t (&v)[8]) {
    for (int i = 7; i >= 0; --i)
        if (v[i] != FrP::m(i)) return v[i] < FrP::m(i);
    return false;
}
static Fr poseidon_draw(PoseidonGrain &g, bool reject) {   // a field element in Montgomery form
    uint32_t v[8];
    for (;;) {
        g.raw254(v);
        if (poseidon_lt_r(v)) break;
        if (reject) continue;
        uint64_t borrow = 0;   // v < 2^254 < 2 r: one subtraction reduces it
        for (int i = 0; i < 8; ++i) {
            const uint64_t d = (uint64_t)v[i] - FrP::m(i) - borrow;
            v[i] = (uint32_t)d;
            borrow = (d >> 32) & 1u;
        }
        break;
    }
    Fr f;
    for (int i = 0; i < 8; ++i) f.l[i] = v[i];
    return fe_to_mont(f);
}
static bool poseidon_spec_ok(uint32_t t, uint32_t r_f, uint32_t r_p) {
    return (t == 3 || t == 5) && r_f >= 2 && (r_f % 2) == 0 && r_f <= 16 && r_p <= 256;
}

}  // namespace h2

using namespace h2;

extern "C" {

// ------------------------------------------------------------------ K8 Poseidon
int h2hip_poseidon_set_spec(h2hip_ctx *ctx, uint32_t t, uint32_t r_f, uint32_t r_p, const void *round_constants, const void *mds) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && round_constants && mds, "NULL argument");
    H2_REQUIRE(t == 3 || t == 5, "state width t must be 3 or 5");
    H2_REQUIRE(poseidon_spec_ok(t, r_f, r_p), "round numbers out of range");
    size_t nrc = (size_t)(r_f + r_p) * t, nm = (size_t)t * t;
    Fr *buf = nullptr;
    // [rc][mds][2^64: the sponge's initial s[0]][one Fr-sized slot whose first word counts the over-long messages of a hash_batch call]
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_POSEIDON, sizeof(Fr) * (nrc + nm + 2), (void **)&buf));
    // the kernel multiplies in the unsaturated R' = 2^261 domain: store c * 2^261 (packed 8 x 32 bit) once here
    std::vector<Fr> conv(nrc + nm + 1);
    for (size_t j = 0; j < nrc + nm; ++j) {
        Fr c;
        memcpy(&c, (const char *)(j < nrc ? round_constants : mds) + sizeof(Fr) * (j < nrc ? j : j - nrc), sizeof(Fr));
        conv[j] = f29_pack_canonical<FrP>(fr29_from_sat(c));
    }
    Fr two64;
    for (int i = 0; i < 8; ++i) two64.l[i] = i == 2 ? 1u : 0u;
    conv[nrc + nm] = f29_pack_canonical<FrP>(fr29_from_sat(fe_to_mont(two64)));
    H2_HIPCHK(hipMemcpyAsync(buf, conv.data(), sizeof(Fr) * (nrc + nm + 1), hipMemcpyHostToDevice, ctx->stream));
    H2_HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->pos_t = t;
    ctx->pos_rf = r_f;
    ctx->pos_rp = r_p;
    return H2HIP_OK;
}
int h2hip_poseidon_permute_batch_dev(h2hip_ctx *ctx, void *states, const void *inputs, uint32_t num_inputs, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (n == 0 || states), "NULL argument");
    H2_REQUIRE(ctx->pos_t != 0, "call h2hip_poseidon_set_spec first");
    H2_REQUIRE(num_inputs < ctx->pos_t, "num_inputs must be <= RATE = t-1");
    H2_REQUIRE(num_inputs == 0 || inputs || n == 0, "inputs is NULL");
    if (!n) return H2HIP_OK;
    const Fr *rc = (const Fr *)ctx->ws[h2hip_ctx::WS_POSEIDON].p;
    const Fr *mds = rc + (size_t)(ctx->pos_rf + ctx->pos_rp) * ctx->pos_t;
    dim3 g((uint32_t)((n + 255) / 256)), blk(256);
    prof_begin(ctx, "poseidon_permute_kernel");
    if (ctx->pos_t == 3)
        hipLaunchKernelGGL(poseidon_permute_kernel<3>, g, blk, 0, ctx->stream, (Fr *)states, (const Fr *)inputs, num_inputs, n, rc, mds, ctx->pos_rf,
                           ctx->pos_rp);
    else
        hipLaunchKernelGGL(poseidon_permute_kernel<5>, g, blk, 0, ctx->stream, (Fr *)states, (const Fr *)inputs, num_inputs, n, rc, mds, ctx->pos_rf,
                           ctx->pos_rp);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

static PoseidonSpecDev poseidon_spec_dev(const h2hip_ctx *ctx) {
    const Fr *rc = (const Fr *)ctx->ws[h2hip_ctx::WS_POSEIDON].p;
    const Fr *mds = rc + (size_t)(ctx->pos_rf + ctx->pos_rp) * ctx->pos_t;
    return PoseidonSpecDev{rc, mds, mds + (size_t)ctx->pos_t * ctx->pos_t, ctx->pos_rf, ctx->pos_rp};
}
int h2hip_poseidon_hash_batch_dev(h2hip_ctx *ctx, void *digests_dev, const void *inputs_dev, size_t max_len, const uint32_t *lens_dev, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (n == 0 || digests_dev), "NULL argument");
    H2_REQUIRE(ctx->pos_t != 0, "call h2hip_poseidon_set_spec first");
    H2_REQUIRE(max_len == 0 || inputs_dev || n == 0, "inputs_dev is NULL");
    H2_REQUIRE(n <= ((size_t)1 << 39), "too many messages");
    if (!n) return H2HIP_OK;
    const PoseidonSpecDev sp = poseidon_spec_dev(ctx);
    uint32_t *bad = (uint32_t *)(sp.init0 + 1);
    if (lens_dev) H2_HIPCHK(hipMemsetAsync(bad, 0, sizeof(uint32_t), ctx->stream));
    dim3 g((uint32_t)((n + 255) / 256)), blk(256);
    prof_begin(ctx, "poseidon_hash_kernel");
    if (ctx->pos_t == 3)
        hipLaunchKernelGGL(poseidon_hash_kernel<3>, g, blk, 0, ctx->stream, (Fr *)digests_dev, (const Fr *)inputs_dev, max_len, lens_dev, n, sp, bad);
    else
        hipLaunchKernelGGL(poseidon_hash_kernel<5>, g, blk, 0, ctx->stream, (Fr *)digests_dev, (const Fr *)inputs_dev, max_len, lens_dev, n, sp, bad);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    if (lens_dev) {   // the call's only host synchronisation
        uint32_t nbad = 0;
        H2_CHK(sync_results(ctx, &nbad, bad, sizeof(uint32_t)));
        if (nbad) {
            set_error("%s: invalid argument: %u of %zu messages have a length above max_len = %zu", __func__, nbad, n, max_len);
            return H2HIP_ERR_INVALID;
        }
    }
    return H2HIP_OK;
}
int h2hip_poseidon_merkle_tree_dev(h2hip_ctx *ctx, void *nodes_dev, const void *leaves_dev, uint32_t log_leaves) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && nodes_dev, "NULL argument");
    H2_REQUIRE(ctx->pos_t != 0, "call h2hip_poseidon_set_spec first");
    H2_REQUIRE(log_leaves <= 30, "log_leaves must be <= 30");
    Fr *nodes = (Fr *)nodes_dev;
    const size_t leaves = (size_t)1 << log_leaves;
    if (leaves_dev && leaves_dev != (const void *)(nodes + leaves))
        H2_HIPCHK(hipMemcpyAsync(nodes + leaves, leaves_dev, sizeof(Fr) * leaves, hipMemcpyDeviceToDevice, ctx->stream));
    H2_HIPCHK(hipMemsetAsync(nodes, 0, sizeof(Fr), ctx->stream));
    const PoseidonSpecDev sp = poseidon_spec_dev(ctx);
    if (ctx->pos_t == 3) poseidon_tree_launch<3>(ctx, nodes, log_leaves, sp);
    else poseidon_tree_launch<5>(ctx, nodes, log_leaves, sp);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
int h2hip_poseidon_spec_generate(uint32_t t, uint32_t r_f, uint32_t r_p, void *round_constants_out, void *mds_out) {
    H2_REQUIRE(round_constants_out && mds_out, "NULL argument");
    H2_REQUIRE(t == 3 || t == 5, "state width t must be 3 or 5");
    H2_REQUIRE(poseidon_spec_ok(t, r_f, r_p), "round numbers out of range");
    PoseidonGrain g(t, r_f, r_p);
    const size_t nrc = (size_t)(r_f + r_p) * t;
    for (size_t j = 0; j < nrc; ++j) {
        const Fr c = poseidon_draw(g, true);
        memcpy((char *)round_constants_out + sizeof(Fr) * j, &c, sizeof(Fr));
    }
    Fr xs[5], ys[5];
    for (uint32_t i = 0; i < t; ++i) xs[i] = poseidon_draw(g, false);
    for (uint32_t i = 0; i < t; ++i) ys[i] = poseidon_draw(g, false);
    for (uint32_t i = 0; i < t; ++i)
        for (uint32_t j = 0; j < t; ++j) {
            const Fr m = fe_inv(fe_add(xs[i], ys[j]));
            memcpy((char *)mds_out + sizeof(Fr) * (i * t + j), &m, sizeof(Fr));
        }
    return H2HIP_OK;
}

}  // extern "C"
