// Pointwise F_r kernels around the MSM/NTT core: the "witness-column Montgomery mul"
// batches of halo2-base's GateInstructions (reference halo2-base/src/gates/flex_gate/mod.rs:158-277: add /
// sub / mul / mul_add on column values), the one-pass linear combination, batch inversion and the prefix / grand
// products.  (K6: quotient.hip, K7: poly_eval.hip, K8: poseidon.hip, the micro-benchmark probes: probes.hip.)
#include "internal.h"
#include "fr29.cuh"
#include "fq29.cuh"

namespace h2 {


enum { OP_ADD = 0, OP_SUB = 1, OP_MUL = 2 };

template <int OP>
__global__ __launch_bounds__(256) void fr_binop_kernel(Fr *__restrict__ out, const Fr *__restrict__ a, const Fr *__restrict__ b, size_t n) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        Fr x = a[i], y = b[i];
        out[i] = OP == OP_ADD ? fe_add(x, y) : OP == OP_SUB ? fe_sub(x, y) : fe_mul(x, y);
    }
}

// out[i] = a[i]*b[i] + c[i]   (GateInstructions::mul_add, flex_gate/mod.rs:262-277)
__global__ __launch_bounds__(256) void fr_mul_add_kernel(Fr *__restrict__ out, const Fr *__restrict__ a, const Fr *__restrict__ b,
                                                         const Fr *__restrict__ c, size_t n) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = fe_add(fe_mul(a[i], b[i]), c[i]);
}

// y[i] = y[i]*s + a*x[i]: the polynomial linear combinations of the multiopen argument (Polynomial * F, += of scaled
// polynomials in SHPLONK's rotation-set quotients); x may be null (pure scaling)
__global__ __launch_bounds__(256) void fr_axpby_kernel(Fr *__restrict__ y, Fr s, bool scale_y, const Fr *__restrict__ x, Fr a, size_t n) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        Fr v = y[i];
        if (scale_y) v = fe_mul(v, s);
        if (x) v = fe_add(v, fe_mul(a, x[i]));
        y[i] = v;
    }
}

// out[i] = (accumulate ? out[i] : 0) + sum_j c_j * p_j[i], up to LINCOMB_MAX polynomials per pass: the multiopen argument's sum_j y^j P_j(X)
// and its linearisation in ONE read of every operand instead of an axpy (read y, read x, write y) per term.  The data stays in its
// saturated Montgomery form x*2^256 as a 9x29-bit integer (f29_split: no multiplication), the coefficients come in the 2^261 form, so a
// product c'*x*2^-261 is again x-form; five products share one Montgomery reduction (f29_dot).
constexpr uint32_t LINCOMB_MAX = 15;
struct LinCombArgs {
    const Fr *p[LINCOMB_MAX];
    Fr29 c[LINCOMB_MAX];   // coefficient * 2^261, normalised, < 1.01 r
    uint32_t count, accumulate;
};
__global__ __launch_bounds__(256) void fr_lincomb_kernel(Fr *out, LinCombArgs a, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        Fr29 tot = a.accumulate ? f29_split<R29P>(out[i]) : Fr29::zero();
        for (uint32_t j0 = 0; j0 < a.count; j0 += 5) {
            Fr29 x[5], c[5];
#pragma unroll
            for (uint32_t t = 0; t < 5; ++t) {
                const bool live = j0 + t < a.count;
                x[t] = live ? f29_split<R29P>(a.p[j0 + t][i]) : Fr29::zero();
                c[t] = live ? a.c[j0 + t] : Fr29::zero();
            }
            tot = f29_add(tot, f29_dot<5>(x, c));   // lazy: at most 1 + 3 normalised terms, limbs < 2^31
        }
        out[i] = f29_pack_canonical<FrP>(f29_weak_reduce(f29_norm(tot)));   // < r + 3 * 1.03 r -> < 2 r -> canonical
    }
}

// ------------------------------------------------------------------ K4: BatchInvert (0 -> 0)
// Montgomery's trick over strided runs: lane t owns a[t], a[t+T], a[t+2T], ... (coalesced), one inversion
// (division steps, modinv.cuh) per lane.  [UPSTREAM ff::BatchInvert / halo2 batch_invert_assigned; denominators come from
// reference halo2-base/src/gates/flex_gate/mod.rs:677-681,791-795]
// (r06) src -> dst: out of place when they differ — the grand products invert their denominators straight out of the factor array instead of
// copying it first (a 32 MiB device copy per proof at k = 19, on the critical path between the factors and the prefix products).  In place
// (h2hip_fr_batch_invert_dev) src == dst, so neither carries __restrict__ (finding 4): a lane reads src[i] before it writes dst[i].
__global__ __launch_bounds__(256) void fr_batch_invert_kernel(const Fr *src, Fr *dst, Fr *__restrict__ scratch, size_t n) {
    const size_t T = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    Fr acc = Fr::one();
    size_t last = t;
    for (size_t i = t; i < n; i += T) {
        Fr v = src[i];
        scratch[i] = acc;
        if (!v.is_zero()) acc = fe_mul(acc, v);
        last = i;
    }
    Fr inv = fe_inv(acc);
    for (size_t i = last;; i -= T) {
        Fr v = src[i];
        if (!v.is_zero()) {
            dst[i] = fe_mul(inv, scratch[i]);
            inv = fe_mul(inv, v);
        } else if (dst != src) {
            dst[i] = v;   // 0 -> 0
        }
        if (i < T) break;
    }
}

// (r05 built the same kernel on unsaturated 9 x 29-bit limbs with the loads issued four elements ahead: bit-exact, 5 - 8 % slower alone — a lane's chain is
// the division steps, not the products — and equal inside proofs, where this kernel's 0.4 ms are the transforms running beside it: 0.129 ms alone for 2^20
// elements.  profiles/r05_invert29_ab.log; removed.)

// ------------------------------------------------------------------ K5: prefix product (grand product core)
// inclusive prefix product over tiles of 256 lanes x SCAN_J consecutive elements
constexpr uint32_t SCAN_J = 8;
// (blockIdx.y = segment: independent products over equal-length segments `seg_stride` elements apart go through the same three launches)
__global__ __launch_bounds__(256) void fr_prefix_prod_tile_kernel(const Fr *__restrict__ in, Fr *__restrict__ out, Fr *__restrict__ tile_prod,
                                                                  size_t n, size_t seg_stride) {
    __shared__ Fr sh[256];
    in += (size_t)blockIdx.y * seg_stride;
    out += (size_t)blockIdx.y * seg_stride;
    tile_prod += (size_t)blockIdx.y * gridDim.x;
    const uint32_t tid = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * 256 + tid) * SCAN_J;
    Fr acc = Fr::one();
    for (uint32_t k = 0; k < SCAN_J; ++k)
        if (base + k < n) acc = fe_mul(acc, in[base + k]);
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        Fr o = Fr::one();
        if (tid >= d) o = sh[tid - d];
        __syncthreads();
        if (tid >= d) sh[tid] = fe_mul(sh[tid], o);
        __syncthreads();
    }
    Fr run = tid ? sh[tid - 1] : Fr::one();   // exclusive prefix of this lane inside the tile
    for (uint32_t k = 0; k < SCAN_J; ++k)
        if (base + k < n) {
            run = fe_mul(run, in[base + k]);
            out[base + k] = run;
        }
    if (tid == 255) tile_prod[blockIdx.x] = sh[255];
}
// exclusive prefix product of the tile totals, one workgroup (tiles <= 1024 * per)
__global__ __launch_bounds__(1024) void fr_prefix_prod_sums_kernel(Fr *__restrict__ tile_prod, uint32_t ntiles) {
    __shared__ Fr sh[1024];
    tile_prod += (size_t)blockIdx.x * ntiles;   // one workgroup per segment
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ntiles + 1023) / 1024, lo = tid * per, hi = lo + per < ntiles ? lo + per : ntiles;
    Fr acc = Fr::one();
    for (uint32_t k = lo; k < hi; ++k) acc = fe_mul(acc, tile_prod[k]);
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        Fr o = Fr::one();
        if (tid >= d) o = sh[tid - d];
        __syncthreads();
        if (tid >= d) sh[tid] = fe_mul(sh[tid], o);
        __syncthreads();
    }
    Fr run = tid ? sh[tid - 1] : Fr::one();
    for (uint32_t k = lo; k < hi; ++k) {
        Fr t = tile_prod[k];
        tile_prod[k] = run;
        run = fe_mul(run, t);
    }
}
__global__ __launch_bounds__(256) void fr_prefix_prod_apply_kernel(Fr *__restrict__ out, const Fr *__restrict__ tile_excl, size_t n, size_t seg_stride) {
    const size_t base = ((size_t)blockIdx.x * 256 + threadIdx.x) * SCAN_J;
    if (blockIdx.x == 0) return;
    out += (size_t)blockIdx.y * seg_stride;
    Fr m = tile_excl[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
    for (uint32_t k = 0; k < SCAN_J; ++k)
        if (base + k < n) out[base + k] = fe_mul(out[base + k], m);
}
// z[0] = 1 (written by the host wrapper), t[i] = num[i] * den_inv[i]
__global__ __launch_bounds__(256) void fr_set_one_kernel(Fr *__restrict__ z) {
    if (threadIdx.x == 0 && blockIdx.x == 0) z[0] = Fr::one();
}
// several grand products at once: the factors num[g] * den_inv[g] of `segments` products of seg_len factors each, laid out for ONE
// (segmented) prefix product.  chained: [1, all factors] — the prefix product over the concatenation IS the chain z_i(0) = z_{i-1}(last);
// otherwise every segment gets its own leading 1: [1, factors of segment 0][1, factors of segment 1]...
__global__ __launch_bounds__(256) void fr_ratio_rows_kernel(Fr *__restrict__ r, const Fr *__restrict__ num, const Fr *__restrict__ den_inv, size_t total,
                                                            size_t seg_len, int chained) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const size_t seg = g / seg_len, i = g - seg * seg_len;
        const size_t dst = chained ? g + 1 : seg * (seg_len + 1) + i + 1;
        r[dst] = fe_mul(num[g], den_inv[g]);
        if (i == 0 && (!chained || seg == 0)) r[dst - 1] = Fr::one();
    }
}
// dst.p[y][i] = src[y * src_stride + i], i < len: rows of a resident matrix out to separately allocated columns (32 per launch)
struct RowPtrs {
    Fr *p[32];
};
__global__ __launch_bounds__(256) void fr_scatter_rows_kernel(RowPtrs dst, const Fr *__restrict__ src, size_t src_stride, size_t len) {
    Fr *__restrict__ d = dst.p[blockIdx.y];
    const Fr *__restrict__ sp = src + (size_t)blockIdx.y * src_stride;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) d[i] = sp[i];
}

}  // namespace h2

using namespace h2;

extern "C" {

static int binop(h2hip_ctx *ctx, int op, void *out, const void *a, const void *b, size_t n) {
    H2_REQUIRE(ctx && (n == 0 || (out && a && b)), "NULL argument");
    if (!n) return H2HIP_OK;
    dim3 g(grid_for(ctx, n)), blk(256);
    prof_begin(ctx, "fr_binop_kernel");
    if (op == OP_ADD) hipLaunchKernelGGL(fr_binop_kernel<OP_ADD>, g, blk, 0, ctx->stream, (Fr *)out, (const Fr *)a, (const Fr *)b, n);
    if (op == OP_SUB) hipLaunchKernelGGL(fr_binop_kernel<OP_SUB>, g, blk, 0, ctx->stream, (Fr *)out, (const Fr *)a, (const Fr *)b, n);
    if (op == OP_MUL) hipLaunchKernelGGL(fr_binop_kernel<OP_MUL>, g, blk, 0, ctx->stream, (Fr *)out, (const Fr *)a, (const Fr *)b, n);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
int h2hip_fr_add_batch_dev(h2hip_ctx *ctx, void *out, const void *a, const void *b, size_t n) {
    H2_DEVICE_GUARD(ctx); return binop(ctx, OP_ADD, out, a, b, n); }
int h2hip_fr_sub_batch_dev(h2hip_ctx *ctx, void *out, const void *a, const void *b, size_t n) {
    H2_DEVICE_GUARD(ctx); return binop(ctx, OP_SUB, out, a, b, n); }
int h2hip_fr_mul_batch_dev(h2hip_ctx *ctx, void *out, const void *a, const void *b, size_t n) {
    H2_DEVICE_GUARD(ctx); return binop(ctx, OP_MUL, out, a, b, n); }
int h2hip_fr_mul_add_batch_dev(h2hip_ctx *ctx, void *out, const void *a, const void *b, const void *c, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (n == 0 || (out && a && b && c)), "NULL argument");
    if (!n) return H2HIP_OK;
    prof_begin(ctx, "fr_mul_add_kernel");
    hipLaunchKernelGGL(fr_mul_add_kernel, dim3(grid_for(ctx, n)), dim3(256), 0, ctx->stream, (Fr *)out, (const Fr *)a, (const Fr *)b,
                       (const Fr *)c, n);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
int h2hip_fr_axpy_dev(h2hip_ctx *ctx, void *y, const void *a, const void *x, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && a && (n == 0 || (y && x)), "NULL argument");
    if (!n) return H2HIP_OK;
    Fr av;
    memcpy(&av, a, sizeof(Fr));
    prof_begin(ctx, "fr_axpby_kernel");
    hipLaunchKernelGGL(fr_axpby_kernel, dim3(grid_for(ctx, n)), dim3(256), 0, ctx->stream, (Fr *)y, Fr::one(), false, (const Fr *)x, av, n);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
// y[i] = s*y[i] + a*x[i]
int h2hip_fr_axpby_dev(h2hip_ctx *ctx, void *y, const void *s, const void *a, const void *x, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && a && s && (n == 0 || (y && x)), "NULL argument");
    if (!n) return H2HIP_OK;
    Fr av, sv;
    memcpy(&av, a, sizeof(Fr));
    memcpy(&sv, s, sizeof(Fr));
    prof_begin(ctx, "fr_axpby_kernel");
    hipLaunchKernelGGL(fr_axpby_kernel, dim3(grid_for(ctx, n)), dim3(256), 0, ctx->stream, (Fr *)y, sv, true, (const Fr *)x, av, n);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
int h2hip_fr_scale_dev(h2hip_ctx *ctx, void *y, const void *s, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && s && (n == 0 || y), "NULL argument");
    if (!n) return H2HIP_OK;
    Fr sv;
    memcpy(&sv, s, sizeof(Fr));
    prof_begin(ctx, "fr_axpby_kernel");
    hipLaunchKernelGGL(fr_axpby_kernel, dim3(grid_for(ctx, n)), dim3(256), 0, ctx->stream, (Fr *)y, sv, true, (const Fr *)nullptr, Fr::one(), n);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

// out[i] = sum_j coeffs[j] * polys[j][i]
int h2hip_fr_linear_combination_dev(h2hip_ctx *ctx, void *out, const void *const *polys, const void *coeffs, size_t count, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (n == 0 || out) && (count == 0 || (polys && coeffs)), "NULL argument");
    if (!n) return H2HIP_OK;
    for (size_t j = 0; j < count; ++j) H2_REQUIRE(polys[j], "NULL polynomial");
    if (!count) {
        H2_HIPCHK(hipMemsetAsync(out, 0, sizeof(Fr) * n, ctx->stream));
        return H2HIP_OK;
    }
    const Fr *cs = (const Fr *)coeffs;
    for (size_t j0 = 0; j0 < count; j0 += LINCOMB_MAX) {
        LinCombArgs a;
        a.count = (uint32_t)(count - j0 < LINCOMB_MAX ? count - j0 : LINCOMB_MAX);
        a.accumulate = j0 ? 1u : 0u;
        for (uint32_t t = 0; t < LINCOMB_MAX; ++t) {
            const bool live = t < a.count;
            Fr c;
            if (live) memcpy(&c, cs + j0 + t, sizeof(Fr));
            a.p[t] = live ? (const Fr *)polys[j0 + t] : nullptr;
            a.c[t] = live ? fr29_from_sat(c) : Fr29::zero();
        }
        prof_begin(ctx, "fr_lincomb_kernel");
        hipLaunchKernelGGL(fr_lincomb_kernel, dim3(grid_for(ctx, n)), dim3(256), 0, ctx->stream, (Fr *)out, a, n);
        prof_end(ctx);
    }
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

// ------------------------------------------------------------------ K4 / K5
}  // extern "C"
namespace h2 {
int fr_batch_invert_to(h2hip_ctx *ctx, const Fr *src, Fr *dst, size_t n) {   // dst == src: in place
    if (!n) return H2HIP_OK;
    Fr *scratch = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP1, sizeof(Fr) * n, (void **)&scratch));
    // elements per lane: the inversion (division steps, ~50 products' worth of instructions) is cheap enough to spend one
    // per 8 elements — the dependent chain per lane (3 products per element + the inversion) is what the kernel waits for
    size_t per_lane = (size_t)ctx->fr_invert_run;
    if (per_lane < 1) {   // auto: about 2^16 lanes (measured optimum: 4 at 2^16, 8 at 2^19, 16-32 at 2^21; tools/invert_sweep.py)
        per_lane = n >> 16;
        per_lane = per_lane < 4 ? 4 : per_lane > 32 ? 32 : per_lane;
    }
    size_t lanes = (n + per_lane - 1) / per_lane;
    uint32_t blocks = (uint32_t)((lanes + 255) / 256);
    prof_begin(ctx, "fr_batch_invert_kernel");
    hipLaunchKernelGGL(fr_batch_invert_kernel, dim3(blocks), dim3(256), 0, ctx->stream, src, dst, scratch, n);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
}  // namespace h2
extern "C" {
int h2hip_fr_batch_invert_dev(h2hip_ctx *ctx, void *a, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (n == 0 || a), "NULL argument");
    return fr_batch_invert_to(ctx, (const Fr *)a, (Fr *)a, n);
}

// inclusive prefix products of `segments` independent runs of n elements, `seg_stride` elements apart (in -> out, same layout)
static int prefix_product_segments(h2hip_ctx *ctx, const Fr *in, Fr *out, size_t n, size_t segments, size_t seg_stride) {
    const uint32_t tile = 256 * SCAN_J;
    uint32_t ntiles = (uint32_t)((n + tile - 1) / tile);
    H2_REQUIRE(segments >= 1 && segments <= 65535, "1..65535 segments");
    Fr *tp = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP2, sizeof(Fr) * ((size_t)ntiles * segments + 1), (void **)&tp));
    prof_begin(ctx, "fr_prefix_prod_kernels");
    hipLaunchKernelGGL(fr_prefix_prod_tile_kernel, dim3(ntiles, (uint32_t)segments), dim3(256), 0, ctx->stream, in, out, tp, n, seg_stride);
    hipLaunchKernelGGL(fr_prefix_prod_sums_kernel, dim3((uint32_t)segments), dim3(1024), 0, ctx->stream, tp, ntiles);
    hipLaunchKernelGGL(fr_prefix_prod_apply_kernel, dim3(ntiles, (uint32_t)segments), dim3(256), 0, ctx->stream, out, (const Fr *)tp, n, seg_stride);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
static int prefix_product_inplace(h2hip_ctx *ctx, const Fr *in, Fr *out, size_t n) { return prefix_product_segments(ctx, in, out, n, 1, 0); }
}  // extern "C"
namespace h2 {
// dst[j][i] = src[j * src_stride + i], i < len, for `count` separately allocated destinations (32 per launch)
int fr_scatter_rows(h2hip_ctx *ctx, Fr *const *dst, size_t count, const Fr *src, size_t src_stride, size_t len) {
    if (!count || !len) return H2HIP_OK;
    prof_begin(ctx, "fr_scatter_rows_kernel");
    for (size_t s0 = 0; s0 < count; s0 += 32) {
        const uint32_t g = (uint32_t)(count - s0 < 32 ? count - s0 : 32);
        RowPtrs rows;
        for (uint32_t j = 0; j < 32; ++j) rows.p[j] = dst[s0 + (j < g ? j : 0)];
        hipLaunchKernelGGL(fr_scatter_rows_kernel, dim3(grid_for(ctx, len), g), dim3(256), 0, ctx->stream, rows, src + s0 * src_stride, src_stride, len);
    }
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
}  // namespace h2
extern "C" {
int h2hip_fr_prefix_product_dev(h2hip_ctx *ctx, void *out, const void *in, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (n == 0 || (out && in)), "NULL argument");
    if (!n) return H2HIP_OK;
    return prefix_product_inplace(ctx, (const Fr *)in, (Fr *)out, n);
}
// z[0] = 1, z[i+1] = z[i] * num[i] / den[i], i < n  (z has n+1 elements; 0 denominators count as 0^-1 := 0)
int h2hip_fr_grand_product_dev(h2hip_ctx *ctx, void *z, const void *num, const void *den, size_t n) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && z && (n == 0 || (num && den)), "NULL argument");
    Fr *zz = (Fr *)z;
    hipLaunchKernelGGL(fr_set_one_kernel, dim3(1), dim3(64), 0, ctx->stream, zz);
    if (!n) return H2HIP_OK;
    Fr *t = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP0, sizeof(Fr) * n, (void **)&t));
    H2_CHK(fr_batch_invert_to(ctx, (const Fr *)den, t, n));
    H2_CHK(binop(ctx, OP_MUL, t, t, num, n));
    return prefix_product_inplace(ctx, t, zz + 1, n);
}

// `segments` grand products of seg_len factors each in a handful of launches: num / den hold the factors of all segments back to back,
// z[s] receives seg_len + 1 values.  chained != 0: z[s][0] = z[s-1][seg_len] (z[0][0] = 1) — the permutation argument's sets; otherwise every
// z[s][0] = 1 — the lookup arguments.  0 denominators count as 0^-1 := 0.
int h2hip_fr_grand_products_dev(h2hip_ctx *ctx, void *const *z, const void *num, const void *den, size_t segments, size_t seg_len, int chained) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (segments == 0 || z) && (segments == 0 || seg_len == 0 || (num && den)), "NULL argument");
    if (!segments) return H2HIP_OK;
    for (size_t s2 = 0; s2 < segments; ++s2) H2_REQUIRE(z[s2], "NULL product column");
    H2_REQUIRE(segments <= 65535 && seg_len < ((size_t)1 << 40), "too many segments");
    const size_t total = segments * seg_len;
    const size_t rlen = chained ? total + 1 : segments * (seg_len + 1);
    Fr *t = nullptr, *r = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP0, sizeof(Fr) * (total + 2 * rlen), (void **)&t));
    r = t + total;
    Fr *e = r + rlen;
    if (!total) {
        for (size_t s2 = 0; s2 < segments; ++s2) hipLaunchKernelGGL(fr_set_one_kernel, dim3(1), dim3(64), 0, ctx->stream, (Fr *)z[s2]);
        H2_HIPCHK(hipGetLastError());
        return H2HIP_OK;
    }
    H2_CHK(fr_batch_invert_to(ctx, (const Fr *)den, t, total));   // (out of place: no copy of the denominators first)
    prof_begin(ctx, "fr_ratio_rows_kernel");
    hipLaunchKernelGGL(fr_ratio_rows_kernel, dim3(grid_for(ctx, total)), dim3(256), 0, ctx->stream, r, (const Fr *)num, (const Fr *)t, total, seg_len,
                       chained ? 1 : 0);
    prof_end(ctx);
    if (segments == 1) return prefix_product_segments(ctx, r, (Fr *)z[0], rlen, 1, 0);   // one product: straight into its column
    if (chained) H2_CHK(prefix_product_segments(ctx, r, e, rlen, 1, 0));
    else H2_CHK(prefix_product_segments(ctx, r, e, seg_len + 1, segments, seg_len + 1));
    // chained: consecutive products share one element (the last value of one is the first of the next): rows seg_len apart, seg_len + 1 long
    return fr_scatter_rows(ctx, (Fr *const *)z, segments, e, chained ? seg_len : seg_len + 1, seg_len + 1);
}

}  // extern "C"
