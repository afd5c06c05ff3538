// Polynomial evaluation and kate division: the prover's evaluation round and the quotients of the
// multiopen argument, on saturated and on unsaturated 9 x 29-bit limbs (kate_29).
#include "internal.h"
#include "fr29.cuh"
#include "fq29.cuh"

namespace h2 {

// ------------------------------------------------------------------ K7: eval_polynomial / kate_division
struct PowTable {
    Fr p[24];
};
// `count` (polynomial, point) pairs in two launches and one copy-out — the prover's evaluation round (every queried polynomial at x and
// its rotations); a single evaluation is a batch of one.
// stage 1 (blockIdx.y = job): each workgroup evaluates its 256*EVAL_J coefficients relative to its first one: lane Horner over EVAL_J
// coefficients, then a tree with x^(EVAL_J * 2^l).  stage 2: one workgroup per job combines the tile values: sum_b tile_val[b] * X^b with
// X = x^(256*EVAL_J) = pw.p[8]; a lane's value is scaled by X^(per*tid) through a tree with Y^(2^l), Y = X^per.
constexpr uint32_t EVAL_J = 32;   // (r06: 8 -> 32: the 8-level workgroup tree costs a product per level on every lane, as much as 8 Horner steps; PMC: 446 -> see profiles/r06_quotient_pmc.md)
struct EvalJob {
    const Fr *coeffs;
    size_t n;
    Fr x;
    PowTable pw;
    Fr29 x29, one29, pw29[8];   // R' form of x, 1 and x^(EVAL_J * 2^l): the tile kernel on unsaturated limbs (fr29.cuh)
};
__global__ __launch_bounds__(256) void fr_eval_tile_batch_kernel(const EvalJob *__restrict__ jobs, uint32_t ntiles_max, Fr *__restrict__ tile_val) {
    __shared__ Fr sh[256];
    const EvalJob &job = jobs[blockIdx.y];
    const size_t n = job.n;
    const uint32_t tid = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * 256 + tid) * EVAL_J;
    if ((size_t)blockIdx.x * 256 * EVAL_J >= n && blockIdx.x) return;   // tile past the end of this polynomial (uniform per workgroup)
    const Fr x = job.x;
    const Fr *__restrict__ coeffs = job.coeffs;
    Fr acc = Fr::zero();
    for (int k = EVAL_J - 1; k >= 0; --k) {
        acc = fe_mul(acc, x);
        if (base + k < n) acc = fe_add(acc, coeffs[base + k]);
    }
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t d = 1, l = 0; d < 256; d <<= 1, ++l) {
        if ((tid & (2 * d - 1)) == 0) sh[tid] = fe_add(sh[tid], fe_mul(sh[tid + d], job.pw.p[l]));
        __syncthreads();
    }
    if (tid == 0) tile_val[(size_t)blockIdx.y * ntiles_max + blockIdx.x] = sh[0];
}
// the tile kernel on unsaturated limbs: the point is a per-job constant (R' form), coefficients enter as raw splits, the Horner value stays lazy
// between products; the tile's value (< 11 r after the tree) leaves through one product with R'(1)
__global__ __launch_bounds__(256) void fr_eval_tile_batch29_kernel(const EvalJob *__restrict__ jobs, uint32_t ntiles_max, Fr *__restrict__ tile_val) {
    __shared__ Fr29 sh[256];
    const EvalJob &job = jobs[blockIdx.y];
    const size_t n = job.n;
    const uint32_t tid = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * 256 + tid) * EVAL_J;
    if ((size_t)blockIdx.x * 256 * EVAL_J >= n && blockIdx.x) return;   // tile past the end of this polynomial (uniform per workgroup)
    const Fr29 x = job.x29;
    const Fr *__restrict__ coeffs = job.coeffs;
    Fr29 acc = Fr29::zero();
#pragma unroll 1
    for (int k = EVAL_J - 1; k >= 0; --k) {
        acc = f29_mul(acc, x);
        if (base + k < n) acc = f29_add(acc, r29_load(coeffs[base + k]));
    }
    sh[tid] = f29_norm(acc);
    __syncthreads();
    for (uint32_t d = 1, l = 0; d < 256; d <<= 1, ++l) {
        if ((tid & (2 * d - 1)) == 0) sh[tid] = f29_norm(f29_add(sh[tid], f29_mul(sh[tid + d], job.pw29[l])));
        __syncthreads();
    }
    if (tid == 0) tile_val[(size_t)blockIdx.y * ntiles_max + blockIdx.x] = r29_store(f29_mul(sh[0], job.one29));
}
__global__ __launch_bounds__(256) void fr_eval_final_batch_kernel(const EvalJob *__restrict__ jobs, uint32_t ntiles_max, const Fr *__restrict__ tile_val,
                                                                  Fr *__restrict__ out) {
    __shared__ Fr sh[256];
    const EvalJob &job = jobs[blockIdx.x];
    const Fr *tv = tile_val + (size_t)blockIdx.x * ntiles_max;
    uint32_t ntiles = (uint32_t)((job.n + 256 * EVAL_J - 1) / (256 * EVAL_J));
    if (!ntiles) ntiles = 1;
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ntiles + 255) / 256, lo = tid * per;
    const Fr X = job.pw.p[8];
    Fr acc = Fr::zero();
    for (int k = (int)per - 1; k >= 0; --k) {
        acc = fe_mul(acc, X);
        if (lo + k < ntiles) acc = fe_add(acc, tv[lo + k]);
    }
    sh[tid] = acc;
    __syncthreads();
    Fr Y = fe_pow_u64(X, per);
    for (uint32_t d = 1; d < 256; d <<= 1) {
        if ((tid & (2 * d - 1)) == 0) sh[tid] = fe_add(sh[tid], fe_mul(sh[tid + d], Y));
        Y = fe_sqr(Y);
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = sh[0];
}

// kate_division: q[m] = sum_{j>m} c_j b^(j-m-1), m = 0..n-2  (suffix Horner).  Stage 1 computes every
// workgroup's head H = sum_{j in tile} c_j b^(j-lo); stage 2 turns heads into carries
// carry[blk] = sum_{blk'>blk} H[blk'] * (b^TILE)^(blk'-blk-1); stage 3 replays the tile with its carry.
// (the head of one tile of 256 * J coefficients, saturated arithmetic; `top`: a virtual coefficient of index n, see KateJob::top)
template <uint32_t J>
__device__ __forceinline__ Fr kate_tile_head(const Fr *__restrict__ c, size_t n, size_t lo, Fr b, const PowTable &pw, Fr *sh, const Fr *top) {
    const uint32_t tid = threadIdx.x;
    const size_t base = lo + (size_t)tid * J;
    Fr h = Fr::zero();
    for (int k = (int)J - 1; k >= 0; --k) {
        h = fe_mul(h, b);
        if (base + k < n) h = fe_add(h, c[base + k]);
        else if (top && base + k == n) h = fe_add(h, *top);
    }
    sh[tid] = h;
    __syncthreads();
    // inclusive suffix scan: I_t = h_t + b^J * I_{t+1}
    for (uint32_t d = 1, l = 0; d < 256; d <<= 1, ++l) {
        Fr o = Fr::zero();
        if (tid + d < 256) o = sh[tid + d];
        __syncthreads();
        if (tid + d < 256) sh[tid] = fe_add(sh[tid], fe_mul(o, pw.p[l]));   // p[l] = b^(J*2^l)
        __syncthreads();
    }
    return sh[0];
}
// Division by the vanishing polynomial of SEVERAL points in one pass (ProverSHPLONK's per-rotation-set quotient): by partial fractions,
//   (f(X) - r(X)) / prod_j (X - b_j)  =  sum_j w_j * (f(X) - f(b_j)) / (X - b_j),   w_j = 1 / prod_{i != j} (b_j - b_i),
// where r is the interpolant of f on the b_j — so the quotient is a weighted sum of independent kate divisions of the SAME polynomial: the
// heads / carries of all points are computed side by side and one pass over f writes the combined quotient (instead of one
// heads-carry-apply triple per root on a shrinking intermediate).
struct KateJob {
    Fr b, w;
    Fr top;   // range division (h2hip_fr_kate_division_range_dev): sum_{i >= n} f_i b^(i - n) over the coefficients ABOVE the range held here,
              // which enters the suffix Horner as one more coefficient of index n; zero otherwise
    PowTable pw;
};
// (J = coefficients per lane: a tile is 256 * J coefficients.  The multi-point kernels pick J by the polynomial's length — when there are fewer
// waves than SIMDs, a wave's instruction count IS the kernel's time, and short tiles spread a short polynomial over more waves)
template <uint32_t J>
__global__ __launch_bounds__(256) void fr_kate_heads_multi_kernel(const Fr *__restrict__ c, size_t n, const KateJob *__restrict__ jobs, uint32_t ntiles,
                                                                  Fr *__restrict__ heads) {
    __shared__ Fr sh[256];
    const KateJob &job = jobs[blockIdx.y];
    Fr h = kate_tile_head<J>(c, n, (size_t)blockIdx.x * (256 * J), job.b, job.pw, sh, &job.top);
    if (threadIdx.x == 0) heads[(size_t)blockIdx.y * (ntiles + 1) + blockIdx.x] = h;
}
__global__ __launch_bounds__(256) void fr_kate_carry_multi_kernel(const Fr *__restrict__ heads, Fr *__restrict__ carry, uint32_t ntiles,
                                                                  const KateJob *__restrict__ jobs) {
    __shared__ Fr sh[256];
    const uint32_t tid = threadIdx.x;
    const Fr *hd = heads + (size_t)blockIdx.x * (ntiles + 1);
    Fr *cr = carry + (size_t)blockIdx.x * (ntiles + 1);
    const PowTable &pw = jobs[blockIdx.x].pw;
    const uint32_t per = (ntiles + 255) / 256, lo = tid * per;
    const Fr B = pw.p[8];
    Fr h = Fr::zero();
    for (int k = (int)per - 1; k >= 0; --k) {
        h = fe_mul(h, B);
        if (lo + k < ntiles) h = fe_add(h, hd[lo + k]);
    }
    sh[tid] = h;
    __syncthreads();
    Fr Y = fe_pow_u64(B, per);
    for (uint32_t d = 1; d < 256; d <<= 1) {
        Fr o = Fr::zero();
        if (tid + d < 256) o = sh[tid + d];
        __syncthreads();
        if (tid + d < 256) sh[tid] = fe_add(sh[tid], fe_mul(o, Y));
        Y = fe_sqr(Y);
        __syncthreads();
    }
    Fr car = (tid + 1 < 256) ? sh[tid + 1] : Fr::zero();
    for (int k = (int)per - 1; k >= 0; --k) {
        if (lo + k < ntiles) {
            cr[lo + k] = car;
            car = fe_add(hd[lo + k], fe_mul(car, B));
        }
    }
}
// All M points of the set advance together through one pass over the tile: their Horner values, their suffix scans (one pair of barriers
// per doubling step for all points) and their quotient chains; the tile's incoming carry sits in an extra scan slot (index 256), which the scan
// multiplies by the right power of b^J on its own.  Points beyond m (padding up to the compiled M) carry weight 0.
// (static_for, field.cuh: with `for (j < M)` + `#pragma unroll` the compiler leaves the loops around two field multiplications per point rolled
// and the per-point arrays in scratch memory)
template <int M, uint32_t J, bool TOP>
__global__ __launch_bounds__(256) void fr_kate_apply_multi_kernel(const Fr *__restrict__ c, size_t n, const KateJob *__restrict__ jobs, uint32_t m,
                                                                  uint32_t ntiles, const Fr *__restrict__ carry, Fr *__restrict__ q, int accumulate) {
    __shared__ Fr sh[M][257];
    const uint32_t tid = threadIdx.x;
    const size_t lo = (size_t)blockIdx.x * (256 * J), base = lo + (size_t)tid * J;
    const int ktop = TOP && n >= base && n < base + J ? (int)(n - base) : -1;   // the lane (one in the grid) that holds the virtual coefficient n
    const size_t n_out = n + (TOP ? 1 : 0);
    // (no per-lane arrays over k either: the k loops stay rolled, the coefficients are read again in the second pass — the tile was just read,
    // they come from the caches.  The job list is padded with zero jobs up to M: b, w are wave-uniform loads, no select)
    Fr b[M], h[M];
    static_for<M>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        b[j] = jobs[j].b;
        h[j] = Fr::zero();
    });
#pragma unroll 1
    for (int k = (int)J - 1; k >= 0; --k) {
        const Fr cvk = base + k < n ? c[base + k] : Fr::zero();   // coefficients past n are zero
        static_for<M>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            h[j] = fe_add(fe_mul(h[j], b[j]), cvk);
            if (TOP && k == ktop) h[j] = fe_add(h[j], jobs[j].top);
        });
    }
    static_for<M>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        sh[j][tid] = h[j];
        if (tid == 0) sh[j][256] = (uint32_t)j < m ? carry[(size_t)j * (ntiles + 1) + blockIdx.x] : Fr::zero();
    });
    __syncthreads();
    for (uint32_t d = 1, l = 0; d <= 256; d <<= 1, ++l) {   // inclusive suffix scan over 257 slots: I_t = h_t + b^J * I_{t+1}, I_256 = carry
        Fr o[M];
        static_for<M>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            o[j] = tid + d <= 256 ? sh[j][tid + d] : Fr::zero();
        });
        __syncthreads();
        if (tid + d <= 256) {
            static_for<M>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                if ((uint32_t)j < m) sh[j][tid] = fe_add(sh[j][tid], fe_mul(o[j], jobs[j].pw.p[l]));
            });
        }
        __syncthreads();
    }
    Fr tmp[M], w[M];
    static_for<M>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        tmp[j] = sh[j][tid + 1];
        w[j] = jobs[j].w;
    });
#pragma unroll 1
    for (int k = (int)J - 1; k >= 0; --k) {
        const Fr cvk = base + k < n ? c[base + k] : Fr::zero();
        Fr acc = Fr::zero();
        static_for<M>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            tmp[j] = fe_add(cvk, fe_mul(tmp[j], b[j]));             // = quotient coefficient of index base + k - 1 for point j
            if (TOP && k == ktop) tmp[j] = fe_add(tmp[j], jobs[j].top);
            acc = fe_add(acc, fe_mul(w[j], tmp[j]));
        });
        if (base + k < n_out && base + k >= 1) q[base + k - 1] = accumulate ? fe_add(q[base + k - 1], acc) : acc;
    }
}

// ---- the multi-point division on unsaturated limbs (fr29.cuh).  Every product of these kernels has a per-root CONSTANT operand (b, the scan's
// powers of b, the weights), which arrive in R' form: stored coefficients enter as raw splits and everything stays in the stored domain.  Horner
// values are kept lazy (h b + c: limbs < 2^30) where the next product takes them, normalised where LDS or a dot product needs it; the scan's
// values grow by about r per doubling step (< 12 r: far inside the product's input range); a tile's head leaves through one product with R' (1).
struct KateJob29 {
    Fr29 b, w, one;        // R' form of the root, the weight and 1
    Fr29 top;              // raw split of KateJob::top
    Fr29 pw[9];            // R' form of b^(J * 2^l), l <= 8
};
template <uint32_t J>
__global__ __launch_bounds__(256) void fr_kate_heads_multi29_kernel(const Fr *__restrict__ c, size_t n, const KateJob29 *__restrict__ jobs, uint32_t ntiles,
                                                                    Fr *__restrict__ heads, int with_top) {
    __shared__ Fr29 sh[256];
    const KateJob29 &job = jobs[blockIdx.y];
    const uint32_t tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * (256 * J) + (size_t)tid * J;
    const Fr29 b = job.b;
    Fr29 h = Fr29::zero();
#pragma unroll 1
    for (int k = (int)J - 1; k >= 0; --k) {
        h = f29_mul(h, b);
        if (base + k < n) h = f29_add(h, r29_load(c[base + k]));
        else if (with_top && base + k == n) h = f29_add(h, job.top);
    }
    sh[tid] = f29_norm(h);
    __syncthreads();
    for (uint32_t d = 1, l = 0; d < 256; d <<= 1, ++l) {   // inclusive suffix scan: I_t = h_t + b^J * I_{t+1}
        Fr29 o = Fr29::zero();
        if (tid + d < 256) o = sh[tid + d];
        __syncthreads();
        if (tid + d < 256) sh[tid] = f29_norm(f29_add(sh[tid], f29_mul(o, job.pw[l])));
        __syncthreads();
    }
    if (tid == 0) heads[(size_t)blockIdx.y * (ntiles + 1) + blockIdx.x] = r29_store(f29_mul(sh[0], job.one));
}
template <int M, uint32_t J, bool TOP>
__global__ __launch_bounds__(256) void fr_kate_apply_multi29_kernel(const Fr *__restrict__ c, size_t n, const KateJob29 *__restrict__ jobs, uint32_t m,
                                                                    uint32_t ntiles, const Fr *__restrict__ carry, Fr *__restrict__ q, int accumulate) {
    __shared__ Fr29 sh[M][257];
    const uint32_t tid = threadIdx.x;
    const size_t lo = (size_t)blockIdx.x * (256 * J), base = lo + (size_t)tid * J;
    const int ktop = TOP && n >= base && n < base + J ? (int)(n - base) : -1;
    const size_t n_out = n + (TOP ? 1 : 0);
    Fr29 b[M], h[M];
    static_for<M>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        b[j] = jobs[j].b;   // (zero jobs behind the last point: weight 0)
        h[j] = Fr29::zero();
    });
#pragma unroll 1
    for (int k = (int)J - 1; k >= 0; --k) {
        const Fr29 cvk = base + k < n ? r29_load(c[base + k]) : Fr29::zero();
        static_for<M>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            h[j] = f29_add(f29_mul(h[j], b[j]), cvk);                              // lazy: limbs < 2^30, value < 2.02 r
            if (TOP && k == ktop) h[j] = f29_norm(f29_add(h[j], jobs[j].top));
        });
    }
    static_for<M>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        sh[j][tid] = f29_norm(h[j]);
        if (tid == 0) sh[j][256] = (uint32_t)j < m ? r29_load(carry[(size_t)j * (ntiles + 1) + blockIdx.x]) : Fr29::zero();
    });
    __syncthreads();
    for (uint32_t d = 1, l = 0; d <= 256; d <<= 1, ++l) {   // inclusive suffix scan over 257 slots: I_t = h_t + b^J * I_{t+1}, I_256 = carry
        Fr29 o[M];
        static_for<M>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            o[j] = tid + d <= 256 ? sh[j][tid + d] : Fr29::zero();
        });
        __syncthreads();
        if (tid + d <= 256) {
            static_for<M>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                if ((uint32_t)j < m) sh[j][tid] = f29_norm(f29_add(sh[j][tid], f29_mul(o[j], jobs[j].pw[l])));
            });
        }
        __syncthreads();
    }
    Fr29 tmp[M], w[M];
    static_for<M>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        tmp[j] = sh[j][tid + 1];
        w[j] = jobs[j].w;
    });
#pragma unroll 1
    for (int k = (int)J - 1; k >= 0; --k) {
        const Fr29 cvk = base + k < n ? r29_load(c[base + k]) : Fr29::zero();
        static_for<M>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            tmp[j] = f29_add(cvk, f29_mul(tmp[j], b[j]));                          // = quotient coefficient of index base + k - 1 for point j
            if (TOP && k == ktop) tmp[j] = f29_add(tmp[j], jobs[j].top);
            tmp[j] = f29_norm(tmp[j]);                                             // N, < 3.03 r
        });
        const Fr acc = r29_store(f29_dot<M>(w, tmp));                              // sum_j w_j q_j with one reduction: < 1 + M * 3.06 / 169
        if (base + k < n_out && base + k >= 1) q[base + k - 1] = accumulate ? fe_add(q[base + k - 1], acc) : acc;
    }
}

}  // namespace h2

using namespace h2;

extern "C" {

// ------------------------------------------------------------------ K7
static void pow_table(const Fr &x, uint32_t j, PowTable &pw) {
    // p[l] = x^(j*2^l) for l = 0..23
    Fr v = fe_pow_u64(x, j);
    for (int l = 0; l < 24; ++l) {
        pw.p[l] = v;
        v = fe_sqr(v);
    }
}
}  // extern "C"
namespace h2 {
// `count` (polynomial, point) pairs: two launches and one copy-out; n == 0 evaluates to 0
static int eval_polynomials_run(h2hip_ctx *ctx, const void *const *coeffs_dev, const size_t *lens, const void *points, size_t count, void *out_host) {
    std::vector<EvalJob> jobs(count);
    std::vector<size_t> distinct;   // jobs holding the first table of each point
    size_t nmax = 0;
    for (size_t j = 0; j < count; ++j) {
        jobs[j].coeffs = (const Fr *)coeffs_dev[j];
        jobs[j].n = lens[j];
        memcpy(&jobs[j].x, (const char *)points + sizeof(Fr) * j, sizeof(Fr));
        // a proof asks for hundreds of evaluations at a handful of points (x and its rotations): one power table per distinct point
        size_t seen = j;
        for (size_t t = 0; t < distinct.size(); ++t)
            if (jobs[distinct[t]].x == jobs[j].x) {
                seen = distinct[t];
                break;
            }
        if (seen != j) {
            jobs[j].pw = jobs[seen].pw;
            jobs[j].x29 = jobs[seen].x29;
            jobs[j].one29 = jobs[seen].one29;
            for (int l = 0; l < 8; ++l) jobs[j].pw29[l] = jobs[seen].pw29[l];
        } else {
            pow_table(jobs[j].x, EVAL_J, jobs[j].pw);   // p[8] = x^(EVAL_J*256) = x^tile
            jobs[j].x29 = r29_const(jobs[j].x);
            jobs[j].one29 = r29_const(Fr::one());
            for (int l = 0; l < 8; ++l) jobs[j].pw29[l] = r29_const(jobs[j].pw.p[l]);
            if (distinct.size() < 16) distinct.push_back(j);
        }
        if (lens[j] > nmax) nmax = lens[j];
    }
    const uint32_t tile = 256 * EVAL_J;
    uint32_t ntiles = (uint32_t)((nmax + tile - 1) / tile);
    if (!ntiles) ntiles = 1;
    char *buf = nullptr;
    const size_t jobs_bytes = (sizeof(EvalJob) * count + 255) / 256 * 256;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP2, jobs_bytes + sizeof(Fr) * ((size_t)ntiles * count + count), (void **)&buf));
    EvalJob *djobs = (EvalJob *)buf;
    Fr *tv = (Fr *)(buf + jobs_bytes), *res = tv + (size_t)ntiles * count;
    H2_HIPCHK(hipMemcpyAsync(djobs, jobs.data(), sizeof(EvalJob) * count, hipMemcpyHostToDevice, ctx->stream));
    prof_begin(ctx, "fr_eval_kernels");
    if (ctx->kate_29)
        hipLaunchKernelGGL(fr_eval_tile_batch29_kernel, dim3(ntiles, (uint32_t)count), dim3(256), 0, ctx->stream, (const EvalJob *)djobs, ntiles, tv);
    else
        hipLaunchKernelGGL(fr_eval_tile_batch_kernel, dim3(ntiles, (uint32_t)count), dim3(256), 0, ctx->stream, (const EvalJob *)djobs, ntiles, tv);
    hipLaunchKernelGGL(fr_eval_final_batch_kernel, dim3((uint32_t)count), dim3(256), 0, ctx->stream, (const EvalJob *)djobs, ntiles, (const Fr *)tv, res);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return sync_results(ctx, out_host, res, sizeof(Fr) * count);   // (the wait also keeps `jobs` alive until the upload has been consumed)
}
}  // namespace h2
extern "C" {
int h2hip_fr_eval_polynomial_dev(h2hip_ctx *ctx, const void *coeffs, size_t n, const void *x, void *out_host) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && out_host && x && (n == 0 || coeffs), "NULL argument");
    return eval_polynomials_run(ctx, &coeffs, &n, x, 1, out_host);
}
int h2hip_fr_eval_polynomial_batch_dev(h2hip_ctx *ctx, const void *const *coeffs_dev, const size_t *lens, const void *points, size_t count,
                                       void *out_host) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (count == 0 || (coeffs_dev && lens && points && out_host)), "NULL argument");
    if (!count) return H2HIP_OK;
    H2_REQUIRE(count <= 4096, "too many evaluations in one batch");
    for (size_t j = 0; j < count; ++j) H2_REQUIRE(lens[j] == 0 || coeffs_dev[j], "NULL polynomial");
    return eval_polynomials_run(ctx, coeffs_dev, lens, points, count, out_host);
}
}  // extern "C"
// q[0..n-1) = sum_j weights[j] * (f(X) - f(points[j])) / (X - points[j]),  m <= 8 points; q_dev must not alias coeffs_dev
// one quotient of the kind above per SET: sets[i] = (coefficients, points, weights, tops or NULL, m, output, add to the output?), all of n coefficients.
// The sets share one job table, one upload and ONE launch of the latency-bound carry kernel (a workgroup per job); heads and apply run per set.
struct KateSet {
    const void *coeffs, *points, *weights, *tops;
    uint32_t m;
    void *q;
    bool add_to_q;
};
template <uint32_t J>
static int kate_division_sets_run(h2hip_ctx *ctx, const KateSet *sets, size_t nsets, size_t n) {
    const uint32_t tile = 256 * J;
    bool any_top = false;
    for (size_t i = 0; i < nsets; ++i) any_top |= sets[i].tops != nullptr;
    const uint32_t ntiles = (uint32_t)((n + (any_top ? 1 : 0) + tile - 1) / tile);   // the virtual coefficient n may open a tile of its own
    // a pass handles up to four points and reads that many jobs: every set's jobs are padded with zero jobs (b = w = top = 0) to a multiple of four
    std::vector<uint32_t> first(nsets);
    uint32_t total = 0;
    for (size_t i = 0; i < nsets; ++i) {
        first[i] = total;
        total += (sets[i].m + 3) / 4 * 4;
    }
    std::vector<KateJob> jobs(total);
    memset((void *)jobs.data(), 0, sizeof(KateJob) * total);
    const bool k29 = ctx->kate_29 != 0;
    std::vector<KateJob29> jobs29(k29 ? total : 0);
    if (k29) memset((void *)jobs29.data(), 0, sizeof(KateJob29) * total);
    for (size_t i = 0; i < nsets; ++i)
        for (uint32_t j = 0; j < sets[i].m; ++j) {
            KateJob &jb = jobs[first[i] + j];
            memcpy(&jb.b, (const char *)sets[i].points + sizeof(Fr) * j, sizeof(Fr));
            memcpy(&jb.w, (const char *)sets[i].weights + sizeof(Fr) * j, sizeof(Fr));
            if (sets[i].tops) memcpy(&jb.top, (const char *)sets[i].tops + sizeof(Fr) * j, sizeof(Fr));
            pow_table(jb.b, J, jb.pw);   // p[l] = b^(J * 2^l): p[8] = b^tile
            if (k29) {   // the same job for the kernels on unsaturated limbs: constants in R' form
                KateJob29 &j9 = jobs29[first[i] + j];
                j9.b = r29_const(jb.b);
                j9.w = r29_const(jb.w);
                j9.one = r29_const(Fr::one());
                j9.top = r29_load(jb.top);
                for (int l = 0; l < 9; ++l) j9.pw[l] = r29_const(jb.pw.p[l]);
            }
        }
    char *buf = nullptr;
    const size_t jobs_bytes = (sizeof(KateJob) * total + 255) / 256 * 256, jobs29_bytes = (sizeof(KateJob29) * jobs29.size() + 255) / 256 * 256;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP2, jobs_bytes + jobs29_bytes + sizeof(Fr) * 2 * (size_t)total * (ntiles + 1), (void **)&buf));
    KateJob *djobs = (KateJob *)buf;
    KateJob29 *djobs29 = (KateJob29 *)(buf + jobs_bytes);
    Fr *heads = (Fr *)(buf + jobs_bytes + jobs29_bytes), *carry = heads + (size_t)total * (ntiles + 1);
    H2_CHK(upload_jobs(ctx, djobs, jobs.data(), sizeof(KateJob) * total));   // through the pinned ring: no synchronisation per call
    if (k29) H2_CHK(upload_jobs(ctx, djobs29, jobs29.data(), sizeof(KateJob29) * total));
    prof_begin(ctx, "fr_kate_kernels");
    if (nsets > 1) H2_HIPCHK(hipMemsetAsync(heads, 0, sizeof(Fr) * (size_t)total * (ntiles + 1), ctx->stream));   // (the padding jobs' rows: the carry launch reads them)
    for (size_t i = 0; i < nsets; ++i) {
        const uint32_t g0 = first[i];
        Fr *hd = heads + (size_t)g0 * (ntiles + 1);
        if (k29)
            hipLaunchKernelGGL(fr_kate_heads_multi29_kernel<J>, dim3(ntiles, sets[i].m), dim3(256), 0, ctx->stream, (const Fr *)sets[i].coeffs, n,
                               (const KateJob29 *)(djobs29 + g0), ntiles, hd, sets[i].tops ? 1 : 0);
        else
            hipLaunchKernelGGL(fr_kate_heads_multi_kernel<J>, dim3(ntiles, sets[i].m), dim3(256), 0, ctx->stream, (const Fr *)sets[i].coeffs, n,
                               (const KateJob *)(djobs + g0), ntiles, hd);
    }
    hipLaunchKernelGGL(fr_kate_carry_multi_kernel, dim3(nsets > 1 ? total : sets[0].m), dim3(256), 0, ctx->stream, (const Fr *)heads, carry, ntiles,
                       (const KateJob *)djobs);
    for (size_t i = 0; i < nsets; ++i) {
        const uint32_t m = sets[i].m;
        const int with_top = sets[i].tops != nullptr;
        for (uint32_t j0 = 0; j0 < m; j0 += 4) {   // four points per pass (the scans of a pass share the workgroup's LDS); halo2-base's sets stop at 4
            const uint32_t mm = m - j0 < 4 ? m - j0 : 4, g0 = first[i] + j0;
            const KateJob *jb = djobs + g0;
            const Fr *cr = carry + (size_t)g0 * (ntiles + 1);
            const int accumulate = (j0 || sets[i].add_to_q) ? 1 : 0;
            const Fr *cf = (const Fr *)sets[i].coeffs;
            Fr *qo = (Fr *)sets[i].q;
            auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(ntiles), dim3(256), 0, ctx->stream, cf, n, jb, mm, ntiles, cr, qo, accumulate); };
            const KateJob29 *jb29 = djobs29 + g0;
            auto go29 = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(ntiles), dim3(256), 0, ctx->stream, cf, n, jb29, mm, ntiles, cr, qo, accumulate); };
            if (k29 && with_top) {
                if (mm == 1) go29(fr_kate_apply_multi29_kernel<1, J, true>);
                else if (mm == 2) go29(fr_kate_apply_multi29_kernel<2, J, true>);
                else go29(fr_kate_apply_multi29_kernel<4, J, true>);
            } else if (k29) {
                if (mm == 1) go29(fr_kate_apply_multi29_kernel<1, J, false>);
                else if (mm == 2) go29(fr_kate_apply_multi29_kernel<2, J, false>);
                else go29(fr_kate_apply_multi29_kernel<4, J, false>);
            } else if (with_top) {
                if (mm == 1) go(fr_kate_apply_multi_kernel<1, J, true>);
                else if (mm == 2) go(fr_kate_apply_multi_kernel<2, J, true>);
                else go(fr_kate_apply_multi_kernel<4, J, true>);
            } else {
                if (mm == 1) go(fr_kate_apply_multi_kernel<1, J, false>);
                else if (mm == 2) go(fr_kate_apply_multi_kernel<2, J, false>);
                else go(fr_kate_apply_multi_kernel<4, J, false>);
            }
        }
    }
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
static int kate_division_sets_pick(h2hip_ctx *ctx, const KateSet *sets, size_t nsets, size_t n) {
    uint32_t j = ctx->kate_coeffs_per_lane;
    if (j != 1 && j != 2 && j != 4 && j != 8) j = n >= ((size_t)1 << 20) ? 8 : n >= ((size_t)1 << 18) ? 4 : n >= ((size_t)1 << 17) ? 2 : 1;   // (2^19: 4 and 8 within noise, 4 ahead by 0.04 ms per proof; 2^21: 8 ahead by 0.4 ms — profiles/archive/r04_kate_tile_ab.log)
    if (j == 8) return kate_division_sets_run<8>(ctx, sets, nsets, n);
    if (j == 4) return kate_division_sets_run<4>(ctx, sets, nsets, n);
    if (j == 2) return kate_division_sets_run<2>(ctx, sets, nsets, n);
    return kate_division_sets_run<1>(ctx, sets, nsets, n);
}
// coefficients per lane: a tile is 256 * J coefficients; about one wave per SIMD or more (ctx->kate_coeffs_per_lane overrides: 1, 2, 4, 8)
static int kate_division_multi_pick(h2hip_ctx *ctx, void *q, const void *coeffs, size_t n, const void *points, const void *weights, uint32_t m, const void *tops,
                                    bool add_to_q = false) {
    const KateSet one = {coeffs, points, weights, tops, m, q, add_to_q};
    return kate_division_sets_pick(ctx, &one, 1, n);
}
extern "C" {
int h2hip_fr_kate_division_multi_dev(h2hip_ctx *ctx, void *q, const void *coeffs, size_t n, const void *points, const void *weights, uint32_t m) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && points && weights && n >= 1 && coeffs && (n == 1 || q) && m >= 1 && m <= 8, "bad argument (1..8 points)");
    H2_REQUIRE(q != coeffs, "q must not alias coeffs");
    if (n == 1) return H2HIP_OK;
    return kate_division_multi_pick(ctx, q, coeffs, n, points, weights, m, nullptr);
}
// q[0..n-1) += the same sum: SHPLONK adds the rotation sets' quotients up with weights v^i — folded into weights[], the sum lands in its
// accumulator without a pass of its own
int h2hip_fr_kate_division_multi_acc_dev(h2hip_ctx *ctx, void *q, const void *coeffs, size_t n, const void *points, const void *weights, uint32_t m) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && points && weights && n >= 1 && coeffs && (n == 1 || q) && m >= 1 && m <= 8, "bad argument (1..8 points)");
    H2_REQUIRE(q != coeffs, "q must not alias coeffs");
    if (n == 1) return H2HIP_OK;
    return kate_division_multi_pick(ctx, q, coeffs, n, points, weights, m, nullptr, true);
}
// q[0..n-1) (+)= sum over `nsets` polynomials of that sum: coeffs_dev[i] with set_sizes[i] points / weights taken from the flat arrays in order (every
// set 1..8 points, all polynomials of n coefficients).  SHPLONK's whole v-weighted sum over the rotation sets in one call: one job table, one upload,
// ONE launch of the latency-bound carry kernel for all (set, point) pairs.  accumulate = 0: q is overwritten (by the first set).
int h2hip_fr_kate_division_sets_dev(h2hip_ctx *ctx, void *q, const void *const *coeffs, size_t n, const void *points, const void *weights,
                                    const uint32_t *set_sizes, size_t nsets, int accumulate) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && n >= 1 && (nsets == 0 || (coeffs && points && weights && set_sizes)) && (n == 1 || q) && nsets <= 64, "bad argument");
    if (n == 1 || !nsets) return H2HIP_OK;
    std::vector<KateSet> sets(nsets);
    size_t off = 0;
    for (size_t i = 0; i < nsets; ++i) {
        H2_REQUIRE(coeffs[i] && coeffs[i] != q && set_sizes[i] >= 1 && set_sizes[i] <= 8, "bad set (1..8 points, q must not alias a polynomial)");
        sets[i] = {coeffs[i], (const char *)points + sizeof(Fr) * off, (const char *)weights + sizeof(Fr) * off, nullptr, set_sizes[i], q, accumulate != 0 || i > 0};
        off += set_sizes[i];
    }
    return kate_division_sets_pick(ctx, sets.data(), nsets, n);
}
// q[0..n-1) = (f(X) - f(b)) / (X - b)   [UPSTREAM arithmetic::kate_division]: the one-point case of the kernels above (weight 1)
int h2hip_fr_kate_division_dev(h2hip_ctx *ctx, void *q, const void *coeffs, size_t n, const void *b) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && b && n >= 1 && coeffs && (n == 1 || q), "bad argument");
    H2_REQUIRE(q != coeffs, "q must not alias coeffs");
    if (n == 1) return H2HIP_OK;
    const Fr one = Fr::one();
    return kate_division_multi_pick(ctx, q, coeffs, n, b, &one, 1, nullptr);
}
// The same division for ONE COEFFICIENT RANGE [lo, lo + n) of f (the multi-GPU prover: a rank holds the range of its SRS slice): coeffs_dev = that
// range, carries[j] = sum_{i >= lo + n} f_i points[j]^(i - lo - n) — what the ranges above contribute, assembled by the caller from the ranks'
// partial evaluations (zero for the top range) — and q_dev[0..n) = the quotient's coefficients lo .. lo + n - 1 (n values, one more than the
// whole-polynomial call writes: the quotient coefficient lo + n - 1 is the carry itself).
int h2hip_fr_kate_division_range_dev(h2hip_ctx *ctx, void *q, const void *coeffs, size_t n, const void *points, const void *weights, const void *carries,
                                     uint32_t m) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && points && weights && carries && n >= 1 && coeffs && q && m >= 1 && m <= 8, "bad argument (1..8 points)");
    H2_REQUIRE(q != coeffs, "q must not alias coeffs");
    return kate_division_multi_pick(ctx, q, coeffs, n, points, weights, m, carries);
}

}  // extern "C"
