// The identities of the quotient polynomial h(X) on the extended domain: halo2-base's gate term, the
// lookup and permutation arguments, the division by the vanishing polynomial — on saturated and on unsaturated
// 9 x 29-bit limbs (quotient_29).
#include "internal.h"
#include "fr29.cuh"
#include "fq29.cuh"

namespace h2 {

// ------------------------------------------------------------------ K6: the identities of h(X)
// Pointwise over the extended domain (ne = 2^ext_k points, one circuit row = `step` = 2^(ext_k-k) points), every
// identity folded into the numerator as acc = acc*y + term in upstream's order [UPSTREAM evaluation.rs, SURVEY.md A.4/A.5;
// halo2-base creates these arguments at halo2-base/src/gates/range/mod.rs:131-150 (lookup) and
// halo2-base/src/gates/flex_gate/mod.rs:69,124-128 (equality-enabled columns)].
// gate term:  q[i] * (a[i] + a[i+s]*a[i+2s] - a[i+3s])  (indices mod ne, s = step): the single custom gate of halo2-base,
//        q*(a + b*c - d) at rotations 0..3 (reference halo2-base/src/gates/flex_gate/mod.rs:80-91)
// lookup terms: l0*(1-z) ; l_last*(z^2-z) ; active*(z(wX)(a'+beta)(s'+gamma) - z(X)(a+beta)(s+gamma)) ; l0*(a'-s') ;
//        active*(a'-s')*(a'-a'(w^-1 X)),   active = 1 - (l_last + l_blind)
// terms for one permutation set i: [first set] l0*(1-z) ; [last set] l_last*(z^2-z) ; [i>0] l0*(z_i - z_{i-1}(w^last X)) ;
//        active*( z(wX) prod_j(p_j + beta*s_j + gamma) - z(X) prod_j(p_j + delta^j*beta*X + gamma) ),  X = zeta*w_ext^i
constexpr int PERM_MAX_COLS = 8;

// One permutation set on unsaturated limbs (fr29.cuh): every product at the 9 x 29 rate, acc*y + term with ONE reduction.  One operand of every
// data x data product carries the factor 32 — taken when a stored element is split (r29_load32) or folded into the constants of the factor
// it is built from: the X term's start value, beta and gamma arrive as 32 beta zeta delta^j0, 32 beta, 32 gamma.  Bounds (multiples of r):
// acc < 1.64, the factors 32 p + 32 beta s + 32 gamma < 34.02, left / right < 1.25, every term's operands 32 x 3.3 at most.
struct PermArgs29 {
    const Fr *z, *z_prev, *l0, *l_last, *l_blind;
    const Fr *cols[PERM_MAX_COLS], *sigmas[PERM_MAX_COLS];
    uint32_t ncols, terms, last_rot_points;
    Fr29 beta32, delta, y, xstep;               // R' form (r29_const) of 32 beta, delta, y, ext_omega^(grid stride)
    Fr29 x0_delta32;                            // raw split of 32 beta zeta delta^j0 (stored domain): the X term's start = ext_omega^i0 (table, R' form) x this
    Fr29 gamma32;                               // raw split of (32 gamma mod r) in the stored domain
    OmegaTable pw;                              // ext_omega^e, e < 2^ext_k: the coset transforms' twiddle set (r06: was ~28 saturated products per lane)
};
__global__ __launch_bounds__(256, 3) void quotient_permutation29_kernel(Fr *__restrict__ acc, PermArgs29 g, size_t ne, uint32_t step) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, mask = ne - 1;
    const Fr one_sat = Fr::one();
    const Fr29 one = r29_load(one_sat);
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 >= ne) return;   // (the table holds ext_omega^e for e < ne only)
    Fr29 xbase = f29_mul(pow_lookup(g.pw.t1, g.pw.t2, g.pw.lo_bits, (uint64_t)i0), g.x0_delta32);   // 32 beta delta^j0 zeta w_ext^i, < 1.01
    for (size_t i = i0; i < ne; i += stride, xbase = f29_mul(xbase, g.xstep)) {
        const size_t inext = (i + step) & mask;
        const Fr z_sat = g.z[i], ll_sat = g.l_last[i];
        const Fr29 z = r29_load(z_sat);
        Fr29 v = r29_load(acc[i]);
        if (g.terms & H2HIP_PERM_FIRST) v = f29_mul2(v, g.y, r29_load32(g.l0[i]), f29_sub<2>(one, z));            // 1.64 + 32 * 3
        if (g.terms & H2HIP_PERM_LAST) {
            const Fr29 zz = f29_mul(r29_load32(z_sat), f29_sub<2>(z, one));                                       // z (z - 1) < 1.57
            v = f29_mul2(v, g.y, r29_load32(ll_sat), zz);
        }
        if (g.terms & H2HIP_PERM_CHAIN)
            v = f29_mul2(v, g.y, r29_load32(g.l0[i]), f29_sub<2>(z, r29_load(g.z_prev[(i + g.last_rot_points) & mask])));
        if (g.terms & H2HIP_PERM_PRODUCT) {
            Fr29 left = r29_load(g.z[inext]), right = z, xterm = xbase;
            for (uint32_t j = 0; j < g.ncols; ++j) {
                const Fr29 p32 = f29_add(r29_load32(g.cols[j][i]), g.gamma32);                                    // lazy, limbs < 2^30
                const Fr29 fl = f29_norm(f29_add(p32, f29_mul(r29_load(g.sigmas[j][i]), g.beta32)));              // 32 (p + beta s + gamma) < 34.02
                const Fr29 fr = f29_norm(f29_add(p32, xterm));
                left = f29_mul(left, fl);
                right = f29_mul(right, fr);
                xterm = f29_mul(xterm, g.delta);
            }
            const Fr active = fe_sub(one_sat, fe_add(ll_sat, g.l_blind[i]));
            v = f29_mul2(v, g.y, r29_load32(active), f29_sub<2>(left, right));                                    // 1.64 + 32 * 3.25
        }
        acc[i] = r29_store(v);
    }
}

// ---- the same identities for MANY columns / sets / lookups per launch (wide shapes: hundreds of columns of a few thousand rows): every
// launch reads and writes the accumulator once and folds its jobs in order, acc = acc*y + term per job — the same values as one launch per
// job, without a few-hundred-workgroup launch (and an accumulator round trip) per column.  Job tables travel as kernel arguments.
constexpr uint32_t GATE_BATCH = 64, LOOKUP_BATCH = 32, PERM_BATCH = 12;
struct GateBatchArgs {
    const Fr *q[GATE_BATCH], *a[GATE_BATCH];
    uint32_t count;
    Fr y;
};
__global__ __launch_bounds__(256) void quotient_flex_gate_batch_kernel(Fr *__restrict__ acc, GateBatchArgs g, size_t n_ext, uint32_t rot_step) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, mask = n_ext - 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ext; i += stride) {
        const size_t i1 = (i + rot_step) & mask, i2 = (i + 2 * (size_t)rot_step) & mask, i3 = (i + 3 * (size_t)rot_step) & mask;
        Fr v = acc[i];
        for (uint32_t j = 0; j < g.count; ++j) {
            const Fr *__restrict__ a = g.a[j];
            Fr t = fe_mul(g.q[j][i], fe_sub(fe_add(a[i], fe_mul(a[i1], a[i2])), a[i3]));
            v = fe_add(fe_mul(v, g.y), t);
        }
        acc[i] = v;
    }
}
// the RLC gate, q * (a * gamma + a(wX) - a(w^2 X)): one product by a constant and one by the selector per column, the same grid policy
struct RlcGateBatchArgs {
    const Fr *q[GATE_BATCH], *a[GATE_BATCH];
    uint32_t count;
    Fr gamma, y;
};
__global__ __launch_bounds__(256) void quotient_rlc_gate_batch_kernel(Fr *__restrict__ acc, RlcGateBatchArgs g, size_t n_ext, uint32_t rot_step) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, mask = n_ext - 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ext; i += stride) {
        const size_t i1 = (i + rot_step) & mask, i2 = (i + 2 * (size_t)rot_step) & mask;
        Fr v = acc[i];
        for (uint32_t j = 0; j < g.count; ++j) {
            const Fr *__restrict__ a = g.a[j];
            Fr t = fe_mul(g.q[j][i], fe_sub(fe_add(fe_mul(a[i], g.gamma), a[i1]), a[i2]));
            v = fe_add(fe_mul(v, g.y), t);
        }
        acc[i] = v;
    }
}
struct LookupJob {
    const Fr *z, *a, *s, *ap, *sp;
};
struct LookupBatchArgs {
    const Fr *l0, *l_last, *l_blind;
    Fr beta, gamma, y;
    uint32_t count;
    LookupJob jobs[LOOKUP_BATCH];
};
__global__ __launch_bounds__(256) void quotient_lookup_batch_kernel(Fr *__restrict__ acc, LookupBatchArgs g, size_t ne, uint32_t step) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, mask = ne - 1;
    const Fr one = Fr::one();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += stride) {
        const size_t inext = (i + step) & mask, iprev = (i + ne - step) & mask;
        const Fr l0 = g.l0[i], ll = g.l_last[i];
        const Fr active = fe_sub(one, fe_add(ll, g.l_blind[i]));
        Fr v = acc[i];
        for (uint32_t j = 0; j < g.count; ++j) {
            const LookupJob &q = g.jobs[j];
            Fr z = q.z[i], a = q.a[i], sv = q.s[i], ap = q.ap[i], sp = q.sp[i];
            v = fe_add(fe_mul(v, g.y), fe_mul(l0, fe_sub(one, z)));
            v = fe_add(fe_mul(v, g.y), fe_mul(ll, fe_sub(fe_sqr(z), z)));
            Fr left = fe_mul(fe_mul(q.z[inext], fe_add(ap, g.beta)), fe_add(sp, g.gamma));
            Fr right = fe_mul(fe_mul(z, fe_add(a, g.beta)), fe_add(sv, g.gamma));
            v = fe_add(fe_mul(v, g.y), fe_mul(active, fe_sub(left, right)));
            Fr d = fe_sub(ap, sp);
            v = fe_add(fe_mul(v, g.y), fe_mul(l0, d));
            v = fe_add(fe_mul(v, g.y), fe_mul(active, fe_mul(d, fe_sub(ap, q.ap[iprev]))));
        }
        acc[i] = v;
    }
}
struct PermJob {
    const Fr *z, *z_prev;
    const Fr *cols[PERM_MAX_COLS], *sigmas[PERM_MAX_COLS];
    Fr x0_delta;   // beta * zeta * delta^(first column index of the set)
    uint32_t ncols, terms;
};
struct PermBatchArgs {
    const Fr *l0, *l_last, *l_blind;
    Fr beta, gamma, delta, y, ext_omega, xstep;
    uint32_t last_rot_points, njobs;
    PermJob jobs[PERM_BATCH];
};
__global__ __launch_bounds__(256) void quotient_permutation_batch_kernel(Fr *__restrict__ acc, PermBatchArgs g, size_t ne, uint32_t step) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, mask = ne - 1;
    const Fr one = Fr::one();
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fr wpow = fe_pow_u64(g.ext_omega, (uint64_t)i0);   // w_ext^i
    for (size_t i = i0; i < ne; i += stride, wpow = fe_mul(wpow, g.xstep)) {
        const size_t inext = (i + step) & mask;
        const Fr l0 = g.l0[i], ll = g.l_last[i];
        const Fr active = fe_sub(one, fe_add(ll, g.l_blind[i]));
        Fr v = acc[i];
        for (uint32_t jb = 0; jb < g.njobs; ++jb) {
            const PermJob &q = g.jobs[jb];
            const Fr z = q.z[i];
            if (q.terms & H2HIP_PERM_FIRST) v = fe_add(fe_mul(v, g.y), fe_mul(l0, fe_sub(one, z)));
            if (q.terms & H2HIP_PERM_LAST) v = fe_add(fe_mul(v, g.y), fe_mul(ll, fe_sub(fe_sqr(z), z)));
            if (q.terms & H2HIP_PERM_CHAIN) v = fe_add(fe_mul(v, g.y), fe_mul(l0, fe_sub(z, q.z_prev[(i + g.last_rot_points) & mask])));
            if (q.terms & H2HIP_PERM_PRODUCT) {
                Fr left = q.z[inext], right = z;
                Fr xterm = fe_mul(q.x0_delta, wpow);
                for (uint32_t j = 0; j < q.ncols; ++j) {
                    Fr p = q.cols[j][i];
                    left = fe_mul(left, fe_add(fe_add(p, fe_mul(g.beta, q.sigmas[j][i])), g.gamma));
                    right = fe_mul(right, fe_add(fe_add(p, xterm), g.gamma));
                    xterm = fe_mul(xterm, g.delta);
                }
                v = fe_add(fe_mul(v, g.y), fe_mul(active, fe_sub(left, right)));
            }
        }
        acc[i] = v;
    }
}

// ---- the batched kernels on unsaturated limbs (fr29.cuh; see quotient_permutation29_kernel for the factor-of-32 bookkeeping).  Differences of
// stored elements that enter a data x data product are formed in saturated arithmetic first (an add-with-carry chain) and split with the factor.
__global__ __launch_bounds__(256) void quotient_flex_gate_batch29_kernel(Fr *__restrict__ acc, GateBatchArgs g, Fr29 y, size_t n_ext, uint32_t rot_step) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, mask = n_ext - 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ext; i += stride) {
        const size_t i1 = (i + rot_step) & mask, i2 = (i + 2 * (size_t)rot_step) & mask, i3 = (i + 3 * (size_t)rot_step) & mask;
        Fr29 v = r29_load(acc[i]);
        for (uint32_t j = 0; j < g.count; ++j) {
            const Fr *__restrict__ a = g.a[j];
            const Fr29 bc = f29_mul(r29_load32(a[i1]), r29_load(a[i2]));                        // < 1.19
            const Fr29 t = f29_sub<2>(f29_add(r29_load(a[i]), bc), r29_load(a[i3]));          // a + b c - d + 2 r < 4.2
            v = f29_mul2(v, y, r29_load32(g.q[j][i]), t);                                     // 1.8 + 32 * 4.2 = 136.2 -> < 1.81
        }
        acc[i] = r29_store(v);
    }
}
struct LookupConsts29 {
    Fr29 y;                  // R' form
    Fr29 beta32, gamma32;    // raw splits of 32 beta, 32 gamma (stored domain)
};
__global__ __launch_bounds__(256, 3) void quotient_lookup_batch29_kernel(Fr *__restrict__ acc, LookupBatchArgs g, LookupConsts29 k29, size_t ne, uint32_t step) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, mask = ne - 1;
    const Fr one_sat = Fr::one();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += stride) {
        const size_t inext = (i + step) & mask, iprev = (i + ne - step) & mask;
        const Fr ll_sat = g.l_last[i];
        const Fr29 l0 = r29_load32(g.l0[i]), ll = r29_load32(ll_sat), active = r29_load32(fe_sub(one_sat, fe_add(ll_sat, g.l_blind[i])));
        Fr29 v = r29_load(acc[i]);
        for (uint32_t j = 0; j < g.count; ++j) {
            const LookupJob &q = g.jobs[j];
            const Fr z_sat = q.z[i], ap_sat = q.ap[i], sp_sat = q.sp[i];
            const Fr29 z = r29_load(z_sat);
            v = f29_mul2(v, k29.y, l0, r29_load(fe_sub(one_sat, z_sat)));                                          // l0 (1 - z): 1.7 + 32
            v = f29_mul2(v, k29.y, ll, f29_mul(r29_load32(z_sat), r29_load(fe_sub(z_sat, one_sat))));              // l_last z (z - 1)
            Fr29 left = f29_mul(r29_load(q.z[inext]), f29_add(r29_load32(ap_sat), k29.beta32));                    // 1 x 33
            left = f29_mul(left, f29_add(r29_load32(sp_sat), k29.gamma32));                                        // 1.2 x 33
            Fr29 right = f29_mul(z, f29_add(r29_load32(q.a[i]), k29.beta32));
            right = f29_mul(right, f29_add(r29_load32(q.s[i]), k29.gamma32));
            v = f29_mul2(v, k29.y, active, f29_sub<2>(left, right));                                               // 1.7 + 32 * 3.25
            const Fr d_sat = fe_sub(ap_sat, sp_sat);
            v = f29_mul2(v, k29.y, l0, r29_load(d_sat));                                                           // l0 (a' - s')
            v = f29_mul2(v, k29.y, active, f29_mul(r29_load32(d_sat), r29_load(fe_sub(ap_sat, q.ap[iprev]))));     // active (a' - s')(a' - a'(w^-1 X))
        }
        acc[i] = r29_store(v);
    }
}
struct PermConsts29 {
    Fr29 beta32, delta, y, xstep;   // R' form of 32 beta, delta, y, ext_omega^(grid stride)
    Fr29 gamma32;                   // raw split of 32 gamma
    Fr29 x0_delta32[PERM_BATCH];    // raw split of 32 beta zeta delta^(first column of the job's set) (the X term = w_ext^i in R' form x this)
    OmegaTable pw;                  // ext_omega^e, e < 2^ext_k
};
__global__ __launch_bounds__(256, 3) void quotient_permutation_batch29_kernel(Fr *__restrict__ acc, PermBatchArgs g, PermConsts29 k29, size_t ne, uint32_t step) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, mask = ne - 1;
    const Fr one_sat = Fr::one();
    const Fr29 one = r29_load(one_sat);
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 >= ne) return;   // (the table holds ext_omega^e for e < ne only)
    Fr29 wpow = pow_lookup(k29.pw.t1, k29.pw.t2, k29.pw.lo_bits, (uint64_t)i0);   // w_ext^i in R' form (the chain stays there: xstep is an R' constant)
    for (size_t i = i0; i < ne; i += stride, wpow = f29_mul(wpow, k29.xstep)) {
        const size_t inext = (i + step) & mask;
        const Fr ll_sat = g.l_last[i];
        const Fr29 l0 = r29_load32(g.l0[i]), ll = r29_load32(ll_sat), active = r29_load32(fe_sub(one_sat, fe_add(ll_sat, g.l_blind[i])));
        Fr29 v = r29_load(acc[i]);
        for (uint32_t jb = 0; jb < g.njobs; ++jb) {
            const PermJob &q = g.jobs[jb];
            const Fr z_sat = q.z[i];
            const Fr29 z = r29_load(z_sat);
            if (q.terms & H2HIP_PERM_FIRST) v = f29_mul2(v, k29.y, l0, f29_sub<2>(one, z));
            if (q.terms & H2HIP_PERM_LAST) v = f29_mul2(v, k29.y, ll, f29_mul(r29_load32(z_sat), f29_sub<2>(z, one)));
            if (q.terms & H2HIP_PERM_CHAIN) v = f29_mul2(v, k29.y, l0, f29_sub<2>(z, r29_load(q.z_prev[(i + g.last_rot_points) & mask])));
            if (q.terms & H2HIP_PERM_PRODUCT) {
                Fr29 left = r29_load(q.z[inext]), right = z;
                Fr29 xterm = f29_mul(wpow, k29.x0_delta32[jb]);
                for (uint32_t j = 0; j < q.ncols; ++j) {
                    const Fr29 p32 = f29_add(r29_load32(q.cols[j][i]), k29.gamma32);
                    const Fr29 fl = f29_norm(f29_add(p32, f29_mul(r29_load(q.sigmas[j][i]), k29.beta32)));
                    const Fr29 fr = f29_norm(f29_add(p32, xterm));
                    left = f29_mul(left, fl);
                    right = f29_mul(right, fr);
                    xterm = f29_mul(xterm, k29.delta);
                }
                v = f29_mul2(v, k29.y, active, f29_sub<2>(left, right));
            }
        }
        acc[i] = r29_store(v);
    }
}

// ---- one launch path per family: the job list in; the batch chunking, the quotient_29 choice, the timer label and the launch here
static int quotient_gates_run(h2hip_ctx *ctx, Fr *acc, const void *const *q, const void *const *a, size_t count, uint32_t ext_k, uint32_t k, const Fr &y) {
    const size_t n_ext = (size_t)1 << ext_k;
    for (size_t j0 = 0; j0 < count; j0 += GATE_BATCH) {
        GateBatchArgs g;
        memset(&g, 0, sizeof(g));
        g.count = (uint32_t)(count - j0 < GATE_BATCH ? count - j0 : GATE_BATCH);
        g.y = y;
        for (uint32_t j = 0; j < g.count; ++j) {
            g.q[j] = (const Fr *)q[j0 + j];
            g.a[j] = (const Fr *)a[j0 + j];
        }
        prof_begin(ctx, "quotient_flex_gate_batch_kernel");
        if (ctx->quotient_29)
            hipLaunchKernelGGL(quotient_flex_gate_batch29_kernel, dim3(grid_for(ctx, n_ext)), dim3(256), 0, ctx->stream, acc, g, r29_const(g.y), n_ext,
                               1u << (ext_k - k));
        else
            hipLaunchKernelGGL(quotient_flex_gate_batch_kernel, dim3(grid_for(ctx, n_ext)), dim3(256), 0, ctx->stream, acc, g, n_ext, 1u << (ext_k - k));
        prof_end(ctx);
    }
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
static int quotient_rlc_gates_run(h2hip_ctx *ctx, Fr *acc, const void *const *q, const void *const *a, size_t count, uint32_t ext_k, uint32_t k, const Fr &gamma,
                                  const Fr &y) {
    const size_t n_ext = (size_t)1 << ext_k;
    for (size_t j0 = 0; j0 < count; j0 += GATE_BATCH) {
        RlcGateBatchArgs g;
        memset(&g, 0, sizeof(g));
        g.count = (uint32_t)(count - j0 < GATE_BATCH ? count - j0 : GATE_BATCH);
        g.gamma = gamma;
        g.y = y;
        for (uint32_t j = 0; j < g.count; ++j) {
            g.q[j] = (const Fr *)q[j0 + j];
            g.a[j] = (const Fr *)a[j0 + j];
        }
        prof_begin(ctx, "quotient_rlc_gate_batch_kernel");
        hipLaunchKernelGGL(quotient_rlc_gate_batch_kernel, dim3(grid_for(ctx, n_ext)), dim3(256), 0, ctx->stream, acc, g, n_ext, 1u << (ext_k - k));
        prof_end(ctx);
    }
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
static int quotient_lookups_run(h2hip_ctx *ctx, Fr *acc, const LookupJob *jobs, size_t count, const void *l0, const void *l_last, const void *l_blind,
                                uint32_t ext_k, uint32_t k, const void *beta, const void *gamma, const void *y) {
    const size_t ne = (size_t)1 << ext_k;
    for (size_t j0 = 0; j0 < count; j0 += LOOKUP_BATCH) {
        LookupBatchArgs g;
        memset(&g, 0, sizeof(g));
        g.l0 = (const Fr *)l0; g.l_last = (const Fr *)l_last; g.l_blind = (const Fr *)l_blind;
        g.beta = ld_fr(beta); g.gamma = ld_fr(gamma); g.y = ld_fr(y);
        g.count = (uint32_t)(count - j0 < LOOKUP_BATCH ? count - j0 : LOOKUP_BATCH);
        for (uint32_t j = 0; j < g.count; ++j) g.jobs[j] = jobs[j0 + j];
        prof_begin(ctx, "quotient_lookup_batch_kernel");
        if (ctx->quotient_29) {
            LookupConsts29 k29;
            k29.y = r29_const(g.y);
            k29.beta32 = r29_load(fe_x32(g.beta));
            k29.gamma32 = r29_load(fe_x32(g.gamma));
            hipLaunchKernelGGL(quotient_lookup_batch29_kernel, dim3(grid_for(ctx, ne)), dim3(256), 0, ctx->stream, acc, g, k29, ne, 1u << (ext_k - k));
        } else {
            hipLaunchKernelGGL(quotient_lookup_batch_kernel, dim3(grid_for(ctx, ne)), dim3(256), 0, ctx->stream, acc, g, ne, 1u << (ext_k - k));
        }
        prof_end(ctx);
    }
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
// workgroups of the permutation-identity kernels: 8 points per lane from 2^21 extended points, 4 / 2 / 1 for 2^20 / 2^19 / smaller domains
static uint32_t perm_grid(size_t ne) {
    size_t per_lane = ne >> 18;
    per_lane = per_lane < 1 ? 1 : per_lane > 8 ? 8 : per_lane;
    const size_t g = (ne / per_lane + 255) / 256;
    return g < 1 ? 1u : (uint32_t)g;
}
// (set, terms) jobs folded in order.  ONE job on unsaturated limbs goes to the dedicated one-set kernel (no job loop, the X term without the
// per-job product); everything else through the batched kernels, PERM_BATCH jobs per launch
static int quotient_permutation_run(h2hip_ctx *ctx, Fr *acc, const PermJob *jobs, size_t njobs, const void *l0, const void *l_last, const void *l_blind,
                                    uint32_t ext_k, uint32_t k, int32_t last_rotation, const void *beta, const void *gamma, const void *delta,
                                    const void *ext_omega, const void *y) {
    const size_t ne = (size_t)1 << ext_k;
    const uint32_t step = 1u << (ext_k - k);
    PermBatchArgs g;
    memset(&g, 0, sizeof(g));
    g.l0 = (const Fr *)l0; g.l_last = (const Fr *)l_last; g.l_blind = (const Fr *)l_blind;
    g.beta = ld_fr(beta); g.gamma = ld_fr(gamma); g.delta = ld_fr(delta); g.y = ld_fr(y); g.ext_omega = ld_fr(ext_omega);
    const int64_t n = (int64_t)1 << k;
    const int64_t rot = ((int64_t)last_rotation % n + n) % n;
    g.last_rot_points = (uint32_t)(((uint64_t)rot * step) & (ne - 1));
    // 8 extended points per lane from 2^21 points (fewer below: small domains need the lanes): the per-lane start-up (ext_omega^i0,
    // ~28 products) is amortised, the stride power is one host-side exponentiation
    const uint32_t pgrid = perm_grid(ne);
    g.xstep = fe_pow_u64(g.ext_omega, (uint64_t)pgrid * 256);
    OmegaTable pw = {nullptr, nullptr, 0};
    if (ctx->quotient_29) H2_CHK(ntt_pow_table(ctx, ext_k, g.ext_omega, &pw));   // (before the bracket: a new table launches its own profiled kernel)
    if (ctx->quotient_29 && njobs == 1) {
        const PermJob &q = jobs[0];
        PermArgs29 h;
        memset((void *)&h, 0, sizeof(h));
        h.z = q.z; h.z_prev = q.z_prev; h.l0 = g.l0; h.l_last = g.l_last; h.l_blind = g.l_blind;
        for (uint32_t j = 0; j < q.ncols; ++j) {
            h.cols[j] = q.cols[j];
            h.sigmas[j] = q.sigmas[j];
        }
        h.ncols = q.ncols; h.terms = q.terms; h.last_rot_points = g.last_rot_points;
        h.beta32 = r29_const(fe_x32(g.beta));
        h.delta = r29_const(g.delta);
        h.y = r29_const(g.y);
        h.x0_delta32 = r29_load(fe_x32(q.x0_delta));
        h.xstep = r29_const(g.xstep);
        h.gamma32 = r29_load(fe_x32(g.gamma));
        h.pw = pw;
        prof_begin(ctx, "quotient_permutation_kernel");
        hipLaunchKernelGGL(quotient_permutation29_kernel, dim3(pgrid), dim3(256), 0, ctx->stream, acc, h, ne, step);
        prof_end(ctx);
        H2_HIPCHK(hipGetLastError());
        return H2HIP_OK;
    }
    for (size_t j0 = 0; j0 < njobs; j0 += PERM_BATCH) {
        g.njobs = (uint32_t)(njobs - j0 < PERM_BATCH ? njobs - j0 : PERM_BATCH);
        for (uint32_t j = 0; j < g.njobs; ++j) g.jobs[j] = jobs[j0 + j];
        prof_begin(ctx, "quotient_permutation_batch_kernel");
        if (ctx->quotient_29) {
            PermConsts29 k29;
            k29.beta32 = r29_const(fe_x32(g.beta));
            k29.delta = r29_const(g.delta);
            k29.y = r29_const(g.y);
            k29.xstep = r29_const(g.xstep);
            k29.gamma32 = r29_load(fe_x32(g.gamma));
            for (uint32_t j = 0; j < PERM_BATCH; ++j) k29.x0_delta32[j] = j < g.njobs ? r29_load(fe_x32(g.jobs[j].x0_delta)) : Fr29::zero();
            k29.pw = pw;
            hipLaunchKernelGGL(quotient_permutation_batch29_kernel, dim3(pgrid), dim3(256), 0, ctx->stream, acc, g, k29, ne, step);
        } else {
            hipLaunchKernelGGL(quotient_permutation_batch_kernel, dim3(pgrid), dim3(256), 0, ctx->stream, acc, g, ne, step);
        }
        prof_end(ctx);
    }
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

}  // namespace h2

using namespace h2;

extern "C" {

// EvaluationDomain::divide_by_vanishing_poly [UPSTREAM poly/domain.rs, SURVEY.md A.2]: t(X) = X^n - 1 takes only
// L = 2^(ext_k-k) distinct values on the coset {zeta * ext_omega^i}: t_i = zeta^n * (ext_omega^n)^i - 1, period L.
__global__ __launch_bounds__(64) void vanishing_inverses_kernel(Fr *__restrict__ tinv, uint32_t L, Fr zeta_n, Fr step) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    Fr t = fe_sub(fe_mul(zeta_n, fe_pow_u64(step, i)), Fr::one());
    tinv[i] = fe_inv(t);   // t != 0: the coset avoids the n-th roots of unity
}
__global__ __launch_bounds__(256) void divide_by_vanishing_kernel(Fr *__restrict__ a, const Fr *__restrict__ tinv, size_t n_ext, uint32_t mask) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ext; i += stride) a[i] = fe_mul(a[i], tinv[i & mask]);
}
struct VanishSmall {
    Fr v[8];
};
__global__ __launch_bounds__(256) void divide_by_vanishing_small_kernel(Fr *__restrict__ a, VanishSmall t, size_t n_ext, uint32_t mask) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ext; i += stride) {
        Fr f = t.v[0];
#pragma unroll
        for (uint32_t k = 1; k < 8; ++k)
            if ((i & mask) == k) f = t.v[k];
        a[i] = fe_mul(a[i], f);
    }
}
int h2hip_divide_by_vanishing_poly_dev(h2hip_ctx *ctx, void *a, uint32_t ext_k, uint32_t k, const void *ext_omega, const void *zeta) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && a && ext_omega && zeta, "NULL argument");
    H2_REQUIRE(k <= ext_k && ext_k <= 28 && ext_k - k <= 16, "need k <= ext_k <= 28 and ext_k - k <= 16");
    Fr w, z;
    memcpy(&w, ext_omega, sizeof(Fr));
    memcpy(&z, zeta, sizeof(Fr));
    const uint64_t n = 1ull << k;
    const uint32_t L = 1u << (ext_k - k);
    Fr *tinv;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_VANISH, sizeof(Fr) * L, (void **)&tinv));
    prof_begin(ctx, "divide_by_vanishing_kernels");
    const Fr zn = fe_pow_u64(z, n), wn = fe_pow_u64(w, n);
    size_t n_ext = (size_t)1 << ext_k;
    if (L <= 8) {   // the usual case (ext_k - k <= 3): the few inverses are computed on the host and travel as kernel arguments
        VanishSmall t;
        Fr cur = zn;
        for (uint32_t i = 0; i < 8; ++i) {
            t.v[i] = i < L ? fe_inv(fe_sub(cur, Fr::one())) : Fr::zero();
            cur = fe_mul(cur, wn);
        }
        hipLaunchKernelGGL(divide_by_vanishing_small_kernel, dim3(grid_for(ctx, n_ext)), dim3(256), 0, ctx->stream, (Fr *)a, t, n_ext, L - 1);
    } else {
        hipLaunchKernelGGL(vanishing_inverses_kernel, dim3((L + 63) / 64), dim3(64), 0, ctx->stream, tinv, L, zn, wn);
        hipLaunchKernelGGL(divide_by_vanishing_kernel, dim3(grid_for(ctx, n_ext)), dim3(256), 0, ctx->stream, (Fr *)a, (const Fr *)tinv, n_ext, L - 1);
    }
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

// ------------------------------------------------------------------ K6: one identity per call
int h2hip_quotient_flex_gate_dev(h2hip_ctx *ctx, void *acc, const void *q, const void *a, uint32_t ext_k, uint32_t k, const void *y) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && acc && q && a && y, "NULL argument");
    H2_REQUIRE(k <= ext_k && ext_k <= 28, "need k <= ext_k <= 28");
    H2_REQUIRE(acc != a && acc != q, "acc must not alias an input");
    return quotient_gates_run(ctx, (Fr *)acc, &q, &a, 1, ext_k, k, ld_fr(y));
}
int h2hip_quotient_lookup_dev(h2hip_ctx *ctx, void *acc, const void *z, const void *a, const void *s, const void *a_perm, const void *s_perm,
                              const void *l0, const void *l_last, const void *l_blind, uint32_t ext_k, uint32_t k, const void *beta,
                              const void *gamma, const void *y) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && acc && z && a && s && a_perm && s_perm && l0 && l_last && l_blind && beta && gamma && y, "NULL argument");
    H2_REQUIRE(k <= ext_k && ext_k <= 28, "need k <= ext_k <= 28");
    const LookupJob job = {(const Fr *)z, (const Fr *)a, (const Fr *)s, (const Fr *)a_perm, (const Fr *)s_perm};
    return quotient_lookups_run(ctx, (Fr *)acc, &job, 1, l0, l_last, l_blind, ext_k, k, beta, gamma, y);
}
int h2hip_quotient_permutation_set_dev(h2hip_ctx *ctx, void *acc, const void *z, const void *z_prev, const void *const *cols,
                                       const void *const *sigmas, uint32_t ncols, uint32_t first_col_index, const void *l0, const void *l_last,
                                       const void *l_blind, uint32_t ext_k, uint32_t k, uint32_t terms, int32_t last_rotation,
                                       const void *beta, const void *gamma, const void *delta, const void *zeta, const void *ext_omega, const void *y) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && acc && z && l0 && l_last && l_blind && beta && gamma && delta && zeta && ext_omega && y, "NULL argument");
    H2_REQUIRE(terms != 0 && (terms & ~15u) == 0, "terms must be a non-empty mask of H2HIP_PERM_*");
    H2_REQUIRE(!(terms & H2HIP_PERM_CHAIN) || z_prev, "H2HIP_PERM_CHAIN needs z_prev_dev");
    if (!(terms & H2HIP_PERM_PRODUCT)) ncols = 0;
    H2_REQUIRE(!(terms & H2HIP_PERM_PRODUCT) || (cols && sigmas && ncols >= 1 && ncols <= PERM_MAX_COLS), "1..8 columns per permutation set");
    H2_REQUIRE(k <= ext_k && ext_k <= 28, "need k <= ext_k <= 28");
    PermJob job;
    memset(&job, 0, sizeof(job));
    job.z = (const Fr *)z; job.z_prev = (const Fr *)z_prev;
    for (uint32_t j = 0; j < ncols; ++j) {
        H2_REQUIRE(cols[j] && sigmas[j], "NULL column");
        job.cols[j] = (const Fr *)cols[j];
        job.sigmas[j] = (const Fr *)sigmas[j];
    }
    job.ncols = ncols; job.terms = terms;
    job.x0_delta = fe_mul(fe_mul(ld_fr(beta), ld_fr(zeta)), fe_pow_u64(ld_fr(delta), first_col_index));
    return quotient_permutation_run(ctx, (Fr *)acc, &job, 1, l0, l_last, l_blind, ext_k, k, last_rotation, beta, gamma, delta, ext_omega, y);
}

// ---- batched forms: all gate columns / all permutation sets / all lookups of a proof
int h2hip_quotient_flex_gate_batch_dev(h2hip_ctx *ctx, void *acc, const void *const *q, const void *const *a, size_t count, uint32_t ext_k, uint32_t k,
                                       const void *y) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && acc && y && (count == 0 || (q && a)), "NULL argument");
    H2_REQUIRE(k <= ext_k && ext_k <= 28, "need k <= ext_k <= 28");
    for (size_t j = 0; j < count; ++j) H2_REQUIRE(q[j] && a[j], "NULL column");
    return quotient_gates_run(ctx, (Fr *)acc, q, a, count, ext_k, k, ld_fr(y));
}
int h2hip_quotient_rlc_gate_batch_dev(h2hip_ctx *ctx, void *acc, const void *const *q, const void *const *a, size_t count, uint32_t ext_k, uint32_t k,
                                      const void *gamma, const void *y) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && acc && gamma && y && (count == 0 || (q && a)), "NULL argument");
    H2_REQUIRE(k <= ext_k && ext_k <= 28, "need k <= ext_k <= 28");
    for (size_t j = 0; j < count; ++j) H2_REQUIRE(q[j] && a[j] && q[j] != acc && a[j] != acc, "NULL column, or a column that aliases acc");
    return quotient_rlc_gates_run(ctx, (Fr *)acc, q, a, count, ext_k, k, ld_fr(gamma), ld_fr(y));
}
int h2hip_quotient_lookups_dev(h2hip_ctx *ctx, void *acc, const void *const *z, const void *const *a, const void *const *s, const void *const *a_perm,
                               const void *const *s_perm, size_t count, const void *l0, const void *l_last, const void *l_blind, uint32_t ext_k, uint32_t k,
                               const void *beta, const void *gamma, const void *y) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && acc && l0 && l_last && l_blind && beta && gamma && y && (count == 0 || (z && a && s && a_perm && s_perm)), "NULL argument");
    H2_REQUIRE(k <= ext_k && ext_k <= 28, "need k <= ext_k <= 28");
    std::vector<LookupJob> jobs(count);
    for (size_t t = 0; t < count; ++t) {
        H2_REQUIRE(z[t] && a[t] && s[t] && a_perm[t] && s_perm[t], "NULL column");
        jobs[t] = {(const Fr *)z[t], (const Fr *)a[t], (const Fr *)s[t], (const Fr *)a_perm[t], (const Fr *)s_perm[t]};
    }
    return quotient_lookups_run(ctx, (Fr *)acc, jobs.data(), count, l0, l_last, l_blind, ext_k, k, beta, gamma, y);
}
// the whole permutation argument in evaluate_h's order: FIRST (set 0), LAST (last set), CHAIN (sets 1..), PRODUCT (all sets)
int h2hip_quotient_permutation_sets_dev(h2hip_ctx *ctx, void *acc, const void *const *z, uint32_t num_sets, const void *const *cols, const void *const *sigmas,
                                        uint32_t num_columns, uint32_t chunk_len, const void *l0, const void *l_last, const void *l_blind, uint32_t ext_k,
                                        uint32_t k, int32_t last_rotation, const void *beta, const void *gamma, const void *delta, const void *zeta,
                                        const void *ext_omega, const void *y) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && acc && l0 && l_last && l_blind && beta && gamma && delta && zeta && ext_omega && y, "NULL argument");
    H2_REQUIRE(k <= ext_k && ext_k <= 28, "need k <= ext_k <= 28");
    if (!num_sets) return H2HIP_OK;
    H2_REQUIRE(z && cols && sigmas, "NULL argument");
    H2_REQUIRE(chunk_len >= 1 && chunk_len <= PERM_MAX_COLS, "1..8 columns per permutation set");
    H2_REQUIRE(num_columns > (uint64_t)(num_sets - 1) * chunk_len && num_columns <= (uint64_t)num_sets * chunk_len, "num_sets must be ceil(num_columns / chunk_len)");
    for (uint32_t s2 = 0; s2 < num_sets; ++s2) H2_REQUIRE(z[s2], "NULL product column");
    for (uint32_t c = 0; c < num_columns; ++c) H2_REQUIRE(cols[c] && sigmas[c], "NULL column");
    // the job list in upstream's order
    struct Item {
        uint32_t set, terms;
    };
    std::vector<Item> items;
    if (num_sets == 1) {
        items.push_back({0, H2HIP_PERM_FIRST | H2HIP_PERM_LAST | H2HIP_PERM_PRODUCT});
    } else {
        items.push_back({0, H2HIP_PERM_FIRST});
        items.push_back({num_sets - 1, H2HIP_PERM_LAST});
        for (uint32_t s2 = 1; s2 < num_sets; ++s2) items.push_back({s2, H2HIP_PERM_CHAIN});
        for (uint32_t s2 = 0; s2 < num_sets; ++s2) items.push_back({s2, H2HIP_PERM_PRODUCT});
    }
    const Fr dl = ld_fr(delta);
    Fr x0 = fe_mul(ld_fr(beta), ld_fr(zeta));   // beta * zeta * delta^(first column of set s), kept per set
    std::vector<Fr> set_x0(num_sets);
    for (uint32_t s2 = 0; s2 < num_sets; ++s2) {
        set_x0[s2] = x0;
        for (uint32_t c = 0; c < chunk_len; ++c) x0 = fe_mul(x0, dl);
    }
    std::vector<PermJob> jobs(items.size());
    for (size_t j = 0; j < items.size(); ++j) {
        const Item &it = items[j];
        PermJob &q = jobs[j];
        memset(&q, 0, sizeof(q));
        q.z = (const Fr *)z[it.set];
        q.z_prev = it.set ? (const Fr *)z[it.set - 1] : nullptr;
        q.terms = it.terms;
        q.x0_delta = set_x0[it.set];
        if (it.terms & H2HIP_PERM_PRODUCT) {
            const uint32_t c0 = it.set * chunk_len, c1 = c0 + chunk_len < num_columns ? c0 + chunk_len : num_columns;
            q.ncols = c1 - c0;
            for (uint32_t c = c0; c < c1; ++c) {
                q.cols[c - c0] = (const Fr *)cols[c];
                q.sigmas[c - c0] = (const Fr *)sigmas[c];
            }
        }
    }
    return quotient_permutation_run(ctx, (Fr *)acc, jobs.data(), jobs.size(), l0, l_last, l_blind, ext_k, k, last_rotation, beta, gamma, delta, ext_omega, y);
}

}  // extern "C"
