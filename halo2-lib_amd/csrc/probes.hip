// Micro-benchmark probes behind h2hip_bench_*: the multiplier roofline bench.py quotes, one NTT round in isolation,
// and the HBM gather / stream calibration.  No product path launches them.
#include "internal.h"
#include "fr29.cuh"
#include "fq29.cuh"

namespace h2 {

// Multiplier roofline probe: every lane runs CHAINS independent dependent-multiply chains of `iters` steps.
template <int CHAINS>
__global__ __launch_bounds__(256) void modmul_bench_kernel(Fr *__restrict__ io, uint32_t iters) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fr x[CHAINS];
    Fr y = io[i];
    y.l[7] &= 0x0fffffffu;
#pragma unroll
    for (int k = 0; k < CHAINS; ++k) {
        x[k] = y;
        x[k].l[0] ^= (uint32_t)k;
    }
    for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < CHAINS; ++k) x[k] = fe_mul(x[k], y);
    }
    Fr acc = x[0];
#pragma unroll
    for (int k = 1; k < CHAINS; ++k) acc = fe_add(acc, x[k]);
    io[i] = acc;
}


// the same probe on the unsaturated 9 x 29-bit representation (fq29.cuh) the MSM and NTT kernels multiply in
template <int CHAINS>
__global__ __launch_bounds__(256) void modmul29_bench_kernel(Fr *__restrict__ io, uint32_t iters) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fr y0 = io[i];
    y0.l[7] &= 0x0fffffffu;
    Fr29 y = f29_split<R29P>(y0), x[CHAINS];
#pragma unroll
    for (int k = 0; k < CHAINS; ++k) {
        x[k] = y;
        x[k].l[0] ^= (uint32_t)k;
    }
    for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < CHAINS; ++k) x[k] = f29_mul(x[k], y);
    }
    Fr29 acc = x[0];
#pragma unroll
    for (int k = 1; k < CHAINS; ++k) acc = f29_norm(f29_add(acc, x[k]));
    io[i] = f29_pack_canonical<FrP>(f29_mul(acc, Fr29::one()));
}

// r04 probe: ONE radix-4 round of the NTT pass kernel (ntt.hip: two stages, four products per lane, the lazy adds / subs / norms between
// them) in a loop, with the parts of the real kernel switched on one at a time — MODE 0: registers only; 1: the four elements and three
// twiddles come from LDS and go back to it every iteration (48-byte elements, conflict-free addresses of a later round); 2: + a block
// barrier per iteration; 3: like 2 with the first round's 4-way conflicting addresses.  Modes >= 1 declare the real kernel's LDS footprint
// (three workgroups per CU).  Reported as products/s (4 per lane and iteration): against h2hip_bench_modmul29's rate it says what the
// round's own instruction stream, its LDS round trip and its barrier each cost (tools/issue_probe.py).
struct alignas(16) ProbeElem {
    Fr29 v;
    uint32_t pad[3];
};
template <int MODE>
__global__ __launch_bounds__(256, 3) void ntt_round_probe_kernel(Fr *__restrict__ io, uint32_t iters) {
    HIP_DYNAMIC_SHARED(ProbeElem, plds)
    const uint32_t tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + tid;
    Fr y0 = io[i];
    y0.l[7] &= 0x0fffffffu;
    const Fr29 y = f29_split<R29P>(y0);
    Fr29 x0 = y, x1 = y, x2 = y, x3 = y;
    x1.l[0] ^= 1u;
    x2.l[0] ^= 2u;
    x3.l[0] ^= 3u;
    // addresses of a radix-4 group in a 1024-element tile with 4 columns: a later round (st = 2: conflict-free) or the first (st = 0)
    const uint32_t c = tid & 3u, p = tid >> 2;
    const uint32_t st = MODE == 3 ? 0u : 2u, h = 1u << st;
    const uint32_t e0 = ((((p >> st) << (st + 2)) + (p & (h - 1))) << 2) + c, stride = h << 2;
    ProbeElem *tw = plds + 1024;
    if (MODE >= 1) {
        plds[e0].v = x0;
        plds[e0 + stride].v = x1;
        plds[e0 + 2 * stride].v = x2;
        plds[e0 + 3 * stride].v = x3;
        if (tid < 128) tw[tid].v = y;
        __syncthreads();
    }
    Fr29 w1 = y, w2 = y, w3 = y;
    w2.l[1] ^= 5u;
    w3.l[1] ^= 9u;
    for (uint32_t it = 0; it < iters; ++it) {
        if (MODE >= 1) {
            x0 = plds[e0].v;
            x1 = plds[e0 + stride].v;
            x2 = plds[e0 + 2 * stride].v;
            x3 = plds[e0 + 3 * stride].v;
            w1 = tw[(tid + it) & 127u].v;
            w2 = tw[(tid + 2 * it + 1) & 127u].v;
            w3 = tw[(tid + 3 * it + 2) & 127u].v;
        }
        x1 = f29_mul(x1, w1);
        x3 = f29_mul(x3, w1);
        const Fr29 a0 = f29_add(x0, x1), a1 = f29_sub_lazy<2>(x0, x1);
        const Fr29 a2 = f29_mul_wide(f29_add(x2, x3), w2);
        const Fr29 a3 = f29_mul_wide(f29_sub_lazy<2>(x2, x3), w3);
        x0 = f29_norm(f29_add(a0, a2));
        x2 = f29_sub<2>(a0, a2);
        x1 = f29_norm(f29_add(a1, a3));
        x3 = f29_sub<2>(a1, a3);
        // keep the values inside the products' input bounds over many iterations (the real kernel runs <= 5 rounds per tile)
        x0 = f29_weak_reduce(x0);
        x1 = f29_weak_reduce(x1);
        x2 = f29_weak_reduce(x2);
        x3 = f29_weak_reduce(x3);
        if (MODE >= 1) {
            plds[e0].v = x0;
            plds[e0 + stride].v = x1;
            plds[e0 + 2 * stride].v = x2;
            plds[e0 + 3 * stride].v = x3;
        }
        if (MODE >= 2) __syncthreads();
    }
    const Fr29 acc = f29_norm(f29_add(f29_norm(f29_add(x0, x1)), f29_norm(f29_add(x2, x3))));
    io[i] = f29_pack_canonical<FrP>(f29_mul(acc, Fr29::one()));
}

// HBM-counter calibration probes (profiles/archive/r02_*_pmc_*.md): a random gather of aligned ENTRY-byte table entries — the access pattern
// of msm_accum_kernel's base-table reads (one aligned 64-byte entry per mixed addition out of a table far larger than the 256 MiB
// Infinity Cache) — with an exactly known useful byte count, and a coalesced stream of the same volume.
template <int ENTRY>
__global__ __launch_bounds__(256) void gather_probe_kernel(const uint4 *__restrict__ table, uint64_t entries, uint32_t per_lane, uint4 *__restrict__ out) {
    const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t state = lane * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    uint4 acc = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < per_lane; ++k) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t idx = (state >> 20) % entries;
        const uint4 *e = table + idx * (ENTRY / 16);
#pragma unroll
        for (int q = 0; q < ENTRY / 16; ++q) {
            uint4 v = e[q];
            acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w;
        }
    }
    out[lane] = acc;
}
__global__ __launch_bounds__(256) void stream_probe_kernel(const uint4 *__restrict__ table, uint64_t vec16, uint4 *__restrict__ out) {
    const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    uint4 acc = {0u, 0u, 0u, 0u};
    for (uint64_t i = lane; i < vec16; i += stride) {
        uint4 v = table[i];
        acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w;
    }
    out[lane] = acc;
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2hip_bench_modmul29(h2hip_ctx *ctx, uint32_t blocks, uint32_t iters, uint32_t chains, double *elapsed_ms, double *modmuls) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && elapsed_ms && modmuls && blocks && iters, "bad argument");
    H2_REQUIRE(chains == 1 || chains == 2 || (chains >= 16 && chains <= 19), "chains must be 1 or 2 (16..19: the NTT round probe, mode = chains - 16)");
    Fr *buf = nullptr;
    size_t lanes = (size_t)blocks * 256;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP0, sizeof(Fr) * lanes, (void **)&buf));
    H2_HIPCHK(hipMemsetAsync(buf, 0x5a, sizeof(Fr) * lanes, ctx->stream));
    const size_t probe_lds = sizeof(ProbeElem) * (1024 + 128 + 8);
    for (int rep = 0; rep < 2; ++rep) {   // rep 0 = warm-up
        H2_CHK(h2hip_timer_start(ctx));
        if (chains == 1) hipLaunchKernelGGL(modmul29_bench_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, buf, iters);
        if (chains == 2) hipLaunchKernelGGL(modmul29_bench_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, buf, iters);
        if (chains == 16) hipLaunchKernelGGL(ntt_round_probe_kernel<0>, dim3(blocks), dim3(256), 0, ctx->stream, buf, iters);
        if (chains == 17) hipLaunchKernelGGL(ntt_round_probe_kernel<1>, dim3(blocks), dim3(256), probe_lds, ctx->stream, buf, iters);
        if (chains == 18) hipLaunchKernelGGL(ntt_round_probe_kernel<2>, dim3(blocks), dim3(256), probe_lds, ctx->stream, buf, iters);
        if (chains == 19) hipLaunchKernelGGL(ntt_round_probe_kernel<3>, dim3(blocks), dim3(256), probe_lds, ctx->stream, buf, iters);
        H2_HIPCHK(hipGetLastError());
        H2_CHK(h2hip_timer_stop(ctx, elapsed_ms));
    }
    *modmuls = (double)lanes * iters * (chains >= 16 ? 4 : chains);
    return H2HIP_OK;
}

int h2hip_bench_modmul(h2hip_ctx *ctx, uint32_t blocks, uint32_t iters, uint32_t chains, double *elapsed_ms, double *modmuls) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && elapsed_ms && modmuls && blocks && iters, "bad argument");
    H2_REQUIRE(chains == 1 || chains == 2 || chains == 4, "chains must be 1, 2 or 4");
    Fr *buf = nullptr;
    size_t lanes = (size_t)blocks * 256;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP0, sizeof(Fr) * lanes, (void **)&buf));
    H2_HIPCHK(hipMemsetAsync(buf, 0x5a, sizeof(Fr) * lanes, ctx->stream));
    for (int rep = 0; rep < 2; ++rep) {   // rep 0 = warm-up
        H2_CHK(h2hip_timer_start(ctx));
        if (chains == 1) hipLaunchKernelGGL(modmul_bench_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, buf, iters);
        if (chains == 2) hipLaunchKernelGGL(modmul_bench_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, buf, iters);
        if (chains == 4) hipLaunchKernelGGL(modmul_bench_kernel<4>, dim3(blocks), dim3(256), 0, ctx->stream, buf, iters);
        H2_HIPCHK(hipGetLastError());
        H2_CHK(h2hip_timer_stop(ctx, elapsed_ms));
    }
    *modmuls = (double)lanes * iters * chains;
    return H2HIP_OK;
}

// kind 0: coalesced stream of table_bytes; kind 64 / 128: lanes * per_lane random gathers of aligned 64- / 128-byte entries from a
// table of table_bytes.  *useful_bytes = the bytes the lanes asked for.
int h2hip_bench_gather(h2hip_ctx *ctx, uint32_t kind, size_t table_bytes, uint32_t lanes, uint32_t per_lane, double *elapsed_ms, double *useful_bytes) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && elapsed_ms && useful_bytes && table_bytes >= 4096 && lanes >= 256 && per_lane >= 1, "bad argument");
    H2_REQUIRE(kind == 0 || kind == 64 || kind == 128, "kind must be 0 (stream), 64 or 128");
    void *table = nullptr, *out = nullptr;
    H2_HIPCHK(hipMalloc(&table, table_bytes));
    if (hipMalloc(&out, sizeof(uint4) * (size_t)lanes) != hipSuccess) {
        hipFree(table);
        set_error("hipMalloc failed");
        return H2HIP_ERR_NOMEM;
    }
    hipMemsetAsync(table, 0x5a, table_bytes, ctx->stream);
    const uint32_t blocks = lanes / 256;
    int rc = H2HIP_OK;
    for (int rep = 0; rep < 2 && rc == H2HIP_OK; ++rep) {   // rep 0 = warm-up
        rc = h2hip_timer_start(ctx);
        if (kind == 0) hipLaunchKernelGGL(stream_probe_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const uint4 *)table, (uint64_t)(table_bytes / 16), (uint4 *)out);
        if (kind == 64) hipLaunchKernelGGL(gather_probe_kernel<64>, dim3(blocks), dim3(256), 0, ctx->stream, (const uint4 *)table, (uint64_t)(table_bytes / 64), per_lane, (uint4 *)out);
        if (kind == 128) hipLaunchKernelGGL(gather_probe_kernel<128>, dim3(blocks), dim3(256), 0, ctx->stream, (const uint4 *)table, (uint64_t)(table_bytes / 128), per_lane, (uint4 *)out);
        if (rc == H2HIP_OK) rc = h2hip_timer_stop(ctx, elapsed_ms);
    }
    hipStreamSynchronize(ctx->stream);
    hipFree(table);
    hipFree(out);
    *useful_bytes = kind == 0 ? (double)table_bytes : (double)blocks * 256.0 * per_lane * kind;
    return rc;
}

}  // extern "C"
