// h2hip_plonk_check_witness's kernels: MockProver's verdict (halo2-base/src/utils/testing.rs:183-188) for the one gate form and the lookup forms
// halo2-lib builds, over columns that are already resident.  plonk.hip derives the layout from the key (WitnessCheckJob); here:
//   one launch per kind over all its columns (blockIdx.y = column or lookup, x = rows): a failing (column, row) sets one bit of a mask laid out
//   [gate columns][lookups][permutation columns] x stride rows (stride = usable rows rounded up to 32), which is the canonical order;
//   a count kernel (popcount per 8192-unit block), the block counts to the host (64-bit prefix sums and the exact total), and a write kernel
//   over the blocks that hold the first max_failures: two host round trips per call whatever the number of columns.
// Each (column, row) is handled by exactly one thread, so a bit is set at most once and atomicAdd sets it as an OR would.
#include <algorithm>
#include <vector>

#include "internal.h"

namespace h2 {

namespace {

constexpr uint32_t WC_THREADS = 256;
constexpr uint32_t WC_BLOCK_WORDS = 256;   // mask words per count / write workgroup (8192 units)

struct alignas(16) WcKey {   // a 32-byte sort key, compared from limb 7 down (lookup_sort_keys_dev)
    uint32_t l[8];
};

__device__ __forceinline__ void wc_flag(uint32_t *mask, size_t unit) { atomicAdd(&mask[unit >> 5], 1u << (unit & 31)); }

// GATE: q * (a[r] + b[r+1] * c[r+2] - d[r+3]) on gate column blockIdx.y (flex_gate/mod.rs:80-91, the prover's quotient term); the gates from
// first_rlc on are RLC gates, q * (a[r] * gamma + a[r+1] - a[r+2])
__global__ __launch_bounds__(WC_THREADS) void wc_gate_kernel(const Fr *const *__restrict__ cols, const uint32_t *__restrict__ gate_adv,
                                                            const uint32_t *__restrict__ gate_q, uint32_t u, uint32_t stride, uint32_t *mask,
                                                            uint32_t first_rlc, Fr gamma) {
    const uint32_t g = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= u) return;
    const Fr q = cols[gate_q[g]][r];
    if (q.is_zero()) return;
    const uint32_t last = g >= first_rlc ? 2 : 3;
    bool fail = true;   // rows r + last >= u reach the blinding rows
    if (r + last < u) {
        const Fr *__restrict__ a = cols[gate_adv[g]];
        const Fr e = g >= first_rlc ? fe_mul(q, fe_sub(fe_add(fe_mul(a[r], gamma), a[r + 1]), a[r + 2]))
                                    : fe_mul(q, fe_sub(fe_add(a[r], fe_mul(a[r + 1], a[r + 2])), a[r + 3]));
        fail = !e.is_zero();
    }
    if (fail) wc_flag(mask, (size_t)g * stride + r);
}

// lower bound of key (limbs 7 .. from) among ks[0, u)
__device__ __forceinline__ uint32_t wc_lower_bound(const WcKey *__restrict__ ks, uint32_t u, const uint32_t *key, int from) {
    uint32_t lo = 0, hi = u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const WcKey m = ks[mid];
        bool less = false;
        for (int i = 7; i >= from; --i)
            if (m.l[i] != key[i]) {
                less = m.l[i] < key[i];
                break;
            }
        if (less) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// LOOKUP (range): the input q_lookup * a or a is a member of the table's sorted canonical keys
__global__ __launch_bounds__(WC_THREADS) void wc_lookup_range_kernel(const Fr *const *__restrict__ cols, const uint32_t *__restrict__ lk_in,
                                                                    const uint32_t *__restrict__ lk_q, const WcKey *__restrict__ table, uint32_t u,
                                                                    uint32_t stride, uint32_t *mask) {
    const uint32_t l = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= u) return;
    Fr v = cols[lk_in[l]][r];
    if (lk_q[l] != WC_NONE) v = fe_mul(cols[lk_q[l]][r], v);
    const Fr c = fe_from_mont(v);
    const uint32_t i = wc_lower_bound(table, u, c.l, 0);
    bool found = i < u;
    if (found) {
        const WcKey t = table[i];
        for (int j = 0; j < 8; ++j) found = found && t.l[j] == c.l[j];
    }
    if (!found) wc_flag(mask, (size_t)l * stride + r);
}

// a tuple's search key: Horner_theta over the tuple, canonical, limbs 7 .. 1 (limb 0 of a table key is its row)
__device__ __forceinline__ Fr wc_tuple_hash(const Fr *const *__restrict__ cols, const uint32_t *__restrict__ idx, uint32_t w, uint32_t r,
                                            const Fr &theta) {
    Fr acc = cols[idx[0]][r];
    for (uint32_t j = 1; j < w; ++j) acc = fe_add(fe_mul(acc, theta), cols[idx[j]][r]);
    return fe_from_mont(acc);
}
__global__ __launch_bounds__(WC_THREADS) void wc_dyn_keys_kernel(const Fr *const *__restrict__ cols, const uint32_t *__restrict__ tab, uint32_t w,
                                                                Fr theta, uint32_t u, uint32_t N, WcKey *__restrict__ keys) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    WcKey k;
    if (r < u) {
        const Fr h = wc_tuple_hash(cols, tab, w, r, theta);
        k.l[0] = r;
        for (int j = 1; j < 8; ++j) k.l[j] = h.l[j];
    } else {
        for (int j = 0; j < 8; ++j) k.l[j] = 0xFFFFFFFFu;   // above every canonical element
    }
    keys[r] = k;
}
// LOOKUP (dynamic table): exact membership of the input tuple; every table row whose key matches the hash is compared component by component,
// so a hash collision can neither hide nor invent a failure
__global__ __launch_bounds__(WC_THREADS) void wc_lookup_dyn_kernel(const Fr *const *__restrict__ cols, const uint32_t *__restrict__ in,
                                                                  const uint32_t *__restrict__ tab, uint32_t w, Fr theta,
                                                                  const WcKey *__restrict__ keys, uint32_t u, uint32_t stride, uint32_t *mask) {
    const uint32_t l = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= u) return;
    const uint32_t *__restrict__ mine = in + (size_t)l * w;
    const Fr h = wc_tuple_hash(cols, mine, w, r, theta);
    bool found = false;
    for (uint32_t i = wc_lower_bound(keys, u, h.l, 1); i < u && !found; ++i) {
        const WcKey k = keys[i];
        bool same = true;
        for (int j = 1; j < 8; ++j) same = same && k.l[j] == h.l[j];
        if (!same) break;
        found = true;
        for (uint32_t j = 0; j < w; ++j) found = found && cols[tab[j]][k.l[0]] == cols[mine[j]][r];
    }
    if (!found) wc_flag(mask, (size_t)l * stride + r);
}

// COPY: cell (p, r) equals sigma(p, r)
__global__ __launch_bounds__(WC_THREADS) void wc_copy_kernel(const Fr *const *__restrict__ cols, const uint32_t *__restrict__ perm_col,
                                                            const uint16_t *__restrict__ sigma_c, const uint32_t *__restrict__ sigma_r, uint32_t u,
                                                            uint32_t stride, uint32_t *mask) {
    const uint32_t p = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= u) return;
    const size_t i = (size_t)p * u + r;
    const uint32_t pc = sigma_c[i], pr = sigma_r[i];
    if (pc == p && pr == r) return;
    if (cols[perm_col[p]][r] != cols[perm_col[pc]][pr]) wc_flag(mask, (size_t)blockIdx.y * stride + r);
}

// failures per WC_BLOCK_WORDS mask words
__global__ __launch_bounds__(WC_BLOCK_WORDS) void wc_count_kernel(const uint32_t *__restrict__ mask, size_t words, uint32_t *__restrict__ counts) {
    __shared__ uint32_t part[WC_BLOCK_WORDS];
    const size_t w = (size_t)blockIdx.x * WC_BLOCK_WORDS + threadIdx.x;
    part[threadIdx.x] = w < words ? (uint32_t)__popc(mask[w]) : 0u;
    __syncthreads();
    for (uint32_t s = WC_BLOCK_WORDS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = part[0];
}

struct WcSegments {
    uint32_t gates, lookups, stride;
};
// the failures of block blockIdx.x, ranked from prefix[blockIdx.x] in mask order; ranks >= max are dropped
__global__ __launch_bounds__(WC_BLOCK_WORDS) void wc_write_kernel(const uint32_t *__restrict__ mask, size_t words, const uint64_t *__restrict__ prefix,
                                                                 uint64_t max, WcSegments seg, const uint32_t *__restrict__ gate_report,
                                                                 const uint16_t *__restrict__ sigma_c, const uint32_t *__restrict__ sigma_r, uint32_t u,
                                                                 h2hip_witness_failure *__restrict__ out) {
    __shared__ uint32_t scan[WC_BLOCK_WORDS];
    const size_t w = (size_t)blockIdx.x * WC_BLOCK_WORDS + threadIdx.x;
    uint32_t bits = w < words ? mask[w] : 0u;
    const uint32_t mine = (uint32_t)__popc(bits);
    scan[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t s = 1; s < WC_BLOCK_WORDS; s <<= 1) {   // inclusive scan (Hillis-Steele)
        const uint32_t add = threadIdx.x >= s ? scan[threadIdx.x - s] : 0u;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    uint64_t rank = prefix[blockIdx.x] + scan[threadIdx.x] - mine;
    while (bits && rank < max) {
        const uint32_t b = (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1;
        const size_t unit = w * 32 + b;
        const uint32_t col = (uint32_t)(unit / seg.stride), row = (uint32_t)(unit % seg.stride);
        h2hip_witness_failure f;
        f.row = row;
        f.peer_column = f.peer_row = 0;
        if (col < seg.gates) {
            f.kind = H2HIP_WITNESS_GATE;
            f.column = gate_report[col];
        } else if (col < seg.gates + seg.lookups) {
            f.kind = H2HIP_WITNESS_LOOKUP;
            f.column = col - seg.gates;
        } else {
            const uint32_t p = col - seg.gates - seg.lookups;
            f.kind = H2HIP_WITNESS_COPY;
            f.column = p;
            f.peer_column = sigma_c[(size_t)p * u + row];
            f.peer_row = sigma_r[(size_t)p * u + row];
        }
        out[rank++] = f;
    }
}

// the key's tuple hash constant (any fixed element: collisions are resolved exactly)
Fr wc_theta() {
    Fr t = Fr::zero();
    t.l[0] = 0x7F4A7C15u;
    t.l[1] = 0x9E3779B9u;
    t.l[2] = 0x85EBCA6Bu;
    return fe_to_mont(t);
}

}  // namespace

int witness_check_run(h2hip_ctx *ctx, const WitnessCheckJob &job, h2hip_witness_failure *failures_out, size_t max_failures, size_t *num_failures) {
    hipStream_t st = ctx->stream;
    const uint32_t u = job.u, G = (uint32_t)job.gate_adv.size(), L = job.num_lookups, M = (uint32_t)job.perm_col.size();
    H2_REQUIRE(u >= 4, "witness check: too few usable rows");
    H2_REQUIRE(G <= 65535 && L <= 65535 && M <= 65535, "witness check: too many columns");
    const uint32_t stride = (u + 31) & ~31u;
    const uint64_t units = (uint64_t)(G + L + M) * stride;
    const size_t words = (size_t)(units / 32), blocks = (words + WC_BLOCK_WORDS - 1) / WC_BLOCK_WORDS;
    // ---- device tables: column pointers, then the index lists
    std::vector<uint32_t> idx;
    auto put = [&](const std::vector<uint32_t> &v) {
        const size_t at = idx.size();
        idx.insert(idx.end(), v.begin(), v.end());
        return at;
    };
    const size_t o_gadv = put(job.gate_adv), o_gq = put(job.gate_q), o_grep = put(job.gate_report), o_lin = put(job.lk_in), o_lq = put(job.lk_q),
                 o_din = put(job.dyn_in), o_dtab = put(job.dyn_tab), o_perm = put(job.perm_col);
    idx.push_back(0);
    const size_t ptr_bytes = sizeof(void *) * job.cols.size(), tab_bytes = (ptr_bytes + 255) / 256 * 256 + sizeof(uint32_t) * idx.size();
    char *tabs = nullptr;
    uint32_t *mask = nullptr, *counts = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP2, tab_bytes, (void **)&tabs));
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP0, sizeof(uint32_t) * words, (void **)&mask));
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP1, sizeof(uint64_t) * (blocks + 1), (void **)&counts));
    const Fr *const *cols = (const Fr *const *)tabs;
    const uint32_t *ix = (const uint32_t *)(tabs + (ptr_bytes + 255) / 256 * 256);
    H2_HIPCHK(hipMemcpyAsync(tabs, job.cols.data(), ptr_bytes, hipMemcpyHostToDevice, st));
    H2_HIPCHK(hipMemcpyAsync((void *)ix, idx.data(), sizeof(uint32_t) * idx.size(), hipMemcpyHostToDevice, st));
    H2_HIPCHK(hipMemsetAsync(mask, 0, sizeof(uint32_t) * words, st));
    const uint32_t gx = (u + WC_THREADS - 1) / WC_THREADS;
    if (G) {
        prof_begin(ctx, "wc_gate_kernel");
        hipLaunchKernelGGL(wc_gate_kernel, dim3(gx, G), dim3(WC_THREADS), 0, st, cols, ix + o_gadv, ix + o_gq, u, stride, mask, G - job.num_rlc_gates,
                           job.num_rlc_gates ? job.rlc_gamma : Fr::zero());
        prof_end(ctx);
    }
    uint32_t *lmask = mask + (size_t)G * stride / 32, *cmask = mask + (size_t)(G + L) * stride / 32;
    if (L && job.dyn_width) {
        const uint32_t N = lookup_padded_keys(u);
        WcKey *keys = nullptr;
        H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_LK3, sizeof(WcKey) * N, (void **)&keys));
        const Fr theta = wc_theta();
        prof_begin(ctx, "wc_dyn_keys_kernel");
        hipLaunchKernelGGL(wc_dyn_keys_kernel, dim3((N + WC_THREADS - 1) / WC_THREADS), dim3(WC_THREADS), 0, st, cols, ix + o_dtab, job.dyn_width, theta, u,
                           N, keys);
        prof_end(ctx);
        H2_CHK(lookup_sort_keys_dev(ctx, keys, N));
        prof_begin(ctx, "wc_lookup_dyn_kernel");
        hipLaunchKernelGGL(wc_lookup_dyn_kernel, dim3(gx, L), dim3(WC_THREADS), 0, st, cols, ix + o_din, ix + o_dtab, job.dyn_width, theta,
                           (const WcKey *)keys, u, stride, lmask);
        prof_end(ctx);
    } else if (L) {
        H2_REQUIRE(job.table_sorted, "witness check: the key has no sorted lookup table");
        prof_begin(ctx, "wc_lookup_range_kernel");
        hipLaunchKernelGGL(wc_lookup_range_kernel, dim3(gx, L), dim3(WC_THREADS), 0, st, cols, ix + o_lin, ix + o_lq, (const WcKey *)job.table_sorted, u,
                           stride, lmask);
        prof_end(ctx);
    }
    if (M) {
        prof_begin(ctx, "wc_copy_kernel");
        hipLaunchKernelGGL(wc_copy_kernel, dim3(gx, M), dim3(WC_THREADS), 0, st, cols, ix + o_perm, job.sigma_c, job.sigma_r, u, stride, cmask);
        prof_end(ctx);
    }
    H2_HIPCHK(hipGetLastError());
    *num_failures = 0;
    if (!blocks) return H2HIP_OK;
    prof_begin(ctx, "wc_count_kernel");
    hipLaunchKernelGGL(wc_count_kernel, dim3((uint32_t)blocks), dim3(WC_BLOCK_WORDS), 0, st, (const uint32_t *)mask, words, counts);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    // ---- round trip 1: the block counts; 64-bit prefixes and the total on the host
    std::vector<uint32_t> cnt(blocks);
    H2_HIPCHK(hipMemcpyAsync(cnt.data(), counts, sizeof(uint32_t) * blocks, hipMemcpyDeviceToHost, st));
    H2_HIPCHK(hipStreamSynchronize(st));
    std::vector<uint64_t> prefix;
    uint64_t total = 0;
    size_t wblocks = 0;   // blocks that hold one of the first max_failures
    for (size_t b = 0; b < blocks; ++b) {
        if (total < max_failures && cnt[b]) wblocks = b + 1;
        if (total < max_failures) prefix.push_back(total);
        total += cnt[b];
    }
    *num_failures = (size_t)total;
    const size_t take = (size_t)std::min<uint64_t>(total, max_failures);
    if (!take) return H2HIP_OK;
    // ---- round trip 2: the first `take` failures in mask (= canonical) order
    h2hip_witness_failure *out = nullptr;
    uint64_t *pre = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_OUT, sizeof(h2hip_witness_failure) * take, (void **)&out));
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_SCAN, sizeof(uint64_t) * wblocks, (void **)&pre));
    H2_HIPCHK(hipMemcpyAsync(pre, prefix.data(), sizeof(uint64_t) * wblocks, hipMemcpyHostToDevice, st));
    prof_begin(ctx, "wc_write_kernel");
    hipLaunchKernelGGL(wc_write_kernel, dim3((uint32_t)wblocks), dim3(WC_BLOCK_WORDS), 0, st, (const uint32_t *)mask, words, (const uint64_t *)pre,
                       (uint64_t)take, WcSegments{G, L, stride}, ix + o_grep, job.sigma_c, job.sigma_r, u, out);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    H2_HIPCHK(hipMemcpyAsync(failures_out, out, sizeof(h2hip_witness_failure) * take, hipMemcpyDeviceToHost, st));
    H2_HIPCHK(hipStreamSynchronize(st));
    return H2HIP_OK;
}

}  // namespace h2
