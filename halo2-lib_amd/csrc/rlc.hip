// RLC columns filled on the device: RlcChip::compute_rlc_fixed_len's cells [UPSTREAM-RECALL: downstream's RlcChip, restated from memory] for
// many chains at once.  A chain over v_0 .. v_{len-1} is the Horner scan r_0 = v_0, r_i = r_{i-1} * gamma + v_i; its cells alternate values
// and running sums (include/h2hip.h states the two piece forms).
//
// The pieces' values form one flat stream (piece after piece, in list order); position p carries the affine map x -> x * m_p + v_p with
// m_p = 0 at the head of a chain and gamma everywhere else, so the running sums are the prefix compositions applied to 0 and a chain's head
// cuts off everything before it without a segment table (and without gamma^-1: gamma = 0 is an ordinary value).  Composition of (m1, a1)
// then (m2, a2) is (m2 m1, a1 m2 + a2).  Three plain launches as the prefix product's (fr_ops.hip) — per tile of 256 lanes x RLC_J values;
// over the tile totals, one workgroup; the tiles' incoming values applied — and one placement kernel driven by the piece table.  No
// workgroup waits for another.
#include "internal.h"

namespace h2 {

constexpr uint32_t RLC_J = 8, RLC_TILE = 256 * RLC_J;
struct RlcPiece {   // a piece as the kernels read it: `start` = its first position in the stream (entry `count` closes the table with the stream's length)
    uint64_t start, value_offset;
    uint32_t column, row, len, flags;
};
struct RlcPair {
    Fr m, a;
};

// the piece that holds stream position p: the last one with start <= p (starts strictly increase: len >= 1)
__device__ __forceinline__ uint32_t rlc_find(const RlcPiece *__restrict__ t, uint32_t count, uint64_t p) {
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t[mid].start <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ bool rlc_is_head(const RlcPiece &pc, uint64_t p) { return p == pc.start && !(pc.flags & H2HIP_RLC_CARRY); }

// inclusive scan of the lanes' maps in LDS (Hillis-Steele, as fr_prefix_prod_tile_kernel's)
template <uint32_t LANES>
__device__ __forceinline__ void rlc_scan_lanes(Fr *shm, Fr *sha, uint32_t tid) {
    for (uint32_t d = 1; d < LANES; d <<= 1) {
        Fr om = Fr::one(), oa = Fr::zero();
        if (tid >= d) {
            om = shm[tid - d];
            oa = sha[tid - d];
        }
        __syncthreads();
        if (tid >= d) {
            const Fr sm = shm[tid];
            sha[tid] = fe_add(fe_mul(oa, sm), sha[tid]);
            shm[tid] = fe_mul(sm, om);
        }
        __syncthreads();
    }
}

// r[p] = the running sum at p as if the tile's incoming value were 0; lane_m = the multiplier the incoming value reaches the lane's first
// position with (0 behind a head); tile_tot = the tile's map
__global__ __launch_bounds__(256) void rlc_scan_tile_kernel(const Fr *__restrict__ values, const RlcPiece *__restrict__ t, uint32_t count, uint64_t total,
                                                            Fr gamma, Fr *__restrict__ r, Fr *__restrict__ lane_m, RlcPair *__restrict__ tile_tot) {
    __shared__ Fr shm[256], sha[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t lane = (uint64_t)blockIdx.x * 256 + tid, base = lane * RLC_J;
    Fr m = Fr::one(), a = Fr::zero();
    uint32_t j0 = 0;
    if (base < total) {
        j0 = rlc_find(t, count, base);
        uint32_t j = j0;
        for (uint32_t k = 0; k < RLC_J && base + k < total; ++k) {
            const uint64_t p = base + k;
            while (p >= t[j + 1].start) ++j;
            const Fr v = values[t[j].value_offset + (p - t[j].start)];
            if (rlc_is_head(t[j], p)) {
                m = Fr::zero();
                a = v;
            } else {
                m = fe_mul(m, gamma);
                a = fe_add(fe_mul(a, gamma), v);
            }
        }
    }
    shm[tid] = m;
    sha[tid] = a;
    __syncthreads();
    rlc_scan_lanes<256>(shm, sha, tid);
    const Fr em = tid ? shm[tid - 1] : Fr::one();
    Fr run = tid ? sha[tid - 1] : Fr::zero();
    lane_m[lane] = em;
    if (base < total) {
        uint32_t j = j0;
        for (uint32_t k = 0; k < RLC_J && base + k < total; ++k) {
            const uint64_t p = base + k;
            while (p >= t[j + 1].start) ++j;
            const Fr v = values[t[j].value_offset + (p - t[j].start)];
            run = rlc_is_head(t[j], p) ? v : fe_add(fe_mul(run, gamma), v);
            r[p] = run;
        }
    }
    if (tid == 255) {
        tile_tot[blockIdx.x].m = shm[255];
        tile_tot[blockIdx.x].a = sha[255];
    }
}
// tile_tot[k].a <- the value that enters tile k (the tiles before it applied to 0); one workgroup
__global__ __launch_bounds__(512) void rlc_scan_sums_kernel(RlcPair *__restrict__ tile_tot, uint32_t ntiles) {
    __shared__ Fr shm[512], sha[512];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ntiles + 511) / 512, lo = tid * per, hi = lo + per < ntiles ? lo + per : ntiles;
    Fr m = Fr::one(), a = Fr::zero();
    for (uint32_t k = lo; k < hi; ++k) {
        const Fr tm = tile_tot[k].m;
        a = fe_add(fe_mul(a, tm), tile_tot[k].a);
        m = fe_mul(m, tm);
    }
    shm[tid] = m;
    sha[tid] = a;
    __syncthreads();
    rlc_scan_lanes<512>(shm, sha, tid);
    Fr run = tid ? sha[tid - 1] : Fr::zero();
    for (uint32_t k = lo; k < hi; ++k) {
        const Fr tm = tile_tot[k].m, ta = tile_tot[k].a;
        tile_tot[k].a = run;
        run = fe_add(fe_mul(run, tm), ta);
    }
}
// r[p] += (the multiplier from the tile's start to p) * (the tile's incoming value), up to the first head behind the lane's start
__global__ __launch_bounds__(256) void rlc_scan_apply_kernel(Fr *__restrict__ r, const Fr *__restrict__ lane_m, const RlcPair *__restrict__ tile_tot,
                                                             const RlcPiece *__restrict__ t, uint32_t count, uint64_t total, Fr gamma) {
    if (blockIdx.x == 0) return;
    const uint64_t lane = (uint64_t)blockIdx.x * 256 + threadIdx.x, base = lane * RLC_J;
    if (base >= total) return;
    Fr c = lane_m[lane];
    if (c.is_zero()) return;
    const Fr inc = tile_tot[blockIdx.x].a;
    uint32_t j = rlc_find(t, count, base);
    for (uint32_t k = 0; k < RLC_J && base + k < total; ++k) {
        const uint64_t p = base + k;
        while (p >= t[j + 1].start) ++j;
        if (rlc_is_head(t[j], p)) return;
        c = fe_mul(c, gamma);
        r[p] = fe_add(r[p], fe_mul(c, inc));
    }
}
// the cells: a head piece's v_0, v_1, r_1, v_2, r_2, ...; a carry piece's r_prev, v_0, r_0', v_1, r_1', ...
__global__ __launch_bounds__(256) void rlc_place_kernel(Fr *const *__restrict__ cols, const Fr *__restrict__ values, const Fr *__restrict__ r,
                                                        const RlcPiece *__restrict__ t, uint32_t count, uint64_t total) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const RlcPiece pc = t[rlc_find(t, count, p)];
        const uint64_t i = p - pc.start;
        Fr *__restrict__ col = cols[pc.column] + pc.row;
        const Fr v = values[pc.value_offset + i];
        if (pc.flags & H2HIP_RLC_CARRY) {
            if (i == 0) col[0] = r[p - 1];   // the break cell, duplicated (a carry piece is never piece 0: p >= 1)
            col[2 * i + 1] = v;
            col[2 * i + 2] = r[p];
        } else if (i == 0) {
            col[0] = v;
        } else {
            col[2 * i - 1] = v;
            col[2 * i] = r[p];
        }
    }
}

}  // namespace h2

using namespace h2;

extern "C" int h2hip_rlc_fill_chains_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const void *values_dev,
                                         size_t num_values, const h2hip_rlc_chain *chains_host, size_t count, const void *gamma) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && gamma && (count == 0 || (chains_host && columns_dev && values_dev)), "NULL argument");
    H2_REQUIRE(count < 0xFFFFFFFFu, "too many pieces");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched
    std::vector<RlcPiece> table(count + 1);
    uint64_t total = 0;
    for (size_t j = 0; j < count; ++j) {
        const h2hip_rlc_chain &c = chains_host[j];
        const bool carry = (c.flags & H2HIP_RLC_CARRY) != 0;
        H2_REQUIRE((c.flags & ~(uint32_t)H2HIP_RLC_CARRY) == 0, "unknown piece flags");
        H2_REQUIRE(c.column < num_columns && columns_dev[c.column], "a piece's column index is out of range (or the column is NULL)");
        H2_REQUIRE(c.len >= 1, "a piece without values (len == 0)");
        H2_REQUIRE(!(carry && j == 0), "piece 0 cannot be a carry piece");
        const uint64_t cells = carry ? 2 * (uint64_t)c.len + 1 : 2 * (uint64_t)c.len - 1;
        H2_REQUIRE((uint64_t)c.row + cells <= usable_rows, "a piece's cells leave the usable rows");
        H2_REQUIRE(c.value_offset <= num_values && c.len <= num_values - c.value_offset, "a piece's values lie outside values_dev");
        table[j] = RlcPiece{total, c.value_offset, c.column, c.row, c.len, c.flags};
        total += c.len;
    }
    table[count] = RlcPiece{total, 0, 0, 0, 0, 0};
    H2_REQUIRE(total <= ((uint64_t)1 << 32), "more than 2^32 values in one call");
    const uint32_t ntiles = (uint32_t)((total + RLC_TILE - 1) / RLC_TILE);
    // ---- workspace: [piece table][column pointers] and [r][lane multipliers][tile totals]
    const size_t table_bytes = sizeof(RlcPiece) * table.size(), ptr_off = (table_bytes + 255) / 256 * 256, ptr_bytes = sizeof(void *) * num_columns;
    char *tabs = nullptr, *scan = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP1, ptr_off + ptr_bytes, (void **)&tabs));
    const size_t r_bytes = sizeof(Fr) * (size_t)total, lm_bytes = sizeof(Fr) * 256 * (size_t)ntiles;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP0, r_bytes + lm_bytes + sizeof(RlcPair) * (size_t)ntiles, (void **)&scan));
    H2_CHK(upload_jobs(ctx, tabs, table.data(), table_bytes));
    H2_CHK(upload_jobs(ctx, tabs + ptr_off, columns_dev, ptr_bytes));
    const RlcPiece *t = (const RlcPiece *)tabs;
    Fr *r = (Fr *)scan, *lane_m = (Fr *)(scan + r_bytes);
    RlcPair *tot = (RlcPair *)(scan + r_bytes + lm_bytes);
    const Fr g = ld_fr(gamma);
    const uint32_t cnt = (uint32_t)count;
    prof_begin(ctx, "rlc_scan_kernels");
    hipLaunchKernelGGL(rlc_scan_tile_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, (const Fr *)values_dev, t, cnt, total, g, r, lane_m, tot);
    hipLaunchKernelGGL(rlc_scan_sums_kernel, dim3(1), dim3(512), 0, ctx->stream, tot, ntiles);
    hipLaunchKernelGGL(rlc_scan_apply_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, r, (const Fr *)lane_m, (const RlcPair *)tot, t, cnt, total, g);
    prof_end(ctx);
    prof_begin(ctx, "rlc_place_kernel");
    hipLaunchKernelGGL(rlc_place_kernel, dim3(grid_for(ctx, (size_t)total)), dim3(256), 0, ctx->stream, (Fr *const *)(tabs + ptr_off), (const Fr *)values_dev,
                       (const Fr *)r, t, cnt, total);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
