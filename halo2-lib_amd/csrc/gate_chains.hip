// Flex-gate chains filled on the device: the cells s_0, a_1, b_1, s_1, a_2, b_2, s_2, ... with s_i = s_{i-1} + a_i * b_i that GateChip's
// inner_product*, sum, select_by_indicator and select_from_idx (and RangeChip's limb recomposition) write [UPSTREAM: flex_gate/mod.rs], for
// many chains at once (include/h2hip.h states the four piece forms).
//
// The pieces' pairs form one flat stream (piece after piece, in list order); position p carries the term e_p = a_p * b_p (a_0 itself at the
// first position of a START_A head) and the bit "a chain starts here".  The running sums are the segmented additive scan of the terms: a head
// cuts off what came before it.  One field element and one bit per position, one product per position.  The host puts the stream position of
// every piece's chain head into the piece table, so no kernel searches backwards for it.  Three plain launches: per tile of 256 lanes x
// GATE_J pairs (the sums as if nothing entered the tile, and the tile's total); over the tile totals, one workgroup (the value that enters
// every tile); and the placement kernel, which adds a tile's incoming value to the positions whose chain began before the tile and writes
// the a, b and s cells per piece form.  No workgroup waits for another; no atomics.
#include "internal.h"
#include "trace_host.h"   // ByteRange, pack_tables

namespace h2 {

constexpr uint32_t GATE_J = 8, GATE_TILE = 256 * GATE_J, GATE_SUMS_LANES = 512;
constexpr uint32_t GATE_FORMS = H2HIP_GATE_CARRY | H2HIP_GATE_JOIN | H2HIP_GATE_START_A;
struct GatePiece {   // a piece as the kernels read it: `start` = its first position in the stream (entry `count` closes the table with the stream's length), `head` = the first position of its chain
    uint64_t start, head, a_offset, b_offset;
    uint32_t column, row, len, flags, a_stride, b_stride;
};

// the piece that holds stream position p: the last one with start <= p (starts strictly increase: len >= 1)
__device__ __forceinline__ uint32_t gate_find(const GatePiece *__restrict__ t, uint32_t count, uint64_t p) {
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t[mid].start <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the term of position p = pc.start + i
__device__ __forceinline__ Fr gate_term(const GatePiece &pc, uint64_t i, const Fr *a, const Fr *b) {
    const Fr av = a[pc.a_offset + i * pc.a_stride];
    if (i == 0 && (pc.flags & H2HIP_GATE_START_A)) return av;
    return fe_mul(av, b[pc.b_offset + i * pc.b_stride]);
}

// inclusive segmented scan of the lanes' (sum, a chain starts in the lane) in LDS (Hillis-Steele)
template <uint32_t LANES>
__device__ __forceinline__ void gate_scan_lanes(Fr *sha, uint32_t *shf, uint32_t tid) {
    for (uint32_t d = 1; d < LANES; d <<= 1) {
        Fr oa = Fr::zero();
        uint32_t of = 0;
        if (tid >= d) {
            oa = sha[tid - d];
            of = shf[tid - d];
        }
        __syncthreads();
        if (tid >= d) {
            if (!shf[tid]) sha[tid] = fe_add(oa, sha[tid]);
            shf[tid] |= of;
        }
        __syncthreads();
    }
}

// s[p] = the running sum at p as if nothing entered the tile; tile_sum / tile_cut = the tile's total and whether a chain starts in it
__global__ __launch_bounds__(256) void gate_scan_tile_kernel(const Fr *a, const Fr *b, const GatePiece *__restrict__ t, uint32_t count, uint64_t total,
                                                             Fr *__restrict__ s, Fr *__restrict__ tile_sum, uint32_t *__restrict__ tile_cut) {
    __shared__ Fr sha[256];
    __shared__ uint32_t shf[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = ((uint64_t)blockIdx.x * 256 + tid) * GATE_J;
    Fr acc = Fr::zero();
    uint32_t cut = 0, j0 = 0;
    if (base < total) {
        j0 = gate_find(t, count, base);
        uint32_t j = j0;
        for (uint32_t k = 0; k < GATE_J && base + k < total; ++k) {
            const uint64_t p = base + k;
            while (p >= t[j + 1].start) ++j;
            const Fr e = gate_term(t[j], p - t[j].start, a, b);
            if (p == t[j].head) {
                acc = e;
                cut = 1;
            } else {
                acc = fe_add(acc, e);
            }
        }
    }
    sha[tid] = acc;
    shf[tid] = cut;
    __syncthreads();
    gate_scan_lanes<256>(sha, shf, tid);
    Fr run = tid ? sha[tid - 1] : Fr::zero();
    if (base < total) {
        uint32_t j = j0;
        for (uint32_t k = 0; k < GATE_J && base + k < total; ++k) {
            const uint64_t p = base + k;
            while (p >= t[j + 1].start) ++j;
            const Fr e = gate_term(t[j], p - t[j].start, a, b);
            run = p == t[j].head ? e : fe_add(run, e);
            s[p] = run;
        }
    }
    if (tid == 255) {
        tile_sum[blockIdx.x] = sha[255];
        tile_cut[blockIdx.x] = shf[255];
    }
}
// tile_sum[k] <- the sum that enters tile k (the tiles before it, from the last chain start among them); one workgroup, every lane a run of tiles
__global__ __launch_bounds__(GATE_SUMS_LANES) void gate_scan_sums_kernel(Fr *__restrict__ tile_sum, const uint32_t *__restrict__ tile_cut, uint32_t ntiles) {
    __shared__ Fr sha[GATE_SUMS_LANES];
    __shared__ uint32_t shf[GATE_SUMS_LANES];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ntiles + GATE_SUMS_LANES - 1) / GATE_SUMS_LANES;
    const uint32_t lo = tid * per < ntiles ? tid * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    Fr acc = Fr::zero();
    uint32_t cut = 0;
    for (uint32_t k = lo; k < hi; ++k) {
        acc = tile_cut[k] ? tile_sum[k] : fe_add(acc, tile_sum[k]);
        cut |= tile_cut[k];
    }
    sha[tid] = acc;
    shf[tid] = cut;
    __syncthreads();
    gate_scan_lanes<GATE_SUMS_LANES>(sha, shf, tid);
    Fr run = tid ? sha[tid - 1] : Fr::zero();
    for (uint32_t k = lo; k < hi; ++k) {
        const Fr ts = tile_sum[k];
        tile_sum[k] = run;
        run = tile_cut[k] ? ts : fe_add(run, ts);
    }
}
// the final running sum at p, in the piece pc: the tile's incoming value reaches p when p's chain began before the tile
__device__ __forceinline__ Fr gate_sum_at(const Fr *__restrict__ s, const Fr *__restrict__ tile_in, uint64_t head, uint64_t p) {
    const uint64_t tile = p / GATE_TILE;
    return head < tile * GATE_TILE ? fe_add(s[p], tile_in[tile]) : s[p];
}
// the cells of every piece form (include/h2hip.h); a_dev / b_dev may point into the columns (at cells this call does not write: the host checked)
__global__ __launch_bounds__(256) void gate_place_kernel(Fr *const *__restrict__ cols, const Fr *a, const Fr *b, const Fr *__restrict__ s,
                                                         const Fr *__restrict__ tile_in, const GatePiece *__restrict__ t, uint32_t count, uint64_t total) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const GatePiece pc = t[gate_find(t, count, p)];
        const uint64_t i = p - pc.start;
        Fr *col = cols[pc.column] + pc.row;
        const Fr av = a[pc.a_offset + i * pc.a_stride];
        const Fr sum = gate_sum_at(s, tile_in, pc.head, p);
        if (pc.flags & H2HIP_GATE_START_A) {
            if (i == 0) {
                col[0] = av;   // s_0 = a_0; b_0 is not read
                continue;
            }
            col += 3 * i - 2;
        } else if (pc.flags & H2HIP_GATE_JOIN) {
            col += 3 * i;
        } else {
            if (i == 0) col[0] = (pc.flags & H2HIP_GATE_CARRY) ? gate_sum_at(s, tile_in, pc.head, p - 1) : Fr::zero();   // the break cell, duplicated (a carry piece is never piece 0: p >= 1)
            col += 3 * i + 1;
        }
        col[0] = av;
        col[1] = b[pc.b_offset + i * pc.b_stride];
        col[2] = sum;
    }
}

}  // namespace h2

using namespace h2;

extern "C" int h2hip_gate_fill_chains_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const void *a_dev, size_t a_len,
                                          const void *b_dev, size_t b_len, const h2hip_gate_chain *chains_host, size_t count) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (count == 0 || (chains_host && columns_dev && a_dev && b_dev)), "NULL argument");
    H2_REQUIRE(count < 0xFFFFFFFFu, "too many pieces");
    if (!count) return H2HIP_OK;
    // ---- every check before anything is launched or uploaded
    H2_REQUIRE(a_len <= SIZE_MAX / sizeof(Fr) && b_len <= SIZE_MAX / sizeof(Fr), "a_len / b_len is no count of field elements");
    std::vector<GatePiece> table(count + 1);
    std::vector<ByteRange> written(count), a_reads(count), b_reads;
    b_reads.reserve(count);
    uint64_t total = 0, prev_cells = 0;
    for (size_t j = 0; j < count; ++j) {
        const h2hip_gate_chain &c = chains_host[j];
        const uint32_t form = c.flags & GATE_FORMS;
        H2_REQUIRE((c.flags & ~GATE_FORMS) == 0, "unknown piece flags");
        H2_REQUIRE((form & (form - 1)) == 0, "more than one of CARRY / JOIN / START_A on a piece");
        H2_REQUIRE(!(j == 0 && (form & (H2HIP_GATE_CARRY | H2HIP_GATE_JOIN))), "piece 0 cannot be a carry or a join piece");
        H2_REQUIRE(c.len >= 1, "a piece without pairs (len == 0)");
        H2_REQUIRE(c.column < num_columns && columns_dev[c.column], "a piece's column index is out of range (or the column is NULL)");
        const uint64_t len = c.len;
        const uint64_t cells = form == H2HIP_GATE_START_A ? 3 * len - 2 : form == H2HIP_GATE_JOIN ? 3 * len : 3 * len + 1;
        H2_REQUIRE((uint64_t)c.row + cells <= usable_rows, "a piece's cells leave the usable rows");
        if (form == H2HIP_GATE_JOIN) {
            const h2hip_gate_chain &q = chains_host[j - 1];
            H2_REQUIRE(c.column == q.column && (uint64_t)c.row == (uint64_t)q.row + prev_cells,
                       "a join piece does not start at the row after the last cell of the piece before it, in its column");
        }
        // operand indices in 64 bits: (len - 1) * stride < 2^64, and the sum is checked against a_len / b_len without wrapping
        const uint64_t a_span = (len - 1) * c.a_stride, b_first = form == H2HIP_GATE_START_A ? 1 : 0, b_span = (len - 1) * c.b_stride;
        H2_REQUIRE(c.a_offset < a_len && a_span < a_len - c.a_offset, "a piece's left operands lie outside a_len");
        if (b_first < len) {   // (a START_A piece of one pair reads no right operand)
            H2_REQUIRE(c.b_offset < b_len && b_span < b_len - c.b_offset, "a piece's right operands lie outside b_len");
            const uintptr_t lo = (uintptr_t)b_dev + sizeof(Fr) * (c.b_offset + b_first * c.b_stride);
            b_reads.push_back(ByteRange{lo, (uintptr_t)b_dev + sizeof(Fr) * (c.b_offset + b_span + 1)});
        }
        a_reads[j] = ByteRange{(uintptr_t)a_dev + sizeof(Fr) * c.a_offset, (uintptr_t)a_dev + sizeof(Fr) * (c.a_offset + a_span + 1)};
        const uintptr_t w = (uintptr_t)columns_dev[c.column] + sizeof(Fr) * (uint64_t)c.row;
        written[j] = ByteRange{w, w + sizeof(Fr) * cells};
        const uint64_t head = form & (H2HIP_GATE_CARRY | H2HIP_GATE_JOIN) ? table[j - 1].head : total;
        table[j] = GatePiece{total, head, c.a_offset, c.b_offset, c.column, c.row, c.len, c.flags, c.a_stride, c.b_stride};
        total += len;
        prev_cells = cells;
    }
    table[count] = GatePiece{total, total, 0, 0, 0, 0, 0, 0, 0, 0};
    H2_REQUIRE(total <= ((uint64_t)1 << 32), "more than 2^32 pairs in one call");
    // the cells of two pieces are disjoint, and no operand range (first to last address read, whatever the stride) meets a written cell:
    // address intervals, sorted (a layout engine's pieces mostly arrive sorted) and swept
    const char *clash = byte_ranges_clash(written, {&a_reads, &b_reads}, "two pieces' cells overlap");
    H2_REQUIRE(!clash, clash);
    const uint32_t ntiles = (uint32_t)((total + GATE_TILE - 1) / GATE_TILE);
    // ---- workspace: [piece table][column pointers] and [s][tile sums][tile cuts]
    DevTables tabs;
    char *scan = nullptr;
    const size_t s_bytes = sizeof(Fr) * (size_t)total, sum_bytes = sizeof(Fr) * (size_t)ntiles;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP0, s_bytes + sum_bytes + sizeof(uint32_t) * (size_t)ntiles, (void **)&scan));
    H2_CHK(pack_tables(ctx, {{table.data(), sizeof(GatePiece) * table.size()}, {columns_dev, sizeof(void *) * num_columns, HostTable::COLUMNS}}, tabs));
    const GatePiece *t = (const GatePiece *)tabs.at[0];
    Fr *s = (Fr *)scan, *tile_sum = (Fr *)(scan + s_bytes);
    uint32_t *tile_cut = (uint32_t *)(scan + s_bytes + sum_bytes);
    const uint32_t cnt = (uint32_t)count;
    prof_begin(ctx, "gate_scan_kernels");
    hipLaunchKernelGGL(gate_scan_tile_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, (const Fr *)a_dev, (const Fr *)b_dev, t, cnt, total, s, tile_sum, tile_cut);
    hipLaunchKernelGGL(gate_scan_sums_kernel, dim3(1), dim3(GATE_SUMS_LANES), 0, ctx->stream, tile_sum, (const uint32_t *)tile_cut, ntiles);
    prof_end(ctx);
    prof_begin(ctx, "gate_place_kernel");
    hipLaunchKernelGGL(gate_place_kernel, dim3(grid_for(ctx, (size_t)total)), dim3(256), 0, ctx->stream, tabs.tc.cols, (const Fr *)a_dev,
                       (const Fr *)b_dev, (const Fr *)s, (const Fr *)tile_sum, t, cnt, total);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}
