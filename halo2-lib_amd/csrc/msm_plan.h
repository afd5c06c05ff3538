// The MSM's host-side DECISIONS, apart from their execution: which window, how the counting sort is chunked, how many entries an accumulation
// lane owns, how a batch is dealt to lanes and fused groups — every geometry rule the r03 - r06 measurements paid for, as pure functions of
// (knobs, base set, sizes).  Host-only and free of HIP calls: msm.hip / msm_batch.hip execute a plan, tests/emu/msm_plan_selftest.cpp prints
// plans on a hand-filled context and compares them with the values recorded before the planners existed (tests/golden/msm_plan_cases.json).
#pragma once
#include "internal.h"

namespace h2 {

constexpr uint32_t MAX_LDS_BUCKETS = 1u << 15;   // the sort kernels' dynamic LDS limit: 128 KiB of u32 counters
constexpr size_t MSM_DIGIT_BYTES = 2;            // sizeof(digit_t), msm.hip

// Window size by a cost model in field multiplications.  Plain bases: every window has its own bucket set, reduced at
// ~28 multiplications per bucket.  Precomputed tables: ONE bucket set, but its reduction is a chain of dependent
// additions whose latency is worth ~150 multiplications of the (parallel) accumulation per bucket — fitted to the
// measured optimum c = 13/14 at 2^16, 15/16 at 2^18, 16 at 2^19 and above (tools/c_sweep.sh).
inline uint32_t pick_window(size_t n, bool precomp = false) {
    uint32_t best = 4;
    double best_cost = 1e300;
    for (uint32_t c = 4; c <= 16; ++c) {
        double W = (double)((255 + c - 1) / c);
        // precomputed tables: W*n mixed additions; every (window, bucket) pair costs a full addition in the per-index presum plus its share of
        // the run boundaries, zero fill and merge (~34 products' worth, fitted on proofs of 2^14..2^17-row shapes: tools/prove_time.py
        // --param=msm_window_bits=..); the running sums over one bucket set per column come last
        const double B = (double)(1u << (c - 1));
        double cost = precomp ? W * 10.0 * (double)n + W * B * 34.0 + 60.0 * B
                              : W * (10.0 * (double)n + 28.0 * B + 400.0 * c);
        if (cost < best_cost) {
            best_cost = cost;
            best = c;
        }
    }
    return best;
}

// workgroup -> (window, chunk).  Workgroups are dealt round-robin to the 8 XCDs, each XCD works through its own sequence in order: the first
// 8 * floor(total / 8) windows are pinned — window w lives on XCD (w mod 8), its G chunk workgroups run together there, one window after the
// other — so that a window's slice of the sorted array stays in ONE 4 MiB L2 while it is written.  The total % 8 windows left over (17 windows:
// one) are dealt chunk by chunk over all XCDs: pinned too, the 17th window was a third round on XCD 0 alone with seven XCDs idle (2.1 rounds of
// work in the time of 3); its 4-byte writes now combine per XCD only (1/17 of the entries).  (block_to_window_chunk, msm.hip, is the inverse.)
inline uint32_t sort_grid_size(uint32_t total, uint32_t G) {
    const uint32_t full = total / 8u, rem = total - 8u * full;
    return 8u * (full * G + (rem * G + 7u) / 8u);
}

inline uint32_t msm_windows(uint32_t c) { return (255 + c - 1) / c; }                                    // windows of one column
inline size_t msm_keys_per_col(uint32_t c) { return (size_t)msm_windows(c) << (c - 1); }               // bucket slots of one column: one set of 2^(c-1) per window

// Everything msm_run_cols decides for one (fused multi-column) MSM of n > 0 scalars per column.
struct MsmPlan {
    size_t n = 0;               // scalars per column; 0: an empty MSM, nothing else is set
    uint32_t ncols = 0;
    bool precomp = false;       // window tables: every column owns one bucket set after the per-index presum
    uint32_t c = 0;             // window bits
    uint32_t Wcol = 0, W = 0;   // windows of one column / windows the sort and the accumulation see (Wcol * ncols)
    uint32_t B = 0;             // buckets per window
    uint32_t nkeys = 0;         // keys of the counting sort = run keys of the accumulation = bucket slots (W * B)
    uint64_t emax = 0;          // entries: n * W
    uint32_t K1 = 0;            // entries per accumulation lane
    uint32_t chunk = 0, G = 0;  // scalars per sort chunk, chunks per window
    uint32_t sort_threads = 0;
    bool hist_packed = false;   // 16-bit counter pairs in the LDS histogram
    uint32_t HS = 0, hist_grid = 0;
    size_t hist_lds = 0;
    uint32_t S = 0, scatter_grid = 0;   // bucket sub-ranges per window in the scatter
    size_t scatter_lds = 0;
    uint32_t table_stride = 0;  // scatter: entries between two windows' tables (precomputed bases), else 0
    uint32_t T1 = 0, accum_blocks = 0;   // accumulation lanes / workgroups
    uint32_t len1 = 0, blocks1 = 0;      // partials the accumulation leaves, workgroups of the first merge level
    // bytes of every workspace slot, in the order they are reserved
    size_t digits_bytes = 0, bhist_bytes = 0, counts_bytes = 0, offsets_bytes = 0, sval_bytes = 0, buckets_bytes = 0, pkey0_bytes = 0, pval0_bytes = 0,
           pkey1_bytes = 0, pval1_bytes = 0;
};

inline int msm_plan(const h2hip_ctx &ctx, const h2hip_bases &bases, size_t n, uint32_t ncols, MsmPlan *out) {
    static const char *const drv = "msm_run_cols";   // the driver the checks were written in, and report under
    MsmPlan p;
    H2_REQUIRE_AS(drv, ncols >= 1 && ncols <= MSM_MAX_COLS, "1..32 columns per fused MSM");
    H2_REQUIRE_AS(drv, n <= bases.n, "more scalars than resident bases");
    H2_REQUIRE_AS(drv, bases.pts29 != nullptr || bases.n == 0, "bases are not prepared");
    H2_REQUIRE_AS(drv, n < (1u << 27), "n too large for 32-bit entry indices");
    p.ncols = ncols;
    if (n == 0) {
        *out = p;
        return H2HIP_OK;
    }
    p.n = n;
    p.precomp = bases.tables > 1;
    H2_REQUIRE_AS(drv, ncols == 1 || p.precomp, "a fused multi-column MSM needs precomputed bases");
    p.c = p.precomp ? bases.window_bits : (ctx.msm_window_bits ? (uint32_t)ctx.msm_window_bits : pick_window(n));
    H2_REQUIRE_AS(drv, p.c >= 2 && p.c <= 16, "window bits must be 2..16 (a window's bucket histogram lives in LDS)");
    p.Wcol = msm_windows(p.c);
    H2_REQUIRE_AS(drv, p.Wcol <= 64, "too many windows");
    H2_REQUIRE_AS(drv, !p.precomp || bases.tables >= p.Wcol, "precomputed table has too few windows");
    p.W = p.Wcol * ncols;
    p.B = 1u << (p.c - 1);
    p.nkeys = p.W * p.B;
    p.emax = (uint64_t)n * p.W;
    H2_REQUIRE_AS(drv, p.emax < 0xFFFFFFF0ull, "n*W overflows 32 bits");
    p.K1 = (uint32_t)ctx.msm_chunk;
    if (p.K1 == 0) {   // auto: as long as possible (fewer shared runs to merge) while the grid is still several waves per SIMD
        // Measured at 2^19 / 17 windows (tools/msm_r03.py): 34 entries per lane = 4096 waves 0.72 ms; 32 = 4352 waves 0.81 ms; 64 = 2176 waves
        // 0.98 ms; ONE exact round of two waves per SIMD (68 entries = 2048 waves) 0.72 ms although its wave-level merge is a single
        // addition per lane — with one round the kernel ends with its slowest wave, shorter lanes in several rounds balance themselves.
        // r06, re-measured in whole proofs with the sort kernels running beside the accumulations (profiles/r06_msm_chunk_ab.log): shorter lanes — more,
        // shorter accumulation workgroups, whose retiring gives the next column's sort its slots sooner — win up to 2^20 points: 24 entries per lane
        // -0.7 ... -1.3 % at k = 19, -1.6 % at k = 18, -3 % at k = 17 (four fused columns), -4 % at k = 16; 2^20 points: 32 (-1.5 ... -3 %; 48: +3 %); from 2^21
        // points the longest lanes stay best (56 / 48 / 32: +1 % / neutral / +1.3 %)
        uint64_t k = p.emax / 262144;
        p.K1 = k < 8 ? 8u : k > 64 ? 64u : (uint32_t)k;
        const bool lone = !ctx.is_lane && ctx.msm_chunk_lone != 0;   // a lone MSM (SHPLONK's W, W'): no other column's sort waits for its slots
        if (lone) {   // r05's rule stays: alone, 34 entries per lane are 1 - 3 % faster than 24 at 2^19 points (warm: sync MSM 1.09 - 1.12 vs 1.12 - 1.13 ms, accumulation 0.70 vs 0.72 - 0.78)
            if (ctx.msm_chunk_lone > 0) p.K1 = (uint32_t)ctx.msm_chunk_lone;
        } else if (p.emax >= 25000000ull) p.K1 = 64;
        else if (p.emax >= 12000000ull) p.K1 = 32;
        else if (p.emax >= 4000000ull) p.K1 = 24;
    }
    // chunking of the counting sort: about 32 chunks per window, 4Ki..64Ki scalars each.  32 = the CUs of an XCD: the (window, chunk)
    // workgroups of one window run together on the window's XCD, one per CU (tried: chunks sized for ONE round over the whole chip,
    // W * G <= CUs — 2^19: scatter 0.081 -> 0.145 ms, 2^20: 0.154 -> 0.242 ms: half of every XCD's CUs idle and three windows' slices
    // competing for one 4 MiB L2).
    // (r06 tried choosing the chunk count so that windows x chunks fills whole rounds of the chip's 2 x CUs sort-workgroup slots — 30 at 17 windows: 510
    // workgroups instead of 544 — on the theory that the 32 left-over workgroups cost a round: warm, a synchronous 2^19-point MSM is 1.08 ms either way
    // and whole proofs do not move (profiles/r06_sort_groups_ab.log; the first sweep's 1.20 -> 1.09 ms was the tool's cold first measurement).  The
    // knob stays: msm_sort_groups, 0 = 32.)
    const uint32_t sort_groups = ctx.msm_sort_groups > 0 ? (uint32_t)ctx.msm_sort_groups : 32u;
    p.chunk = (uint32_t)((n + sort_groups - 1) / sort_groups);
    if (p.chunk < 4096) p.chunk = 4096;
    const uint32_t chunk_cap = ctx.msm_hist_packed ? 65535u : 65536u;   // (r06) a packed histogram counter holds at most 65535: 2^21 points sort as 33 chunks
    if (p.chunk > chunk_cap) p.chunk = chunk_cap;
    p.G = (uint32_t)((n + p.chunk - 1) / p.chunk);
    p.sort_threads = (uint32_t)ctx.msm_sort_threads;
    p.hist_packed = ctx.msm_hist_packed != 0 && p.chunk < 65536u && p.B >= 2;   // (a counter holds at most `chunk`)
    // bucket sub-ranges per window (msm_hist_split, default 1): two 32 KiB sub-ranges at c = 16 would fit one retiring accumulation workgroup's slot where
    // the 64 KiB window needs two — measured: k = 21 / 22 proofs unchanged, k = 20 +0.5 %, a synchronous 2^20-point MSM +4 % (profiles/r06_hist_split_ab.log)
    p.HS = ctx.msm_hist_split > 0 ? (uint32_t)ctx.msm_hist_split : 1u;
    if (p.HS > p.B) p.HS = p.B;
    p.hist_grid = sort_grid_size(p.W * p.HS, p.G);
    p.hist_lds = p.hist_packed ? sizeof(uint32_t) * ((p.B / p.HS + 1) / 2) : sizeof(uint32_t) * (p.B / p.HS);
    p.S = (uint32_t)ctx.msm_scatter_split;   // sub-ranges per window: keep a segment's output slice (n*4/S bytes) within ~2 MiB
    if (p.S == 0) {
        p.S = 1;
        while (p.S < 4 && p.S * 2 <= p.B && ((uint64_t)n * 4) / p.S > (2u << 20)) p.S *= 2;
    }
    if (p.S > p.B) p.S = p.B;
    p.scatter_grid = sort_grid_size(p.W * p.S, p.G);
    p.scatter_lds = ctx.msm_scatter_full_lds ? sizeof(uint32_t) * MAX_LDS_BUCKETS : sizeof(uint32_t) * (p.B / p.S);   // full 128 KiB: one workgroup per CU keeps a segment's writes on one XCD
    p.table_stride = p.precomp ? (uint32_t)bases.n : 0u;
    p.T1 = (uint32_t)((p.emax + p.K1 - 1) / p.K1);
    p.accum_blocks = (p.T1 + 255) / 256;
    p.len1 = 8 * p.accum_blocks;   // the accumulation leaves two partial slots per wave (4 waves per workgroup)
    p.blocks1 = (p.len1 + 255) / 256;
    p.digits_bytes = MSM_DIGIT_BYTES * p.emax;
    p.bhist_bytes = sizeof(uint32_t) * (size_t)p.W * p.G * p.B;
    p.counts_bytes = sizeof(uint32_t) * ((size_t)p.nkeys + 1);
    p.offsets_bytes = sizeof(uint32_t) * ((size_t)p.nkeys + 2);
    p.sval_bytes = sizeof(uint32_t) * (p.emax + 4);   // + 4: the accumulation reads aligned 16-byte groups
    p.buckets_bytes = sizeof(XYZZ29) * p.nkeys;
    p.pkey0_bytes = sizeof(uint32_t) * (size_t)p.len1;
    p.pval0_bytes = sizeof(XYZZ29) * (size_t)p.len1;
    p.pkey1_bytes = sizeof(uint32_t) * 2 * (size_t)p.blocks1;
    p.pval1_bytes = sizeof(XYZZ29) * 2 * (size_t)p.blocks1;
    *out = p;
    return H2HIP_OK;
}

// What msm_batch decides for `count` columns of n scalars each.
struct BatchMsmPlan {
    size_t n = 0, count = 0;    // count == 0: an empty batch, nothing else is set
    bool affine = false;
    size_t point_bytes = 0;     // one result
    bool precomp = false;
    int NL = 0;                 // lanes that carry columns
    int lane_ctxs = 0;          // lane contexts that have to exist (the prover's side work runs on the last one)
    size_t fuse = 1;            // columns per fused multi-column MSM, at most
    struct Group {
        size_t first, size;     // columns [first, first + size): one fused MSM over one base set, on lane (index % NL)
        bool sort_waits;        // (msm_stagger_sorts) its sort starts behind the previous group's (the previous lane's sorted_ev) ...
        bool sort_signals;      // ... and the next group's behind its own
    };
    std::vector<Group> groups;
    size_t keys_per_col = 0;    // precomputed bases: bucket slots a column leaves for the deferred reduction
    bool deferred = false;      // the columns stop after their merge; one bucket reduction per 64 columns after the lanes have joined
    size_t buckets_bytes = 0;   // deferred: the shared bucket array
    bool stagger = false;       // the first round of groups sorts one after the other
};

// bases_per_col (optional): a base set per column; `bases` is then ignored
inline int msm_batch_plan(const h2hip_ctx &ctx, const h2hip_bases *bases, const h2hip_bases *const *bases_per_col, size_t n, size_t count,
                          int point_format, BatchMsmPlan *out) {
    static const char *const drv = "msm_batch";
    BatchMsmPlan p;
    if (bases_per_col && count) bases = bases_per_col[0];
    if (bases_per_col)
        for (size_t j = 0; j < count; ++j) {
            H2_REQUIRE_AS(drv, bases_per_col[j] && n <= bases_per_col[j]->n, "NULL base set / more scalars than bases");
            H2_REQUIRE_AS(drv, (bases_per_col[j]->tables > 1) == (bases->tables > 1) && bases_per_col[j]->window_bits == bases->window_bits,
                            "the base sets of one batch must share their table layout (plain, or precomputed with the same window)");
        }
    auto bases_of = [&](size_t j) -> const h2hip_bases * { return bases_per_col ? bases_per_col[j] : bases; };
    H2_REQUIRE_AS(drv, point_format == H2HIP_POINT_JACOBIAN || point_format == H2HIP_POINT_AFFINE, "unknown point_format");
    if (!count) {
        *out = p;
        return H2HIP_OK;
    }
    H2_REQUIRE_AS(drv, n <= bases->n, "more scalars than bases");
    p.n = n;
    p.count = count;
    p.affine = point_format == H2HIP_POINT_AFFINE;
    p.point_bytes = p.affine ? sizeof(G1Affine) : sizeof(G1Jac);
    // lanes: the kernels of one MSM are issue-bound or latency-bound, so lanes that overlap whole MSMs mostly contend (measured,
    // tools/batch_ab.py, batches of 4 with the deferred reduction: 2^20 1.71 / 1.75 / 1.80 / 1.84 ms per MSM on 1 / 2 / 3 / 4 lanes, 2^19
    // 0.99 / 0.95 / 0.98 / 1.00: r02's kernels) — auto picks 2 lanes from 2^20 points (r04, measured in proofs), 3 below
    p.NL = ctx.msm_lanes;
    if (p.NL <= 0) p.NL = n >= ((size_t)1 << 20) ? 2 : 3;   // (2^18 / 2^19 were on 2 lanes until the window model moved them to c = 15: 3 lanes now win by 2 %, k = 18 / 19 proofs;
                                                            //  r04: 2^21 on 2 lanes 60.3 ms per k = 21 proof against 62.2 on one and 61.0 on three — the next column's sort
                                                            //  runs beside the accumulation: profiles/archive/r04_msm_lanes_large.log)
    if (p.NL > 4) p.NL = 4;
    // (a third context exists even where only two lanes carry columns: the prover's side transforms run on the LAST lane's context, and with two
    // lanes a context of their own ended up behind the grand products on a shared hardware queue — k = 21: the products waited 3.5 ms for
    // the transforms they were meant to run beside, profiles/archive/r04_timeline_k21.md)
    p.lane_ctxs = p.NL < 3 ? 3 : p.NL;
    // Precomputed bases, two shapes (measured, tools/fuse_sweep*.sh):
    //  * up to 2^17 points: columns are FUSED into groups that go through the whole pipeline as one multi-column MSM;
    //  * larger: every column runs its own sort / accumulation / merge on a lane (pipelined), and the latency-bound
    //    bucket reduction is DEFERRED: it runs once, for all columns together, after the lanes have joined.
    p.precomp = bases->tables > 1;
    p.fuse = p.precomp ? (size_t)ctx.msm_fuse_cols : 1;
    if (p.precomp && ctx.msm_fuse_cols == 0) {   // auto: about 2^19 scalars per fused MSM, at most 16 columns (2^17: 4, 2^16: 8, <= 2^15: 16); larger sizes run one by one
        p.fuse = 1;
        if (n <= ((size_t)1 << 17))
            while (p.fuse < 16 && p.fuse * 2 * (n ? n : 1) <= ((size_t)1 << 19)) p.fuse *= 2;
    }
    if (p.fuse < 1) p.fuse = 1;
    if (p.fuse > MSM_MAX_COLS) p.fuse = MSM_MAX_COLS;
    // groups of columns that go through the pipeline as one fused MSM: a fused MSM reads one table, so a group never spans two base sets
    // (runs of columns over the same set are split into balanced groups of at most `fuse`)
    for (size_t r0 = 0; r0 < count;) {
        size_t r1 = r0 + 1;
        while (r1 < count && bases_of(r1) == bases_of(r0)) ++r1;
        const size_t run = r1 - r0, ng = (run + p.fuse - 1) / p.fuse;
        for (size_t g = 0, j = r0; g < ng; ++g) {
            const size_t gs = (r1 - j + (ng - g) - 1) / (ng - g);
            p.groups.push_back({j, gs, false, false});
            j += gs;
        }
        r0 = r1;
    }
    // deferred bucket reduction: every column (or fused group of columns) stops after its merge and leaves its buckets in one array; the
    // latency-bound reduction then runs once per 64 columns for the whole batch instead of once per MSM / group
    if (p.precomp) p.keys_per_col = msm_keys_per_col(bases->window_bits);
    p.deferred = p.precomp && ctx.msm_defer_reduce && count >= 2 && n > 0 && (p.fuse == 1 ? count <= 64 : true) &&
                 sizeof(XYZZ29) * p.keys_per_col * count <= ((size_t)2 << 30);
    if (p.deferred) p.buckets_bytes = sizeof(XYZZ29) * p.keys_per_col * count;
    // the first round of columns: lane g sorts behind lane g - 1's sort
    p.stagger = (ctx.msm_stagger_sorts > 0 || (ctx.msm_stagger_sorts < 0 && p.NL == 2)) && p.precomp && p.fuse == 1;
    for (size_t g = 0; p.stagger && g < p.groups.size() && g < (size_t)p.NL; ++g) {
        p.groups[g].sort_waits = g > 0;
        p.groups[g].sort_signals = g + 1 < (size_t)p.NL && g + 1 < p.groups.size();
    }
    *out = p;
    return H2HIP_OK;
}

}  // namespace h2
