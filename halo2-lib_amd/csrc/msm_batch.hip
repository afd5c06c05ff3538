// The MSM's C ABI and its batch driver: resident base sets, h2hip_msm_g1* (one MSM, or a batch of columns pipelined over lanes) and the
// Jacobian point sums.  What a batch does — lanes, fused groups, the deferred reduction, staggered sorts — is BatchMsmPlan's decision
// (msm_plan.h); this file queues it.
#include "msm_plan.h"

namespace h2 {

// workgroup b: in[b] -> slot first_slot + b of the result array
__global__ void point_finish_slot_kernel(const XYZZ *__restrict__ in, G1Jac *__restrict__ jac, G1Affine *__restrict__ aff, uint32_t first_slot) {
    if (threadIdx.x == 0) {
        XYZZ p = in[blockIdx.x];
        if (jac) jac[first_slot + blockIdx.x] = xyzz_to_jacobian(p);
        if (aff) aff[first_slot + blockIdx.x] = xyzz_to_affine(p);
    }
}

// sum of n Jacobian points (multi-GPU partial results): one workgroup, strided accumulate + LDS tree
__global__ __launch_bounds__(64) void jac_sum_kernel(const G1Jac *__restrict__ pts, uint32_t n, XYZZ *__restrict__ out) {
    __shared__ XYZZ sh[64];
    uint32_t tid = threadIdx.x;
    XYZZ acc = XYZZ::identity();
    for (uint32_t i = tid; i < n; i += 64) {
        G1Jac p = pts[i];
        if (p.z.is_zero()) continue;
        XYZZ q;
        q.x = p.x;
        q.y = p.y;
        q.zz = fe_sqr(p.z);
        q.zzz = fe_mul(q.zz, p.z);
        xyzz_add(acc, q);
    }
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        if (tid < d) {
            XYZZ a = sh[tid];
            xyzz_add(a, sh[tid + d]);
            sh[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) out[0] = sh[0];
}

// in[b] -> slot first_slot + b of `results` (affine or Jacobian points), b < count, on c's stream
static void finish_slots(h2hip_ctx *c, const XYZZ *in, void *results, size_t count, size_t first_slot, bool affine) {
    prof_begin(c, "point_finish_kernel");
    hipLaunchKernelGGL(point_finish_slot_kernel, dim3((uint32_t)count), dim3(64), 0, c->stream, in, affine ? (G1Jac *)nullptr : (G1Jac *)results,
                       affine ? (G1Affine *)results : (G1Affine *)nullptr, (uint32_t)first_slot);
    prof_end(c);
}
// outbuf (WS_OUT, 1 KiB): [0] the sum as the MSM left it, [256] / [512] the Jacobian / affine point that goes back to the host
static int finish_point(h2hip_ctx *ctx, char *outbuf, int point_format, void *out_host) {
    const bool affine = point_format == H2HIP_POINT_AFFINE;
    void *res = outbuf + (affine ? 512 : 256);
    finish_slots(ctx, (const XYZZ *)outbuf, res, 1, 0, affine);
    H2_HIPCHK(hipGetLastError());
    return sync_results(ctx, out_host, res, affine ? sizeof(G1Affine) : sizeof(G1Jac));
}

// Several independent MSMs over the same bases (e.g. the h(X) pieces, or all advice columns of a phase): MSM j runs
// on lane j mod 2 — a child context with its own stream and scratch — so the latency-bound tail of one MSM (merge,
// bucket reduction) overlaps the multiplier-bound accumulation of the next.
// once groups are queued on the lanes, an error return must not leave them running on buffers the caller's next call reuses
static void join_lanes(h2hip_ctx *ctx, int nl) {
    for (int l = 0; l < nl; ++l)
        if (ctx->lane[l]) hipStreamSynchronize(ctx->lane[l]->stream);
}
#define H2_LANES(expr)                                                                           \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            h2::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
            join_lanes(ctx, NL);                                                                 \
            return H2HIP_ERR_HIP;                                                                \
        }                                                                                        \
    } while (0)
#define H2_LANES_RC(expr)         \
    do {                          \
        int r__ = (expr);         \
        if (r__ != H2HIP_OK) {    \
            join_lanes(ctx, NL);  \
            return r__;           \
        }                         \
    } while (0)
// One msm_batch call: the plan, what its stages reserve, and the stages in the order msm_batch runs them
struct BatchMsm {
    h2hip_ctx *ctx;
    const BatchMsmPlan &plan;
    const int NL;
    const h2hip_bases *bases;   // the first column's
    const h2hip_bases *const *bases_per_col;
    const void *const *scalars_in;
    const bool scalars_on_host;
    const BatchMsmHooks &hk;
    bool mid_pending;           // late columns (BatchMsmHooks::mid): the hook runs once, before the first group that holds a column >= mid_after
    char *results = nullptr;
    XYZZ29 *all_buckets = nullptr;   // deferred reduction: every column's buckets
    bool buckets_zeroed = false;
    std::vector<const void *> staged;
    const void *const *scalars_dev = nullptr;

    // (a third context exists even where only two lanes carry columns: BatchMsmPlan::lane_ctxs)
    int ensure_lanes() {
        for (int l = 0; l < plan.lane_ctxs; ++l) {
            if (!ctx->lane[l]) {
                h2hip_ctx *c = nullptr;
                H2_CHK(h2hip_init(ctx->device, nullptr, &c));
                c->msm_window_bits = ctx->msm_window_bits;
                c->is_lane = true;
                ctx->lane[l] = c;
                H2_HIPCHK(hipEventCreate(&ctx->lane_ev[l]));
            }
            inherit_knobs(ctx->lane[l], ctx);
        }
        return H2HIP_OK;
    }
    int fork() {
        if (!ctx->fork_ev) H2_HIPCHK(hipEventCreate(&ctx->fork_ev));
        H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_BATCH, plan.point_bytes * plan.count, (void **)&results));
        H2_HIPCHK(hipEventRecord(ctx->fork_ev, ctx->stream));   // inputs produced on the caller's stream are ready after this
        for (int l = 0; l < NL; ++l) H2_HIPCHK(hipStreamWaitEvent(ctx->lane[l]->stream, ctx->fork_ev, 0));
        return H2HIP_OK;
    }
    int shared_buckets() {
        if (!plan.deferred) return H2HIP_OK;
        H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_BATCH_BUCKETS, plan.buckets_bytes, (void **)&all_buckets));
        // the shared bucket array was zero-filled behind the previous batch's reduction (side stream): the lanes wait for that instead of filling
        // (a fill of the SAME buffer may still be pending on lane 0's stream even when it covered fewer bytes than this batch needs: the lanes wait
        // for it either way, or it could wipe partial sums of lanes 1 / 2 that zero their own regions and start accumulating — ADVICE r04)
        const bool fill_pending = ctx->clean_ev1 && ctx->clean_ptr[1] == all_buckets;
        buckets_zeroed = buckets_prezeroed(ctx, 1, all_buckets, plan.buckets_bytes);
        if (buckets_zeroed || fill_pending)
            for (int l = 0; l < NL; ++l) H2_HIPCHK(hipStreamWaitEvent(ctx->lane[l]->stream, ctx->clean_ev1, 0));
        return H2HIP_OK;
    }
    // host columns: one staging area for all of them; column j is copied on its lane's stream right before its kernels are
    // queued, so the (host-blocking, pageable) copy of column j+1 overlaps the GPU work of column j
    int stage() {
        staged.assign(plan.count, nullptr);
        scalars_dev = scalars_in;
        if (scalars_on_host && plan.n) {
            char *area = nullptr;
            H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_STAGE, sizeof(Fr) * plan.n * plan.count, (void **)&area));
            for (size_t j = 0; j < plan.count; ++j) staged[j] = area + sizeof(Fr) * plan.n * j;
            scalars_dev = staged.data();
        }
        return H2HIP_OK;
    }
    int run_mid() {
        mid_pending = false;
        H2_CHK(hk.mid());
        if (!ctx->fork_ev2) H2_HIPCHK(hipEventCreateWithFlags(&ctx->fork_ev2, hipEventDisableTiming));
        H2_HIPCHK(hipEventRecord(ctx->fork_ev2, ctx->stream));   // what the hook queued on the caller's stream produces the remaining columns
        for (int l = 0; l < NL; ++l) H2_HIPCHK(hipStreamWaitEvent(ctx->lane[l]->stream, ctx->fork_ev2, 0));
        return H2HIP_OK;
    }
    // (two other schedules were built, measured slower and removed in r04: every accumulation on one stream with all sorts / merges on a
    // second, higher-priority one — 2^19 1.00 vs 0.95 ms per MSM, tools/batch_ab.py in r02 — and a column's windows dealt to two lanes —
    // the k = 19 proof 15.7-15.8 vs 14.7 ms, profiles/archive/r03_msm_split_windows_ab.log)
    // (r05, last: the lanes' streams created with the lowest / the highest HIP priority — either way 7 - 10 % slower at k = 17 / 19, profiles/r05_lane_priority_ab.log; removed)
    // (r05 built and measured a third schedule — the sorts of a round of columns queued on ALL lanes before any of their accumulations, so that no
    // sort starts beside an accumulation that holds every CU: the k = 19 proof 13.8-14.0 vs 13.7-13.9 ms, k = 21 53.4-54.0 vs 52.8-53.2, k = 15 / 18
    // equal — profiles/r05_msm_sort_first_ab.log; removed)
    int queue_group(size_t g) {
        const BatchMsmPlan::Group &grp = plan.groups[g];
        const size_t j0 = grp.first, gsize = grp.size;
        h2hip_ctx *c = ctx->lane[g % NL];
        if (hk.col)   // the group's columns are produced now, on the caller's stream (before the mid hook: what it queues may read them)
            for (size_t j = j0; j < j0 + gsize; ++j) H2_LANES_RC(hk.col(j));
        if (mid_pending && j0 + gsize > hk.mid_after) H2_LANES_RC(run_mid());
        if (hk.col) {   // the lane waits for them
            if (!ctx->fork_ev3) H2_LANES(hipEventCreateWithFlags(&ctx->fork_ev3, hipEventDisableTiming));
            H2_LANES(hipEventRecord(ctx->fork_ev3, ctx->stream));
            H2_LANES(hipStreamWaitEvent(c->stream, ctx->fork_ev3, 0));
        }
        hipEvent_t sorted_ev = nullptr;   // what this group's MSM records behind its scatter
        if (grp.sort_waits && ctx->lane[g - 1]->sorted_ev) H2_LANES(hipStreamWaitEvent(c->stream, ctx->lane[g - 1]->sorted_ev, 0));
        if (grp.sort_signals) {
            if (!c->sorted_ev) H2_LANES(hipEventCreateWithFlags(&c->sorted_ev, hipEventDisableTiming));
            sorted_ev = c->sorted_ev;
        }
        for (size_t j = j0; j < j0 + gsize; ++j) {
            if (scalars_on_host && plan.n) H2_LANES(hipMemcpyAsync((void *)staged[j], scalars_in[j], sizeof(Fr) * plan.n, hipMemcpyHostToDevice, c->stream));
        }
        char *outbuf = nullptr;
        H2_LANES_RC(ws_reserve(c, h2hip_ctx::WS_OUT, sizeof(XYZZ) * MSM_MAX_COLS, (void **)&outbuf));
        H2_LANES_RC(msm_run_cols(c, bases_per_col ? bases_per_col[j0] : bases, (const Fr *const *)(scalars_dev + j0), (uint32_t)gsize, plan.n, (XYZZ *)outbuf,
                                 plan.deferred ? all_buckets + plan.keys_per_col * j0 : nullptr, buckets_zeroed, sorted_ev));
        if (!plan.deferred) finish_slots(c, (const XYZZ *)outbuf, results, gsize, j0, plan.affine);   // the group's results, one lane each, into their slots of the batch's result array
        H2_LANES(hipGetLastError());
        return H2HIP_OK;
    }
    int join() {
        for (int l = 0; l < NL; ++l) {
            H2_HIPCHK(hipEventRecord(ctx->lane_ev[l], ctx->lane[l]->stream));
            H2_HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->lane_ev[l], 0));
        }
        return H2HIP_OK;
    }
    // The accumulations are queued and joined: what follows on this stream is the reduction's tail.  The hook runs HERE, before the tail is
    // queued: the device is still hundreds of microseconds of accumulation behind the host at this point, so the hook's few launches do not
    // delay the reduction — and a wait on the event must be issued before more work follows it on this stream (r04 timeline,
    // profiles/archive/r04_timeline_k19.md: issued after the tail and the result copy had been queued, the side transforms started 20 us after that
    // copy FINISHED — the runtime resolved the cross-stream wait against what the stream held at the time of the wait, not of the record)
    int tail_hook(int *hook_rc) {
        if (!hk.tail) return H2HIP_OK;
        if (!ctx->tail_ev) H2_HIPCHK(hipEventCreateWithFlags(&ctx->tail_ev, hipEventDisableTiming));
        H2_HIPCHK(hipEventRecord(ctx->tail_ev, ctx->stream));
        *hook_rc = hk.tail(ctx->tail_ev);
        return H2HIP_OK;
    }
    // one bucket reduction per 64 columns, on the caller's stream
    int reduce_deferred() {
        XYZZ *sums = nullptr;
        H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_OUT, sizeof(XYZZ) * plan.count, (void **)&sums));
        for (size_t c0 = 0; c0 < plan.count; c0 += 64) {
            const uint32_t cc = (uint32_t)(plan.count - c0 < 64 ? plan.count - c0 : 64);
            H2_CHK(msm_reduce_cols(ctx, bases, bases->window_bits, all_buckets + plan.keys_per_col * c0, cc, sums + c0));
        }
        finish_slots(ctx, sums, results, plan.count, 0, plan.affine);
        H2_HIPCHK(hipGetLastError());
        return H2HIP_OK;
    }
};

// bases_per_col (optional): a base set per column — columns over different sets (e.g. a Lagrange-basis and a monomial-basis commitment of
// the same prover round) share the lanes and, when their window tables match, the deferred bucket reduction.  hooks (optional): BatchMsmHooks, internal.h
int msm_batch(h2hip_ctx *ctx, const h2hip_bases *bases, const h2hip_bases *const *bases_per_col, const void *const *scalars_in, bool scalars_on_host,
              size_t n, size_t count, int point_format, void *out_host, const BatchMsmHooks *hooks) {
    if (bases_per_col && count) bases = bases_per_col[0];
    H2_REQUIRE(ctx && bases && (count == 0 || (scalars_in && out_host)), "NULL argument");
    BatchMsmPlan plan;
    H2_CHK(msm_batch_plan(*ctx, bases, bases_per_col, n, count, point_format, &plan));
    if (!count) return H2HIP_OK;
    for (size_t j = 0; j < count; ++j) H2_REQUIRE(n == 0 || scalars_in[j], "NULL scalar column");   // everything checked before the first launch
    const BatchMsmHooks none;
    const BatchMsmHooks &hk = hooks ? *hooks : none;
    BatchMsm run{ctx, plan, plan.NL, bases, bases_per_col, scalars_in, scalars_on_host, hk, (bool)hk.mid};
    H2_CHK(run.ensure_lanes());
    H2_CHK(run.fork());
    H2_CHK(run.shared_buckets());
    H2_CHK(run.stage());
    for (size_t g = 0; g < plan.groups.size(); ++g) H2_CHK(run.queue_group(g));   // (a failing group has joined the lanes)
    const int NL = plan.NL;
    if (run.mid_pending) H2_LANES_RC(run.run_mid());   // (no column behind mid_after: the hook still runs, before the join)
    H2_CHK(run.join());
    int hook_rc = H2HIP_OK;
    H2_CHK(run.tail_hook(&hook_rc));
    if (plan.deferred) {
        H2_CHK(run.reduce_deferred());
        // zero-fill of the shared bucket array for the next batch, off its critical path — queued AFTER the hook's work and on the first lane's stream
        // (the hook works on the last lane's): a fill that waits for the reduction must not sit in front of that work in a shared hardware queue
        H2_CHK(buckets_clean_after_use(ctx, 1, run.all_buckets, plan.buckets_bytes, ctx->clean_on_lane ? ctx->lane[0]->stream : nullptr));
    }
    H2_CHK(sync_results(ctx, out_host, run.results, plan.point_bytes * count));   // the commitments come back (r05: through the host-mapped flag, no runtime wait)
    return hook_rc;   // (the lanes' kernel timers are folded into this context's table when it is read: prof_collect_all)
}

}  // namespace h2

using namespace h2;

extern "C" {

static int bases_create(h2hip_ctx *ctx, const void *src, bool src_on_device, size_t n, uint32_t flags, h2hip_bases **out) {
    H2_REQUIRE(ctx && out && (n == 0 || src), "NULL argument");
    H2_REQUIRE((flags & ~H2HIP_BASES_PRECOMPUTE) == 0, "unknown flags");
    h2hip_bases *b = new h2hip_bases();
    b->n = n;
    hipError_t e = hipMalloc((void **)&b->pts, sizeof(G1Affine) * (n ? n : 1));
    if (e != hipSuccess) {
        set_error("hipMalloc for %zu bases failed: %s", n, hipGetErrorString(e));
        delete b;
        return H2HIP_ERR_NOMEM;
    }
    if (n) {
        e = hipMemcpyAsync(b->pts, src, sizeof(G1Affine) * n, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            set_error("copying bases failed: %s", hipGetErrorString(e));
            hipFree(b->pts);
            delete b;
            return H2HIP_ERR_HIP;
        }
    }
    {
        int rc = msm_prepare_bases(ctx, b, (flags & H2HIP_BASES_PRECOMPUTE) != 0);
        if (rc != H2HIP_OK) {
            hipFree(b->pts);
            delete b;
            return rc;
        }
    }
    *out = b;
    return H2HIP_OK;
}
int h2hip_bases_upload(h2hip_ctx *ctx, const void *g1_affine_host, size_t n, uint32_t flags, h2hip_bases **out) {
    H2_DEVICE_GUARD(ctx);
    return bases_create(ctx, g1_affine_host, false, n, flags, out);
}
int h2hip_bases_from_device(h2hip_ctx *ctx, const void *g1_affine_dev, size_t n, uint32_t flags, h2hip_bases **out) {
    H2_DEVICE_GUARD(ctx);
    return bases_create(ctx, g1_affine_dev, true, n, flags, out);
}
void h2hip_bases_free(h2hip_ctx *ctx, h2hip_bases *bases) {
    H2_DEVICE_GUARD(ctx);
    if (!bases) return;
    if (ctx) hipStreamSynchronize(ctx->stream);
    if (bases->pts) hipFree(bases->pts);
    if (bases->pts29) hipFree(bases->pts29);
    delete bases;
}
size_t h2hip_bases_len(const h2hip_bases *bases) { return bases ? bases->n : 0; }

int h2hip_msm_g1_dev(h2hip_ctx *ctx, const h2hip_bases *bases, const void *scalars_dev, size_t n, int point_format, void *out_host) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && bases && out_host && (n == 0 || scalars_dev), "NULL argument");
    H2_REQUIRE(point_format == H2HIP_POINT_JACOBIAN || point_format == H2HIP_POINT_AFFINE, "unknown point_format");
    char *outbuf = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_OUT, 1024, (void **)&outbuf));
    H2_CHK(msm_run(ctx, bases, (const Fr *)scalars_dev, n, (XYZZ *)outbuf));
    return finish_point(ctx, outbuf, point_format, out_host);
}
int h2hip_msm_g1_batch_dev(h2hip_ctx *ctx, const h2hip_bases *bases, const void *const *scalars_dev, size_t n, size_t count, int point_format,
                           void *out_host) {
    H2_DEVICE_GUARD(ctx);
    return msm_batch(ctx, bases, nullptr, scalars_dev, false, n, count, point_format, out_host, nullptr);
}
int h2hip_msm_g1_multi_dev(h2hip_ctx *ctx, const h2hip_bases *const *bases_per_column, const void *const *scalars_dev, size_t n, size_t count,
                           int point_format, void *out_host) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (count == 0 || bases_per_column), "NULL argument");
    if (!count) return H2HIP_OK;
    return msm_batch(ctx, nullptr, bases_per_column, scalars_dev, false, n, count, point_format, out_host, nullptr);
}
int h2hip_msm_g1_batch(h2hip_ctx *ctx, const h2hip_bases *bases, const void *const *scalars_host, size_t n, size_t count, int point_format,
                       void *out_host) {
    H2_DEVICE_GUARD(ctx);
    return msm_batch(ctx, bases, nullptr, scalars_host, true, n, count, point_format, out_host, nullptr);
}

int h2hip_msm_g1(h2hip_ctx *ctx, const h2hip_bases *bases, const void *scalars_host, size_t n, int point_format, void *out_host) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && bases && out_host && (n == 0 || scalars_host), "NULL argument");
    Fr *stage = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_STAGE, sizeof(Fr) * n, (void **)&stage));
    if (n) H2_HIPCHK(hipMemcpyAsync(stage, scalars_host, sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->stream));
    return h2hip_msm_g1_dev(ctx, bases, stage, n, point_format, out_host);
}

int h2hip_g1_sum_jacobian_dev(h2hip_ctx *ctx, const void *points_dev, size_t n, int point_format, void *out_host) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && out_host && (n == 0 || points_dev), "NULL argument");
    H2_REQUIRE(point_format == H2HIP_POINT_JACOBIAN || point_format == H2HIP_POINT_AFFINE, "unknown point_format");
    H2_REQUIRE(n < (1u << 24), "too many points");
    char *outbuf = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_OUT, 1024, (void **)&outbuf));
    prof_begin(ctx, "jac_sum_kernel");
    hipLaunchKernelGGL(jac_sum_kernel, dim3(1), dim3(64), 0, ctx->stream, (const G1Jac *)points_dev, (uint32_t)n, (XYZZ *)outbuf);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return finish_point(ctx, outbuf, point_format, out_host);
}

// The host half of a point-range sharded commitment round: out[j] = sum over ranks r of gathered[r * count + j] (Jacobian partials as
// h2hip_comm_allgather_host leaves them, rank-major), for all `count` columns in one call — a few dozen point additions on the host,
// no device round trip.  point_format of the OUTPUT: Jacobian (z = 1 or 0) or affine.
int h2hip_g1_sum_partials_host(const void *gathered_jacobian, size_t world, size_t count, int point_format, void *out) {
    H2_REQUIRE((count == 0 || (gathered_jacobian && out)) && world >= 1, "bad argument");
    H2_REQUIRE(point_format == H2HIP_POINT_JACOBIAN || point_format == H2HIP_POINT_AFFINE, "unknown point_format");
    const G1Jac *in = (const G1Jac *)gathered_jacobian;
    for (size_t j = 0; j < count; ++j) {
        XYZZ acc = XYZZ::identity();
        for (size_t r = 0; r < world; ++r) {
            G1Jac p;
            memcpy(&p, &in[r * count + j], sizeof(G1Jac));
            if (p.z.is_zero()) continue;
            XYZZ q;
            q.x = p.x;
            q.y = p.y;
            q.zz = fe_sqr(p.z);
            q.zzz = fe_mul(q.zz, p.z);
            xyzz_add(acc, q);
        }
        const G1Affine a = xyzz_to_affine(acc);
        if (point_format == H2HIP_POINT_AFFINE) {
            memcpy((char *)out + sizeof(G1Affine) * j, &a, sizeof(G1Affine));
        } else {
            G1Jac o;
            o.x = a.x;
            o.y = a.y;
            o.z = a.is_identity() ? Fq::zero() : Fq::one();
            memcpy((char *)out + sizeof(G1Jac) * j, &o, sizeof(G1Jac));
        }
    }
    return H2HIP_OK;
}

}  // extern "C"
