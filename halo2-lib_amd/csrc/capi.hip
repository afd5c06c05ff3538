// C ABI of libh2hip (declared in include/h2hip.h), the part every other file stands on: errors, workspace, host polling, the kernel
// profiler, the context's life cycle, tuning knobs, memory and timers.  (The MSM entries: msm_batch.hip; the NTT entries: ntt.hip.)
#include <stdarg.h>

#include <algorithm>

#include "internal.h"
#include <sched.h>

namespace h2 {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int ws_reserve(h2hip_ctx *ctx, int slot, size_t bytes, void **out) {
    DevBuf &b = ctx->ws[slot];
    if (bytes == 0) bytes = 256;
    if (b.cap < bytes) {
        if (b.p) {
            H2_HIPCHK(hipStreamSynchronize(ctx->stream));
            if (ctx->clean_stream) H2_HIPCHK(hipStreamSynchronize(ctx->clean_stream));   // a pending zero-fill of this buffer ...
            if (ctx->lane[0]) H2_HIPCHK(hipStreamSynchronize(ctx->lane[0]->stream));      // ... (the batch's runs on its first lane's stream)
            H2_HIPCHK(hipFree(b.p));
            b.p = nullptr;
            b.cap = 0;
        }
        size_t cap = (bytes + 0xFFFFF) & ~(size_t)0xFFFFF;   // 1 MiB granules
        hipError_t e = hipMalloc(&b.p, cap);
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu) for workspace slot %d failed: %s", cap, slot, hipGetErrorString(e));
            b.p = nullptr;
            return H2HIP_ERR_NOMEM;
        }
        b.cap = cap;
    }
    *out = b.p;
    return H2HIP_OK;
}

// ---------------------------------------------------------------------------------------------- host round trips through a host-mapped flag (r05)
constexpr size_t POLL_BYTES = 16384;
__global__ __launch_bounds__(256) void publish_kernel(const uint32_t *__restrict__ src, uint32_t *dst_host, uint32_t nwords, unsigned long long *flag_host,
                                                      unsigned long long seq) {
    for (uint32_t i = threadIdx.x; i < nwords; i += 256) dst_host[i] = src[i];
#ifdef H2_HIPEMU
    __syncthreads();
    if (threadIdx.x == 0) *flag_host = seq;
#else
    __threadfence_system();   // every lane's payload stores are visible to the host before ...
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag_host, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // ... the flag is
#endif
}
static int poll_init(h2hip_ctx *ctx) {
    if (ctx->poll_host) return H2HIP_OK;
    void *h = nullptr;
    H2_HIPCHK(hipHostMalloc(&h, 64 + POLL_BYTES, hipHostMallocMapped | hipHostMallocCoherent));   // fine-grained: the flag store is visible while the stream goes on
    memset(h, 0, 64 + POLL_BYTES);
    ctx->poll_host = (char *)h;
#ifdef H2_HIPEMU
    ctx->poll_dev = ctx->poll_host;
#else
    void *d = nullptr;
    H2_HIPCHK(hipHostGetDevicePointer(&d, h, 0));
    ctx->poll_dev = (char *)d;
#endif
    return H2HIP_OK;
}
int sync_results(h2hip_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    if (!ctx->host_poll || bytes > POLL_BYTES || (bytes & 3) || ((uintptr_t)src_dev & 3)) {
        if (bytes) H2_HIPCHK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        H2_HIPCHK(hipStreamSynchronize(ctx->stream));
        return H2HIP_OK;
    }
    H2_CHK(poll_init(ctx));
    const unsigned long long seq = ++ctx->poll_seq;
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(256), 0, ctx->stream, (const uint32_t *)src_dev, (uint32_t *)(ctx->poll_dev + 64), (uint32_t)(bytes / 4),
                       (unsigned long long *)ctx->poll_dev, seq);
    H2_HIPCHK(hipGetLastError());
    const volatile unsigned long long *flag = (const volatile unsigned long long *)ctx->poll_host;
    for (uint64_t spins = 1; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq; ++spins) {
        if ((spins & 0x3FFFF) == 0) {   // every ~10 ms: a faulted stream would never raise the flag
            const hipError_t e = hipStreamQuery(ctx->stream);
            if (e == hipSuccess) break;   // (the stream has drained: the kernel's stores are complete)
            if (e != hipErrorNotReady) H2_HIPCHK(e);
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        if (spins > 20000 && (spins & 0x3F) == 0) sched_yield();   // a wait of more than ~1 ms: leave the core to the other contexts' host threads
    }
    if (bytes) memcpy(dst_host, ctx->poll_host + 64, bytes);
    return H2HIP_OK;
}
int sync_stream(h2hip_ctx *ctx) { return sync_results(ctx, nullptr, ctx->poll_dev ? ctx->poll_dev + 64 : nullptr, 0); }

static hipEvent_t get_event(h2hip_ctx *ctx) {
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void prof_begin(h2hip_ctx *ctx, const char *name) {
    if (!ctx->profiling) return;
    if (!ctx->prof_filter.empty() && strncmp(name, ctx->prof_filter.c_str(), ctx->prof_filter.size()) != 0) return;
    hipEvent_t a = get_event(ctx), b = get_event(ctx);
    if (!a || !b) return;
    hipEventRecord(a, ctx->stream);
    ctx->pending.push_back({name, a, b, false});
}
// a bracket whose two events the LAUNCH itself records (hipExtLaunchKernelGGL's start / stop events: no marker packets of their own in the
// stream — the bench's timed region brackets every accumulation launch, and separate event records cost the proof ~0.3 ms).  false: not profiled
bool prof_launch_events(h2hip_ctx *ctx, const char *name, hipEvent_t *start, hipEvent_t *stop) {
    *start = *stop = nullptr;
    if (!ctx->profiling) return false;
    if (!ctx->prof_filter.empty() && strncmp(name, ctx->prof_filter.c_str(), ctx->prof_filter.size()) != 0) return false;
    hipEvent_t a = get_event(ctx), b = get_event(ctx);
    if (!a || !b) return false;
    ctx->pending.push_back({name, a, b, true});
    *start = a;
    *stop = b;
    return true;
}
// closes the innermost open bracket (brackets nest: the lookup permutation's bracket contains the scan's)
void prof_end(h2hip_ctx *ctx) {
    if (!ctx->profiling || !ctx->prof_filter.empty()) {
        // with a filter the brackets kept are leaf brackets of one name: close the open one of that name, if any
        if (ctx->profiling && !ctx->pending.empty() && !ctx->pending.back().ended) {
            hipEventRecord(ctx->pending.back().end, ctx->stream);
            ctx->pending.back().ended = true;
        }
        return;
    }
    for (size_t i = ctx->pending.size(); i-- > 0;)
        if (!ctx->pending[i].ended) {
            hipEventRecord(ctx->pending[i].end, ctx->stream);
            ctx->pending[i].ended = true;
            return;
        }
}
static void prof_collect(h2hip_ctx *ctx) {
    if (ctx->pending.empty()) return;
    hipStreamSynchronize(ctx->stream);
    for (auto &p : ctx->pending) {
        float ms = 0;
        if (p.ended && hipEventElapsedTime(&ms, p.begin, p.end) == hipSuccess) {
            KernelStat &s = ctx->stats[p.name];
            s.total_ms += ms;
            s.launches += 1;
            float t0 = 0;
            if (ctx->prof_ref && hipEventElapsedTime(&t0, ctx->prof_ref, p.begin) == hipSuccess) s.spans.push_back({t0, t0 + ms});
        }
        ctx->event_pool.push_back(p.begin);
        ctx->event_pool.push_back(p.end);
    }
    (void)hipGetLastError();   // a failed elapsed-time query must not surface as the next launch's error
    ctx->pending.clear();
}

static void prof_collect_all(h2hip_ctx *ctx);
// a child context's (MSM lane, the prover's side stream) kernel timers into the parent's table
void prof_fold_child(h2hip_ctx *parent, h2hip_ctx *child) {
    prof_collect(child);
    for (auto &kv : child->stats) {
        parent->stats[kv.first].total_ms += kv.second.total_ms;
        parent->stats[kv.first].launches += kv.second.launches;
        parent->stats[kv.first].spans.insert(parent->stats[kv.first].spans.end(), kv.second.spans.begin(), kv.second.spans.end());
    }
    child->stats.clear();
}
// this context's timers and its lanes': the lanes' are folded when the table is READ, not after every batch (the elapsed-time queries of a
// proof's bracketed launches are host time inside the bench's timed region otherwise)
static void prof_collect_all(h2hip_ctx *ctx) {
    prof_collect(ctx);
    for (h2hip_ctx *l : ctx->lane)
        if (l) prof_fold_child(ctx, l);
}

}  // namespace h2

using namespace h2;

extern "C" {

const char *h2hip_last_error(void) { return g_err; }
int h2hip_version(void) { return 100; }

int h2hip_device_count(int *count) {
    H2_REQUIRE(count, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return H2HIP_ERR_NO_DEVICE;
    }
    *count = n;
    return H2HIP_OK;
}

int h2hip_init(int device, void *hip_stream, h2hip_ctx **out) {
    H2_REQUIRE(out, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available (libh2hip has no CPU fallback)");
        return H2HIP_ERR_NO_DEVICE;
    }
    H2_REQUIRE(device >= 0 && device < n, "device index out of range");
    H2_HIPCHK(hipSetDevice(device));
    h2hip_ctx *ctx = new h2hip_ctx();
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
        ctx->own_stream = false;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
            delete ctx;
            return H2HIP_ERR_HIP;
        }
        ctx->own_stream = true;
    }
    *out = ctx;
    return H2HIP_OK;
}

}  // extern "C"
namespace h2 {
// Small host tables (job descriptors) -> device without a synchronisation: the bytes are copied into a pinned ring first, so the caller's
// buffer may go away at once and the asynchronous copy has a stable source.  The ring only wraps after a stream synchronisation.
constexpr size_t JOB_RING_BYTES = (size_t)1 << 20;
int upload_jobs(h2hip_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes) {
    if (!bytes) return H2HIP_OK;
    if (bytes > JOB_RING_BYTES / 4) {   // large tables: plain (staged, host-synchronous) copy
        H2_HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
        H2_HIPCHK(hipStreamSynchronize(ctx->stream));
        return H2HIP_OK;
    }
    if (!ctx->job_ring) H2_HIPCHK(hipHostMalloc((void **)&ctx->job_ring, JOB_RING_BYTES, 0));
    const size_t need = (bytes + 255) / 256 * 256;
    if (ctx->job_ring_off + need > JOB_RING_BYTES) {
        H2_HIPCHK(hipStreamSynchronize(ctx->stream));   // everything staged so far has been consumed
        ctx->job_ring_off = 0;
    }
    char *slot = ctx->job_ring + ctx->job_ring_off;
    memcpy(slot, src_host, bytes);
    ctx->job_ring_off += need;
    H2_HIPCHK(hipMemcpyAsync(dst_dev, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
    return H2HIP_OK;
}
}  // namespace h2
extern "C" {

void h2hip_destroy(h2hip_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (int l = 0; l < 4; ++l)
        if (ctx->lane[l]) hipStreamSynchronize(ctx->lane[l]->stream);   // (a zero-fill of this context's bucket array may be queued on a lane's stream)
    if (ctx->clean_stream) {
        hipStreamSynchronize(ctx->clean_stream);
        hipStreamDestroy(ctx->clean_stream);
        hipEventDestroy(ctx->clean_ev);
        hipEventDestroy(ctx->clean_ev1);
        hipEventDestroy(ctx->used_ev);
    }
    if (ctx->tail_ev) hipEventDestroy(ctx->tail_ev);
    if (ctx->sorted_ev) hipEventDestroy(ctx->sorted_ev);
    if (ctx->job_ring) hipHostFree(ctx->job_ring);
    if (ctx->poll_host) hipHostFree(ctx->poll_host);
    for (auto &b : ctx->ws)
        if (b.p) hipFree(b.p);
    for (auto &t : ctx->twiddles) {
        hipFree(t.t1);
        hipFree(t.t2);
        for (int k = 0; k < 4; ++k) {
            if (t.direct[k]) hipFree(t.direct[k]);
        }
    }
    for (auto &p : ctx->pending) {
        hipEventDestroy(p.begin);
        hipEventDestroy(p.end);
    }
    for (auto e : ctx->event_pool) hipEventDestroy(e);
    if (ctx->prof_ref && ctx->own_prof_ref) hipEventDestroy(ctx->prof_ref);
    for (int l = 0; l < 4; ++l)
        if (ctx->lane[l]) {
            h2hip_destroy(ctx->lane[l]);
            hipEventDestroy(ctx->lane_ev[l]);
        }
    if (ctx->fork_ev) hipEventDestroy(ctx->fork_ev);
    if (ctx->fork_ev2) hipEventDestroy(ctx->fork_ev2);
    if (ctx->fork_ev3) hipEventDestroy(ctx->fork_ev3);
    for (auto e : ctx->timer_ev)
        if (e) hipEventDestroy(e);
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int h2hip_sync(h2hip_ctx *ctx) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "ctx is NULL");
    H2_HIPCHK(hipStreamSynchronize(ctx->stream));
    return H2HIP_OK;
}

// (the knobs, their legal values and their inheritance: H2_KNOB_TABLE in internal.h)
static int *param_slot(h2hip_ctx *ctx, const char *name) {
#define H2_KNOB_SLOT(knob, inherit, legal, domain) \
    if (!strcmp(name, #knob)) return &ctx->knob;
    H2_KNOB_TABLE(H2_KNOB_SLOT)
#undef H2_KNOB_SLOT
    return nullptr;
}
int h2hip_set_param(h2hip_ctx *ctx, const char *name, int value) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && name, "NULL argument");
    int *p = param_slot(ctx, name);
    H2_REQUIRE(p, "unknown parameter name");
    // a value outside the knob's domain is refused and the stored value stays
#define H2_KNOB_CHECK(knob, inherit, legal, domain)                                                     \
    if (p == &ctx->knob) {                                                                              \
        const int v = value;                                                                            \
        if (!(legal)) {                                                                                 \
            set_error("h2hip_set_param: invalid argument: " #knob " = %d: must be " domain, value);   \
            return H2HIP_ERR_INVALID;                                                                   \
        }                                                                                               \
    }
    H2_KNOB_TABLE(H2_KNOB_CHECK)
#undef H2_KNOB_CHECK
    *p = value;
    return H2HIP_OK;
}
int h2hip_get_param(h2hip_ctx *ctx, const char *name, int *value) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && name && value, "NULL argument");
    int *p = param_slot(ctx, name);
    H2_REQUIRE(p, "unknown parameter name");
    *value = *p;
    return H2HIP_OK;
}

int h2hip_malloc(h2hip_ctx *ctx, size_t bytes, void **dptr) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && dptr, "NULL argument");
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 256);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return H2HIP_ERR_NOMEM;
    }
    return H2HIP_OK;
}
int h2hip_free(h2hip_ctx *ctx, void *dptr) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "ctx is NULL");
    if (!dptr) return H2HIP_OK;
    H2_HIPCHK(hipStreamSynchronize(ctx->stream));
    H2_HIPCHK(hipFree(dptr));
    return H2HIP_OK;
}
// Page-locks a caller-owned host buffer (e.g. the Vec<Fr> columns a prover re-uses across proofs): uploads from it then run on the DMA
// engines asynchronously instead of through the runtime's pageable staging copies.
int h2hip_host_register(h2hip_ctx *ctx, void *host_ptr, size_t bytes) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && host_ptr && bytes, "NULL argument");
    H2_HIPCHK(hipHostRegister(host_ptr, bytes, hipHostRegisterDefault));
    return H2HIP_OK;
}
int h2hip_host_unregister(h2hip_ctx *ctx, void *host_ptr) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && host_ptr, "NULL argument");
    H2_HIPCHK(hipHostUnregister(host_ptr));
    return H2HIP_OK;
}
int h2hip_upload(h2hip_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (bytes == 0 || (dst_dev && src_host)), "NULL argument");
    if (!bytes) return H2HIP_OK;
    H2_HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    H2_HIPCHK(hipStreamSynchronize(ctx->stream));
    return H2HIP_OK;
}
int h2hip_download(h2hip_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (bytes == 0 || (dst_host && src_dev)), "NULL argument");
    if (!bytes) return H2HIP_OK;
    H2_HIPCHK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    H2_HIPCHK(hipStreamSynchronize(ctx->stream));
    return H2HIP_OK;
}

// ------------------------------------------------------------------ profiling
int h2hip_profile_enable(h2hip_ctx *ctx, int on) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "ctx is NULL");
    prof_collect_all(ctx);
    ctx->profiling = on != 0;
    return H2HIP_OK;
}
int h2hip_profile_filter(h2hip_ctx *ctx, const char *prefix) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "ctx is NULL");
    prof_collect_all(ctx);
    ctx->prof_filter = prefix ? prefix : "";
    return H2HIP_OK;
}
int h2hip_profile_reset(h2hip_ctx *ctx) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "ctx is NULL");
    prof_collect_all(ctx);
    ctx->stats.clear();
    if (!ctx->prof_ref) {
        H2_HIPCHK(hipEventCreate(&ctx->prof_ref));
        ctx->own_prof_ref = true;
    }
    if (ctx->own_prof_ref) {
        H2_HIPCHK(hipEventRecord(ctx->prof_ref, ctx->stream));
        H2_HIPCHK(hipEventSynchronize(ctx->prof_ref));
    }
    return H2HIP_OK;
}
// time during which at least one launch of the matching kernels was executing (union of the launch spans): with
// pipelined MSMs several launches of one kernel overlap, and busy / launches is what one launch effectively costs
int h2hip_profile_get_busy(h2hip_ctx *ctx, const char *prefix, double *busy_ms) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && prefix && busy_ms, "NULL argument");
    prof_collect_all(ctx);
    std::vector<std::pair<float, float>> all;
    size_t len = strlen(prefix);
    for (auto &kv : ctx->stats)
        if (kv.first.compare(0, len, prefix) == 0) all.insert(all.end(), kv.second.spans.begin(), kv.second.spans.end());
    std::sort(all.begin(), all.end());
    double busy = 0;
    float cur0 = 0, cur1 = -1;
    for (auto &sp : all) {
        if (cur1 < cur0 || sp.first > cur1) {
            if (cur1 >= cur0) busy += cur1 - cur0;
            cur0 = sp.first;
            cur1 = sp.second;
        } else if (sp.second > cur1) {
            cur1 = sp.second;
        }
    }
    if (cur1 >= cur0) busy += cur1 - cur0;
    *busy_ms = busy;
    return H2HIP_OK;
}
int h2hip_profile_get(h2hip_ctx *ctx, const char *prefix, double *total_ms, uint64_t *launches) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && prefix, "NULL argument");
    prof_collect_all(ctx);
    double ms = 0;
    uint64_t cnt = 0;
    size_t len = strlen(prefix);
    for (auto &kv : ctx->stats)
        if (kv.first.compare(0, len, prefix) == 0) {
            ms += kv.second.total_ms;
            cnt += kv.second.launches;
        }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = cnt;
    return H2HIP_OK;
}
// every kernel name with launches since the last reset, as "name total_ms launches busy_ms\n" lines (NUL-terminated; truncated at cap)
int h2hip_profile_dump(h2hip_ctx *ctx, char *out, size_t cap, size_t *needed) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && (out || cap == 0), "NULL argument");
    prof_collect_all(ctx);
    std::string text;
    for (auto &kv : ctx->stats) {
        std::vector<std::pair<float, float>> all(kv.second.spans.begin(), kv.second.spans.end());
        std::sort(all.begin(), all.end());
        double busy = 0;
        float cur0 = 0, cur1 = -1;
        for (auto &sp : all) {
            if (cur1 < cur0 || sp.first > cur1) {
                if (cur1 >= cur0) busy += cur1 - cur0;
                cur0 = sp.first;
                cur1 = sp.second;
            } else if (sp.second > cur1) {
                cur1 = sp.second;
            }
        }
        if (cur1 >= cur0) busy += cur1 - cur0;
        char line[256];
        snprintf(line, sizeof(line), "%s %.6f %llu %.6f\n", kv.first.c_str(), kv.second.total_ms, (unsigned long long)kv.second.launches, busy);
        text += line;
    }
    if (needed) *needed = text.size() + 1;
    if (cap) {
        size_t m = text.size() < cap - 1 ? text.size() : cap - 1;
        memcpy(out, text.data(), m);
        out[m] = 0;
    }
    return H2HIP_OK;
}
int h2hip_timer_start(h2hip_ctx *ctx) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx, "ctx is NULL");
    if (!ctx->timer_ev[0]) {   // per context: an event belongs to the device it was created on
        H2_HIPCHK(hipEventCreate(&ctx->timer_ev[0]));
        H2_HIPCHK(hipEventCreate(&ctx->timer_ev[1]));
    }
    H2_HIPCHK(hipEventRecord(ctx->timer_ev[0], ctx->stream));
    return H2HIP_OK;
}
int h2hip_timer_stop(h2hip_ctx *ctx, double *elapsed_ms) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && elapsed_ms && ctx->timer_ev[0], "timer not started");
    H2_HIPCHK(hipEventRecord(ctx->timer_ev[1], ctx->stream));
    H2_HIPCHK(hipEventSynchronize(ctx->timer_ev[1]));
    float ms = 0;
    H2_HIPCHK(hipEventElapsedTime(&ms, ctx->timer_ev[0], ctx->timer_ev[1]));
    *elapsed_ms = ms;
    return H2HIP_OK;
}

}  // extern "C"
