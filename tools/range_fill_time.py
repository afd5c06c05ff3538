"""Range checks filled on the device against the same cells computed on the host.
Usage: python tools/range_fill_time.py [k] [range_bits] [lookup_bits] [reps] [runs]     (defaults 19 88 18 7 3)

The layout is the headline's shape: one gate column of 2^k rows filled down to the usable rows with range checks of range_bits bits at
lookup_bits (88 at 18: five limbs and a tail gate, 17 gate cells and 6 lookup cells per unit) and one lookup-advice column that takes the
units' lookup cells; the checked values lie in a device buffer of their own (what a kernel before the fill produced).
  (a) device   one h2hip_range_fill_checks_dev call on columns resident on the device, then a wait for the stream;
  (b) host     what was possible before: a download of the values, the same cells by tools/range_host_fill.cpp — one host thread on the
               library's host field, the library's own per-slot code — and h2hip_upload of the gate and the lookup column.
`runs` runs of each, alternating, `reps` repetitions per run: the median of every run, one JSON line at the end.  Then the lone fill (events on
the context's stream), cells per second, and the bytes it writes per second next to the HBM bandwidth a streaming copy reaches; and how
that time splits into the kernel (the library's per-kernel events) and the host side of the call."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_lib_amd as H  # noqa: E402
from halo2_lib_amd import plonk as PL  # noqa: E402
from tests.util import R, fr  # noqa: E402

a = [int(v) for v in sys.argv[1:]]
k, rb, lb, reps, runs = (a + [19, 88, 18, 7, 3][len(a):])[:5]
_vp = C.c_void_p
HBM_COPY_TBS = 6.29   # a float4 copy on this part (8.0 TB/s is the specification)


def host_helper():
    src, lib = os.path.join(ROOT, "tools", "range_host_fill.cpp"), os.path.join(ROOT, "tools", "range_host_fill.so")
    deps = [src, os.path.join(ROOT, "include", "h2hip.h"), os.path.join(ROOT, "halo2-lib_amd", "csrc", "range_fill.cuh"),
            os.path.join(ROOT, "halo2-lib_amd", "csrc", "trace_place.cuh")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-shared", "-fPIC",
                               "-Wno-unused-value", "-o", lib, src])
    h = C.CDLL(lib)
    h.range_host_fill_checks.restype = None
    h.range_host_fill_checks.argtypes = [C.POINTER(_vp), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(_vp), C.c_size_t, _vp, _vp, C.c_uint32, C.c_uint32,
                                         C.c_uint32, _vp, C.c_size_t]
    return h


helper = host_helper()
ctx = H.Context()
n = 1 << k
u = n - 7                                     # the usable rows with six blinding factors
ncells, nlk, _ = PL.range_check_layout(rb, lb)
L, rem = -(-rb // lb), rb % lb
count = (u - 2) // ncells                     # the last cell two rows above the end, as gate.max_rows leaves them
assert count * nlk <= u, "the lookup cells do not fit one column"
table = PL.range_check_table([(0, j * ncells, j, 0, j * nlk) for j in range(count)])   # built once
g = np.random.default_rng(k)
vals = fr([int.from_bytes(g.bytes(16), "little") % (1 << rb) for _ in range(count)])
pows = fr([pow(2, i * lb, R) for i in range(L)] + [1 << (lb - rem if rem else 0), 1, R - 1])
print("k=%d: %d range checks of %d bits at %d: %d gate cells and %d lookup cells" % (k, count, rb, lb, count * ncells, count * nlk), flush=True)

d_vals = ctx.to_device(vals)
d_gate = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))
d_lk = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))
host_gate, host_lk = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
host_cols, host_lks = (_vp * 1)(_vp(host_gate.ctypes.data)), (_vp * 1)(_vp(host_lk.ctypes.data))


def device_fill():
    PL.range_fill_checks(ctx, [d_gate], u, None, [d_lk], d_vals, count, rb, lb, table)


def on_device():
    device_fill()
    ctx.sync()


def on_host():
    v = ctx.download(d_vals, (count, 4))
    helper.range_host_fill_checks(host_cols, 1, None, host_lks, 1, _vp(v.ctypes.data), _vp(pows.ctypes.data), rb, lb, 0, C.cast(table, _vp), count)
    ctx.upload(d_gate, host_gate)
    ctx.upload(d_lk, host_lk)
    ctx.sync()


on_host()
want = (host_gate.copy(), host_lk.copy())
ctx.upload(d_gate, np.zeros_like(host_gate))
ctx.upload(d_lk, np.zeros_like(host_lk))
on_device()
assert np.array_equal(ctx.download(d_gate, (n, 4)), want[0]) and np.array_equal(ctx.download(d_lk, (n, 4)), want[1]), "the device fill and the host fill differ"
out = {"k": k, "range_bits": rb, "lookup_bits": lb, "units": count, "gate_cells": count * ncells, "lookup_cells": count * nlk, "device": [], "host": []}
for run in range(runs):
    for name, fn in (("device", on_device), ("host", on_host)):
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        rec = {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
        out[name].append(rec)
        print("run %d %-6s median %.3f ms (min %.3f, max %.3f) over %d" % (run, name, rec["median_ms"], rec["min_ms"], rec["max_ms"], reps), flush=True)

# ---- the lone fill between events on the stream
ms = []
for i in range(reps + 2):
    ctx.timer_start()
    device_fill()
    t = ctx.timer_stop()
    if i >= 2:
        ms.append(t)
fill_ms = float(np.median(ms))
cells = count * (ncells + nlk)
out["fill_alone_ms"], out["cells_per_s"] = round(fill_ms, 4), round(cells / fill_ms * 1e3)
out["written_gb_per_s"], out["hbm_copy_gb_per_s"] = round(cells * 32 / fill_ms / 1e6, 1), HBM_COPY_TBS * 1e3
print("fill alone: %.4f ms for %d cells = %.3g cells/s, %.1f GB/s written (a streaming copy reaches %.0f GB/s)" % (
    fill_ms, cells, cells / fill_ms * 1e3, cells * 32 / fill_ms / 1e6, HBM_COPY_TBS * 1e3), flush=True)
# ---- where the call's time goes: the kernel alone (the library's per-kernel events) and the host side of the call (its checks over the
# unit table and the table's staging), which returns before the kernel has run
ctx.profile_enable(True)
ctx.profile_reset()
host_ms = []
for _ in range(reps):
    t = time.perf_counter()
    device_fill()
    host_ms.append((time.perf_counter() - t) * 1e3)
    ctx.sync()
kernel_ms, launches = ctx.profile_get("range_fill_kernel")
ctx.profile_enable(False)
out["kernel_ms"], out["call_host_ms"] = round(kernel_ms / max(launches, 1), 4), round(float(np.median(host_ms)), 4)
out["kernel_written_gb_per_s"] = round(cells * 32 / (kernel_ms / max(launches, 1)) / 1e6, 1)
print("kernel alone: %.4f ms (%.1f GB/s written); the call's host side: %.4f ms" % (out["kernel_ms"], out["kernel_written_gb_per_s"], out["call_host_ms"]),
      flush=True)
print(json.dumps(out))
for p in (d_vals, d_gate, d_lk):
    ctx.free(p)
ctx.close()
