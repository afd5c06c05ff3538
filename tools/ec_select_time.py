"""Window selections filled on the device against the same cells computed on the host (tools/ec_time_strict.py's sibling).
Usage: python tools/ec_select_time.py [k] [limb_bits] [num_limbs] [lookup_bits] [reps] [runs] [window_bits] [tables]     (defaults 19 88 3 18 7 3 4 64)

One gate column of 2^k rows filled down to the usable rows with ec_select_from_bits units over secp256k1's p at the window given; unit j
selects from table j mod `tables` (the cached multiples of one base point) by bits of its own; tables and bits lie in one device buffer.
  (a) device   plonk.ec_select_fill with its unit table built once (h2hip_ec_select_fill_dev: two kernels), then a wait for the stream;
  (b) host     a download of the tables and the bits, the same cells by tools/ec_select_host_fill.cpp (one host thread on the library's host
               field, the library's own per-unit and per-segment code) and h2hip_upload of the gate column and of the selected points.
`runs` runs of each, alternating, `reps` repetitions per run, after a bit-for-bit comparison of both sides: the median of every run, one
JSON line at the end.  Then each kernel between the library's own per-kernel events, and the host time before the call returns; and the same
three figures for num_to_bits at 256 / window_bits * window_bits bits over as many scalars as fill the column."""
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
k, nbits, nlimbs, lb, reps, runs, w, ntab = (a + [19, 88, 3, 18, 7, 3, 4, 64][len(a):])[:8]
_vp = C.c_void_p
SECP_P = (1 << 256) - (1 << 32) - 977


def host_helper():
    src, lib = os.path.join(ROOT, "tools", "ec_select_host_fill.cpp"), os.path.join(ROOT, "tools", "ec_select_host_fill.so")
    deps = [src, os.path.join(ROOT, "include", "h2hip.h")] + [os.path.join(ROOT, "halo2-lib_amd", "csrc", f) for f in ("ec_select.cuh", "fp_mul.cuh", "range_fill.cuh", "trace_place.cuh")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-shared", "-fPIC",
                               "-Wno-unused-value", "-o", lib, src])
    h = C.CDLL(lib)
    h.ec_select_host_fill.restype = h.num_to_bits_host_fill.restype = C.c_int
    h.ec_select_host_fill.argtypes = [C.POINTER(_vp), C.c_size_t, C.POINTER(C.c_uint32), _vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_size_t]
    h.num_to_bits_host_fill.argtypes = [C.POINTER(_vp), C.c_size_t, C.POINTER(C.c_uint32), _vp, _vp, C.c_uint32, _vp, C.c_size_t]
    return h


helper = host_helper()
ctx = H.Context()
n = 1 << k
u = n - 7                                     # the usable rows with six blinding factors
params = PL.fp_params(nbits, nlimbs, lb, SECP_P)
cells = PL.ec_select_layout(params, PL.EC_SELECT_FROM_BITS, w).num_cells
count = (u - 2) // cells                      # the last cell two rows above the end, as gate.max_rows leaves them
npt, m = 2 * (nlimbs + 1), 1 << w
g = np.random.default_rng(k)
maskn = (1 << nbits) - 1
ops = []
for _ in range(2 * m * ntab):                 # arbitrary reduced coordinates
    x = int.from_bytes(g.bytes(40), "little") % SECP_P
    ops += [(x >> (nbits * i)) & maskn for i in range(nlimbs)] + [x % R]
at_bits = len(ops)
ops += [int(b) for b in g.integers(0, 2, w * count)]
units = PL.ec_select_table([(0, j * cells, (j % ntab) * m * npt, 0, at_bits + w * j) for j in range(count)])   # built once
vals = fr(ops)
d_vals = ctx.to_device(vals)
d_res = ctx.to_device(np.zeros((count * npt, 4), dtype=np.uint64))
d_gate = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))
host_gate, host_res = np.zeros((n, 4), dtype=np.uint64), np.zeros((count * npt, 4), dtype=np.uint64)
host_cols = (_vp * 1)(_vp(host_gate.ctypes.data))
pp = C.cast(C.pointer(params), _vp)
print("k=%d: %d ec_select_from_bits units, w = %d, %d tables, (%d, %d, %d): %d gate cells" % (k, count, w, ntab, nbits, nlimbs, lb, count * cells), flush=True)


def device_fill():
    PL.ec_select_fill(ctx, [d_gate], u, None, params, PL.EC_SELECT_FROM_BITS, w, d_vals, len(ops), d_res, count * npt, units, count)


def on_device():
    device_fill()
    ctx.sync()


def on_host():
    v = ctx.download(d_vals, (len(ops), 4))
    code = helper.ec_select_host_fill(host_cols, 1, None, pp, PL.EC_SELECT_FROM_BITS, w, _vp(v.ctypes.data), _vp(host_res.ctypes.data), C.cast(units, _vp), count)
    assert code == 0
    ctx.upload(d_gate, host_gate)
    ctx.upload(d_res, host_res)
    ctx.sync()


def timed(sides, out):
    for run in range(runs):
        for name, fn in sides:
            ms = []
            for _ in range(reps):
                t = time.perf_counter()
                fn()
                ms.append((time.perf_counter() - t) * 1e3)
            rec = {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
            out[name].append(rec)
            print("run %d %-12s median %.3f ms (min %.3f, max %.3f) over %d" % (run, name, rec["median_ms"], rec["min_ms"], rec["max_ms"], reps), flush=True)


on_host()
want = (host_gate.copy(), host_res.copy())
ctx.upload(d_gate, np.zeros_like(host_gate))
ctx.upload(d_res, np.zeros_like(host_res))
on_device()
assert np.array_equal(ctx.download(d_gate, (n, 4)), want[0]) and np.array_equal(ctx.download(d_res, (count * npt, 4)), want[1]), "the device fill and the host fill differ"
out = {"k": k, "limb_bits": nbits, "num_limbs": nlimbs, "lookup_bits": lb, "window_bits": w, "tables": ntab, "units": count, "gate_cells": count * cells,
       "device": [], "host": [], "bits_device": [], "bits_host": []}
timed((("device", on_device), ("host", on_host)), out)

ctx.profile_enable(True)
ctx.profile_reset()
call_ms = []
for _ in range(reps):
    t = time.perf_counter()
    device_fill()
    call_ms.append((time.perf_counter() - t) * 1e3)
    ctx.sync()
for name in ("ec_select_solve_kernel", "ec_select_place_kernel"):
    ms, launches = ctx.profile_get(name)
    out[name + "_ms"] = round(ms / max(launches, 1), 4)
ctx.profile_enable(False)
out["call_host_ms"] = round(float(np.median(call_ms)), 4)
print("kernels alone: solve %.4f ms, place %.4f ms; host time before the call returns %.4f ms" % (
    out["ec_select_solve_kernel_ms"], out["ec_select_place_kernel_ms"], out["call_host_ms"]), flush=True)

# ---- num_to_bits: scalars cut into chunks of nb bits, as many as fill the column
nb = 256 // w * w if 256 // w * w <= 253 else 252
bcells = PL.num_to_bits_layout(nb)[0]
bcount = (u - 2) // bcells
scal = fr([int.from_bytes(g.bytes(32), "little") % (1 << nb) for _ in range(bcount)])
bunits = PL.bits_unit_table([(0, j * bcells, j) for j in range(bcount)])
d_scal = ctx.to_device(scal)
d_bits = ctx.to_device(np.zeros((bcount * nb, 4), dtype=np.uint64))
host_bits = np.zeros((bcount * nb, 4), dtype=np.uint64)
host_gate[:] = 0
ctx.upload(d_gate, host_gate)


def bits_device():
    PL.num_to_bits_fill(ctx, [d_gate], u, None, d_scal, bcount, d_bits, bcount * nb, nb, bunits, bcount)
    ctx.sync()


def bits_host():
    v = ctx.download(d_scal, (bcount, 4))
    assert helper.num_to_bits_host_fill(host_cols, 1, None, _vp(v.ctypes.data), _vp(host_bits.ctypes.data), nb, C.cast(bunits, _vp), bcount) == 0
    ctx.upload(d_gate, host_gate)
    ctx.upload(d_bits, host_bits)
    ctx.sync()


bits_host()
want = (host_gate.copy(), host_bits.copy())
ctx.upload(d_gate, np.zeros_like(host_gate))
bits_device()
assert np.array_equal(ctx.download(d_gate, (n, 4)), want[0]) and np.array_equal(ctx.download(d_bits, (bcount * nb, 4)), want[1]), "num_to_bits: the device fill and the host fill differ"
out["num_bits"], out["bits_units"] = nb, bcount
print("num_to_bits: %d units of %d bits, %d gate cells" % (bcount, nb, bcount * bcells), flush=True)
timed((("bits_device", bits_device), ("bits_host", bits_host)), out)
ctx.profile_enable(True)
ctx.profile_reset()
for _ in range(reps):
    bits_device()
ms, launches = ctx.profile_get("num_to_bits_kernel")
out["num_to_bits_kernel_ms"] = round(ms / max(launches, 1), 4)
ctx.profile_enable(False)
print("num_to_bits_kernel alone %.4f ms" % out["num_to_bits_kernel_ms"], flush=True)
print(json.dumps(out))
for p in (d_vals, d_res, d_gate, d_scal, d_bits):
    ctx.free(p)
ctx.close()
