"""Strict curve additions filled on the device against the same cells computed on the host (tools/ec_time.py's sibling).
Usage: python tools/ec_time_strict.py [k] [limb_bits] [num_limbs] [lookup_bits] [reps] [runs] [op] [mask]     (defaults 19 88 3 18 7 3 0 7; op: 0 ec_add_unequal, 3 ec_sub_unequal)

One gate column of 2^k rows filled down to the usable rows with strict ec_add_unequal units over secp256k1's p — each the comparison of
check_points_are_unequal (mask 7: both points non-strict) and the addition right behind it — and one lookup-advice column that takes their
lookup cells; the points lie in a device buffer of their own.
  (a) device   plonk.ec_fill_strict_with_ranges with its tables built once: h2hip_fp_cmp_fill_dev and its one range call, h2hip_ec_fill_dev
               and one range call per width, then a wait for the stream;
  (b) host     a download of the points, the same cells by tools/ec_host_fill.cpp (cmp_host_fill, then ec_host_fill: one host thread on the
               library's host field, the library's own per-unit and per-segment code) and h2hip_upload of the gate and the lookup column.
`runs` runs of each, alternating, `reps` repetitions per run, after a bit-for-bit comparison of both sides: the median of every run, one
JSON line at the end.  Then each kernel between the library's own per-kernel events, and the host time before the calls return."""
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
k, nbits, nlimbs, lb, reps, runs, op, mask = (a + [19, 88, 3, 18, 7, 3, 0, 7][len(a):])[:8]
_vp = C.c_void_p
SECP_P = (1 << 256) - (1 << 32) - 977


def host_helper():
    src, lib = os.path.join(ROOT, "tools", "ec_host_fill.cpp"), os.path.join(ROOT, "tools", "ec_host_fill.so")
    deps = [src, os.path.join(ROOT, "include", "h2hip.h")] + [os.path.join(ROOT, "halo2-lib_amd", "csrc", f) for f in ("ec_fill.cuh", "fp_cmp.cuh", "fp_mul.cuh", "range_fill.cuh", "trace_place.cuh")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-shared", "-fPIC",
                               "-Wno-unused-value", "-o", lib, src])
    h = C.CDLL(lib)
    for fn in (h.ec_host_fill, h.cmp_host_fill):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(_vp), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(_vp), C.c_size_t, _vp, C.c_uint32, _vp, _vp, _vp,
                       C.POINTER(C.c_uint64), C.c_size_t]
    return h


helper = host_helper()
ctx = H.Context()
n = 1 << k
u = n - 7                                     # the usable rows with six blinding factors
params = PL.fp_params(nbits, nlimbs, lb, SECP_P)
lay, cl = PL.ec_layout(params, op), PL.fp_cmp_layout(params, mask)
cells, lookups = lay.num_cells + cl.num_cells, lay.num_lookup_cells + cl.num_lookup_cells
count = (u - 2) // cells                      # the last cell two rows above the end, as gate.max_rows leaves them
assert count * lookups <= u, "the lookup cells do not fit one column"
nres, cres, npt = 9 * nlimbs + 3, cl.results_per_unit, 2 * (nlimbs + 1)
units = [(0, j * cells, 2 * npt * j, 2 * npt * j + npt) for j in range(count)]
slots = [j * lookups for j in range(count)]
g = np.random.default_rng(k)
maskn = (1 << nbits) - 1
ops = []
for _ in range(4 * count):                    # arbitrary reduced coordinates: x, y of P, x, y of Q
    x = int.from_bytes(g.bytes(40), "little") % SECP_P
    ops += [(x >> (nbits * i)) & maskn for i in range(nlimbs)] + [x % R]
vals = fr(ops)
d_vals = ctx.to_device(vals)
d_res = ctx.to_device(np.zeros((count * nres, 4), dtype=np.uint64))
d_cres = ctx.to_device(np.zeros((count * cres, 4), dtype=np.uint64))
d_gate = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))
d_lk = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))
host_gate, host_lk = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
host_res, host_cres = np.zeros((count * nres, 4), dtype=np.uint64), np.zeros((count * cres, 4), dtype=np.uint64)
host_cols, host_lks = (_vp * 1)(_vp(host_gate.ctypes.data)), (_vp * 1)(_vp(host_lk.ctypes.data))


def device_fill(tables=None):
    return PL.ec_fill_strict_with_ranges(ctx, [d_gate], u, None, [d_lk], params, op, mask, d_vals, len(ops), d_res, count * nres, d_cres, count * cres,
                                         units, slots, tables=tables)


_eq, _opc, tables = device_fill()             # the tables, built once
cmp_table, cmp_ranges, ec_table, ec_ranges = tables[2]
cmp_slots, ec_slots = (C.c_uint64 * count)(*slots), (C.c_uint64 * count)(*[s + cl.num_lookup_cells for s in slots])
print("k=%d: %d strict %s units, mask %d, (%d, %d, %d): %d gate cells and %d lookup cells, %d range calls per fill" % (
    k, count, {0: "ec_add_unequal", 3: "ec_sub_unequal"}[op], mask, nbits, nlimbs, lb, count * cells, count * lookups,
    len(cmp_ranges) + len(ec_ranges)), flush=True)


def on_device():
    device_fill(tables)
    ctx.sync()


def on_host():
    v = ctx.download(d_vals, (len(ops), 4))
    pp, vp = C.cast(C.pointer(params), _vp), _vp(v.ctypes.data)
    code = helper.cmp_host_fill(host_cols, 1, None, host_lks, 1, pp, mask, vp, _vp(host_cres.ctypes.data), C.cast(cmp_table, _vp), cmp_slots, count)
    code |= helper.ec_host_fill(host_cols, 1, None, host_lks, 1, pp, op, vp, _vp(host_res.ctypes.data), C.cast(ec_table, _vp), ec_slots, count)
    assert code == 0
    ctx.upload(d_gate, host_gate)
    ctx.upload(d_lk, host_lk)
    ctx.sync()


on_host()
want = (host_gate.copy(), host_lk.copy())
ctx.upload(d_gate, np.zeros_like(host_gate))
ctx.upload(d_lk, np.zeros_like(host_lk))
on_device()
assert np.array_equal(ctx.download(d_gate, (n, 4)), want[0]) and np.array_equal(ctx.download(d_lk, (n, 4)), want[1]), "the device fill and the host fill differ"
out = {"k": k, "limb_bits": nbits, "num_limbs": nlimbs, "lookup_bits": lb, "op": op, "mask": mask, "units": count, "gate_cells": count * cells,
       "lookup_cells": count * lookups, "range_calls": len(cmp_ranges) + len(ec_ranges), "device": [], "host": []}
for run in range(runs):
    for name, fn in (("device", on_device), ("host", on_host)):
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        rec = {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
        out[name].append(rec)
        print("run %d %-8s median %.3f ms (min %.3f, max %.3f) over %d" % (run, name, rec["median_ms"], rec["min_ms"], rec["max_ms"], reps), flush=True)

ctx.profile_enable(True)
ctx.profile_reset()
fused_ms, all_ms = [], []
for _ in range(reps):
    t = time.perf_counter()
    PL.fp_cmp_fill(ctx, [d_gate], u, None, params, mask, d_vals, len(ops), d_cres, count * cres, cmp_table)
    PL.ec_fill(ctx, [d_gate], u, None, params, op, d_vals, len(ops), d_res, count * nres, ec_table)
    fused_ms.append((time.perf_counter() - t) * 1e3)
    ctx.sync()
for _ in range(reps):
    t = time.perf_counter()
    device_fill(tables)
    all_ms.append((time.perf_counter() - t) * 1e3)
    ctx.sync()
for name in ("fp_cmp_solve_kernel", "fp_cmp_place_kernel", "ec_solve_kernel", "ec_place_kernel", "range_fill_kernel"):
    ms, launches = ctx.profile_get(name)
    out[name + "_ms"] = round(ms / max(launches, 1), 4)
ctx.profile_enable(False)
out["fused_calls_host_ms"], out["all_calls_host_ms"] = round(float(np.median(fused_ms)), 4), round(float(np.median(all_ms)), 4)
print("kernels alone: cmp solve %.4f ms, cmp place %.4f ms, ec solve %.4f ms, ec place %.4f ms, one range fill %.4f ms; host time before return: "
      "the two fused calls %.4f ms, all %d calls %.4f ms" % (out["fp_cmp_solve_kernel_ms"], out["fp_cmp_place_kernel_ms"], out["ec_solve_kernel_ms"],
                                                            out["ec_place_kernel_ms"], out["range_fill_kernel_ms"], out["fused_calls_host_ms"],
                                                            2 + out["range_calls"], out["all_calls_host_ms"]), flush=True)
print(json.dumps(out))
for p in (d_vals, d_res, d_cres, d_gate, d_lk):
    ctx.free(p)
ctx.close()
