"""EccChip curve operations filled on the device against the same cells computed on the host.
Usage: python tools/ec_time.py [k] [limb_bits] [num_limbs] [lookup_bits] [reps] [runs] [op]     (defaults 19 88 3 18 7 3 0; op: 0 ec_add_unequal, 1 ec_double, 3 ec_sub_unequal)

The layout is the headline's shape: one gate column of 2^k rows filled down to the usable rows with ec_add_unequal units over secp256k1's p
((88, 3, 18): 908 cells and 162 lookup cells per unit, about 577 units) and one lookup-advice column that takes their lookup cells; the
points lie in a device buffer of their own (what a kernel before the fill produced).
  (a) device   plonk.ec_fill_with_ranges (h2hip_ec_fill_dev, then one h2hip_range_fill_checks_dev per width) on columns resident on the
               device, the unit table and the range tables built once, then a wait for the stream;
  (a') default the same call given the units as tuples and the lookup slots: it builds both tables on every call (the unit table in
               Python, the range tables by one h2hip_ec_range_checks call);
  (a-gap)      (a) with every width's table reordered gap-major here in the tool (all units' first gap of that width, then their second, ...),
               as §3l's tables were ordered: whether the library's unit-major order inside a width spares the range call anything;
  (b) host     what was possible before: a download of the points, the same cells by tools/ec_host_fill.cpp — one host thread on the
               library's host field, the library's own per-unit and per-segment code — and h2hip_upload of the gate and the lookup column.
`runs` runs of each, alternating, `reps` repetitions per run: the median of every run, one JSON line at the end.  Then each kernel between
the library's own per-kernel events, and the host time before the calls return."""
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
k, nbits, nlimbs, lb, reps, runs, op = (a + [19, 88, 3, 18, 7, 3, 0][len(a):])[:7]
_vp = C.c_void_p
SECP_P = (1 << 256) - (1 << 32) - 977


def host_helper():
    src, lib = os.path.join(ROOT, "tools", "ec_host_fill.cpp"), os.path.join(ROOT, "tools", "ec_host_fill.so")
    deps = [src, os.path.join(ROOT, "include", "h2hip.h")] + [os.path.join(ROOT, "halo2-lib_amd", "csrc", f) for f in ("ec_fill.cuh", "fp_mul.cuh", "range_fill.cuh", "trace_place.cuh")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-shared", "-fPIC",
                               "-Wno-unused-value", "-o", lib, src])
    h = C.CDLL(lib)
    h.ec_host_fill.restype = C.c_int
    h.ec_host_fill.argtypes = [C.POINTER(_vp), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(_vp), C.c_size_t, _vp, C.c_uint32, _vp, _vp, _vp,
                               C.POINTER(C.c_uint64), C.c_size_t]
    return h


helper = host_helper()
ctx = H.Context()
n = 1 << k
u = n - 7                                     # the usable rows with six blinding factors
params = PL.fp_params(nbits, nlimbs, lb, SECP_P)
lay = PL.ec_layout(params, op)
count = (u - 2) // lay.num_cells              # the last cell two rows above the end, as gate.max_rows leaves them
assert count * lay.num_lookup_cells <= u, "the lookup cells do not fit one column"
nres, npt = 9 * nlimbs + 3, 2 * (nlimbs + 1)
units = [(0, j * lay.num_cells, 2 * npt * j, 2 * npt * j + npt) for j in range(count)]
slots = [j * lay.num_lookup_cells for j in range(count)]
table = PL.ec_op_table(units)                 # built once, as the range tables
range_tables = PL.ec_range_tables(None, 1, params, op, table, slots)


def gap_major(tab):
    """a width's table (unit-major: unit 0's gaps of that width, unit 1's, ...) with the units of one gap consecutive"""
    per = len(tab) // count
    out = (PL.RangeCheckStruct * len(tab))()
    for j in range(per):
        for i in range(count):
            src = tab[i * per + j]
            out[j * count + i] = PL.RangeCheckStruct(src.column, src.row, src.a_offset, src.b_offset, src.lookup_slot)
    return out


gap_tables = [(bits, gap_major(tab)) for bits, tab in range_tables]
g = np.random.default_rng(k)
mask = (1 << nbits) - 1
ops = []
for _ in range(4 * count):                    # arbitrary reduced coordinates: x, y of P, x, y of Q
    x = int.from_bytes(g.bytes(40), "little") % SECP_P
    ops += [(x >> (nbits * i)) & mask for i in range(nlimbs)] + [x % R]
vals = fr(ops)
print("k=%d: %d %s units (%d, %d, %d): %d gate cells (%d own) and %d lookup cells, %d range calls per fill" % (
    k, count, {0: "ec_add_unequal", 1: "ec_double", 3: "ec_sub_unequal"}[op], nbits, nlimbs, lb, count * lay.num_cells, count * lay.num_own_cells,
    count * lay.num_lookup_cells, len(range_tables)), flush=True)

d_vals = ctx.to_device(vals)
d_res = ctx.to_device(np.zeros((count * nres, 4), dtype=np.uint64))
d_gate = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))
d_lk = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))
host_gate, host_lk, host_res = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64), np.zeros((count * nres, 4), dtype=np.uint64)
host_cols, host_lks = (_vp * 1)(_vp(host_gate.ctypes.data)), (_vp * 1)(_vp(host_lk.ctypes.data))
host_slots = (C.c_uint64 * count)(*slots)


def big_fill():
    PL.ec_fill(ctx, [d_gate], u, None, params, op, d_vals, len(ops), d_res, count * nres, table)


def device_fill(tables=range_tables):
    PL.ec_fill_with_ranges(ctx, [d_gate], u, None, [d_lk], params, op, d_vals, len(ops), d_res, count * nres, table, range_tables=tables)


def on_device():
    device_fill()
    ctx.sync()


def on_device_gap_major():
    device_fill(gap_tables)
    ctx.sync()


def on_device_default():
    PL.ec_fill_with_ranges(ctx, [d_gate], u, None, [d_lk], params, op, d_vals, len(ops), d_res, count * nres, units, slots)
    ctx.sync()


def on_host():
    v = ctx.download(d_vals, (len(ops), 4))
    code = helper.ec_host_fill(host_cols, 1, None, host_lks, 1, C.cast(C.pointer(params), _vp), op, _vp(v.ctypes.data), _vp(host_res.ctypes.data),
                               C.cast(table, _vp), host_slots, count)
    assert code == 0
    ctx.upload(d_gate, host_gate)
    ctx.upload(d_lk, host_lk)
    ctx.sync()


on_host()
want = (host_gate.copy(), host_lk.copy())
for fn in (on_device, on_device_gap_major):
    ctx.upload(d_gate, np.zeros_like(host_gate))
    ctx.upload(d_lk, np.zeros_like(host_lk))
    fn()
    assert np.array_equal(ctx.download(d_gate, (n, 4)), want[0]) and np.array_equal(ctx.download(d_lk, (n, 4)), want[1]), "the device fill and the host fill differ"
out = {"k": k, "limb_bits": nbits, "num_limbs": nlimbs, "lookup_bits": lb, "op": op, "units": count, "gate_cells": count * lay.num_cells,
       "lookup_cells": count * lay.num_lookup_cells, "range_calls": len(range_tables), "device": [], "device_default": [], "device_gap_major": [], "host": []}
for run in range(runs):
    for name, fn in (("device", on_device), ("device_default", on_device_default), ("device_gap_major", on_device_gap_major), ("host", on_host)):
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        rec = {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
        out[name].append(rec)
        print("run %d %-16s median %.3f ms (min %.3f, max %.3f) over %d" % (run, name, rec["median_ms"], rec["min_ms"], rec["max_ms"], reps), flush=True)

# ---- where the time goes: each kernel alone (the library's per-kernel events), the host side of the fused call (its checks over the unit
# table and the tables' staging; it returns before the kernels have run), of the whole convenience call and of its range calls in both orders
ctx.profile_enable(True)
ctx.profile_reset()
host_ms, all_ms, gap_ms = [], [], []
for _ in range(reps):
    t = time.perf_counter()
    big_fill()
    host_ms.append((time.perf_counter() - t) * 1e3)
    ctx.sync()
for _ in range(reps):
    t = time.perf_counter()
    device_fill()
    all_ms.append((time.perf_counter() - t) * 1e3)
    ctx.sync()
for name in ("ec_solve_kernel", "ec_place_kernel", "range_fill_kernel"):
    ms, launches = ctx.profile_get(name)
    out[name + "_ms"] = round(ms / max(launches, 1), 4)
ctx.profile_enable(False)
for _ in range(reps):
    t = time.perf_counter()
    device_fill(gap_tables)
    gap_ms.append((time.perf_counter() - t) * 1e3)
    ctx.sync()
out["ec_call_host_ms"], out["all_calls_host_ms"] = round(float(np.median(host_ms)), 4), round(float(np.median(all_ms)), 4)
out["all_calls_host_gap_major_ms"] = round(float(np.median(gap_ms)), 4)
print("kernels alone: solve %.4f ms, place %.4f ms, one range fill %.4f ms; host time before return: the fused call %.4f ms, all %d calls %.4f ms "
      "(gap-major tables: %.4f ms)" % (out["ec_solve_kernel_ms"], out["ec_place_kernel_ms"], out["range_fill_kernel_ms"], out["ec_call_host_ms"],
                                       1 + len(range_tables), out["all_calls_host_ms"], out["all_calls_host_gap_major_ms"]), flush=True)
print(json.dumps(out))
for p in (d_vals, d_res, d_gate, d_lk):
    ctx.free(p)
ctx.close()
