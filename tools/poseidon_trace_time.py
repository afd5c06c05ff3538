"""The gate cells of an in-circuit Poseidon Merkle tree filled on the device against the same cells computed on the host.
Usage: python tools/poseidon_trace_time.py [k] [log_leaves] [reps] [runs]     (defaults 19 10 7 3)

The layout is one thread of a t = 3 (8, 57) tree over 2^log_leaves leaves: the leaves, then 2^log_leaves - 1 two-to-one hash_fix_len_array
traces (4,506 cells each) level by level, laid down gate columns of 2^k rows that are left at row 2^k - 10 (assign_witnesses' placement).
Every level reads the digest cells of the level below from their columns.
  (a) device   one h2hip_poseidon_fill_hashes_dev call per level on columns resident on the device, then a wait for the stream;
  (a1) tree    h2hip_poseidon_merkle_tree_dev over the leaves first, then ONE fill call for all levels whose inputs are the tree's nodes
               (the same cells: a level no longer waits for the level below, whose traces take one lane's serial time whatever its width);
  (b) host     what was possible before: the same cells by tools/poseidon_host_fill.cpp — one host thread on the library's host field —
               and h2hip_upload of every gate column.
`runs` runs of each, alternating, `reps` repetitions per run: the median of every run, one JSON line at the end.  Then the lone fill (events on
the context's stream), cells per second, and the bytes it writes per second next to the HBM bandwidth a streaming copy reaches."""
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
from halo2_lib_amd import poseidon as PS  # noqa: E402
from tests.util import fr, full_range_fr  # noqa: E402

a = [int(v) for v in sys.argv[1:]]
k, log_leaves, reps, runs = (a + [19, 10, 7, 3][len(a):])[:4]
_vp = C.c_void_p
T, R_F, R_P = 3, 8, 57
HBM_COPY_TBS = 6.29   # a float4 copy on this part (8.0 TB/s is the specification)


def host_helper():
    src, lib = os.path.join(ROOT, "tools", "poseidon_host_fill.cpp"), os.path.join(ROOT, "tools", "poseidon_host_fill.so")
    deps = [src, os.path.join(ROOT, "include", "h2hip.h"), os.path.join(ROOT, "halo2-lib_amd", "csrc", "poseidon_trace.cuh"),
            os.path.join(ROOT, "halo2-lib_amd", "csrc", "trace_place.cuh")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-shared", "-fPIC",
                               "-Wno-unused-value", "-o", lib, src])
    h = C.CDLL(lib)
    h.poseidon_host_fill_hashes.restype = None
    h.poseidon_host_fill_hashes.argtypes = [C.POINTER(_vp), C.c_size_t, C.POINTER(C.c_uint32), _vp, C.c_uint32, _vp, C.c_size_t, _vp, C.c_uint32, C.c_uint32,
                                            C.c_uint32]
    return h


helper = host_helper()
ctx = H.Context()
hs = PS.PoseidonHasher.new(ctx, T, R_F, R_P)
hs.select_optimized()
n, leaves = 1 << k, 1 << log_leaves
bp = n - 10                                   # gate.max_rows - 1 with six blinding factors
cells, offs = hs.trace_layout(2, 0)
total = leaves + (leaves - 1) * cells
ncols = 1 if total <= bp + 1 else 1 + -(-(total - (bp + 1)) // bp)
bps = [bp] * (ncols - 1)


def where(i):
    """(column, row) of thread cell i (its first cell, where the break point duplicates it)"""
    if i <= bp:
        return 0, i
    c, r = divmod(i - (bp + 1), bp)
    return 1 + c, 1 + r


flat = lambda i: where(i)[0] * n + where(i)[1]
# level 0 hashes pairs of leaves; level l the digests of level l - 1; unit j of a level starts at thread cell first[l] + j * cells
levels, every, start, prev = [], [], leaves, None
w = leaves // 2
while w >= 1:
    units = []
    for j in range(w):
        if prev is None:
            off, stride = 2 * j, 1
        else:
            d0, d1 = flat(prev + 2 * j * cells + offs[1]), flat(prev + (2 * j + 1) * cells + offs[1])
            off, stride = d0, d1 - d0
        units.append(where(start + j * cells) + (off, stride, 0))
        every.append(where(start + j * cells) + (2 * (w + j), 1, 0))      # node w + j of the heap-layout tree hashes nodes 2 (w + j) and 2 (w + j) + 1
    levels.append(PS.hash_table(units))       # built once: a table of structs costs milliseconds to build
    prev, start, w = start, start + w * cells, w // 2
every = PS.hash_table(every)
nunits = leaves - 1
print("k=%d: %d leaves, %d hashes of %d cells = %d cells in %d gate columns, %d calls" % (k, leaves, nunits, cells, total - leaves, ncols, len(levels)), flush=True)

leaf_vals = full_range_fr(leaves, 7, edges=False)
host = np.zeros((ncols * n, 4), dtype=np.uint64)
host[:leaves] = leaf_vals
d_gate = ctx.to_device(host)
d_cols = [d_gate + 32 * n * c for c in range(ncols)]
spec = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(x).reshape(-1, 4) for x in hs.optimized_spec()] + [fr([1 << 64])]))
host_cols = (_vp * ncols)(*[_vp(host.ctypes.data + 32 * n * c) for c in range(ncols)])
host_bps = (C.c_uint32 * max(ncols - 1, 1))(*bps)


def device_fill():
    for tab in levels:
        hs.fill_hashes(ctx, d_cols, n - 7, bps if bps else None, d_gate, ncols * n, 2, tab)


def on_device():
    device_fill()
    ctx.sync()


d_nodes = ctx.malloc(32 * 2 * leaves)
hs._select()


def on_tree():
    ctx._chk(ctx.lib.h2hip_poseidon_merkle_tree_dev(ctx.handle, _vp(d_nodes), _vp(d_gate), log_leaves))
    hs.fill_hashes(ctx, d_cols, n - 7, bps if bps else None, d_nodes, 2 * leaves, 2, every)
    ctx.sync()


def on_host():
    for tab in levels:
        helper.poseidon_host_fill_hashes(host_cols, ncols, host_bps if bps else None, _vp(host.ctypes.data), 2, C.cast(tab, _vp), len(tab), _vp(spec.ctypes.data),
                                         T, R_F, R_P)
    for c in range(ncols):
        ctx.upload(d_cols[c], host[c * n:(c + 1) * n])
    ctx.sync()


on_host()
want = host.copy()
ctx.upload(d_gate, np.zeros_like(host))
ctx.upload(d_gate, leaf_vals)
on_device()
assert np.array_equal(ctx.download(d_gate, host.shape), want), "the device fill and the host fill differ"
ctx.upload(d_gate, np.zeros_like(host))
ctx.upload(d_gate, leaf_vals)
on_tree()
assert np.array_equal(ctx.download(d_gate, host.shape), want), "the one-call fill over the tree's nodes and the host fill differ"
root = want[flat(start - cells + offs[1])]
assert np.array_equal(root, hs.merkle_tree(leaf_vals)[1]), "the last digest cell is not the tree's root"
out = {"k": k, "leaves": leaves, "hashes": nunits, "cells": total - leaves, "columns": ncols, "device": [], "tree": [], "host": []}
for run in range(runs):
    for name, fn in (("device", on_device), ("tree", on_tree), ("host", on_host)):
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
written = (total - leaves) * 32
out["fill_alone_ms"], out["cells_per_s"] = round(fill_ms, 4), round((total - leaves) / fill_ms * 1e3)
out["written_gb_per_s"], out["hbm_copy_gb_per_s"] = round(written / fill_ms / 1e6, 1), HBM_COPY_TBS * 1e3
print("fill alone: %.4f ms for %d cells = %.3g cells/s, %.1f GB/s written (a streaming copy reaches %.0f GB/s)" % (
    fill_ms, total - leaves, (total - leaves) / fill_ms * 1e3, written / fill_ms / 1e6, HBM_COPY_TBS * 1e3), flush=True)
print(json.dumps(out))
ctx.free(d_gate)
ctx.free(d_nodes)
ctx.close()
