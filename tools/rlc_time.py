"""The phase-1 witness of an RLC circuit filled on the device against the same columns computed on the host.
Usage: python tools/rlc_time.py [k] [reps] [runs] [lookup_bits]     (defaults 19 7 3 18)

The circuit is tests/rlc_checks.py's shape A (one phase-0 gate column with q_lookup, one RLC column whose chains run down to the end of the
usable rows), proven by h2hip_plonk_create_proof_phased with phase 0 resident on the device.  Two witness callbacks:
  (a) device   h2hip_rlc_fill_chains_dev over values uploaded once, before the proofs (phase_witness_dev);
  (b) host     the same cells by tools/rlc_host_fill.cpp — one host thread on the library's host field — then h2hip_upload of the column:
               what a caller of h2hip_phase_witness_fn could do before the device fill existed.
`runs` runs of each, alternating, `reps` proofs per run: the median callback length and proof time of every run, one JSON line at the end.
Then the lone fill (events on the context's stream) next to h2hip_fr_prefix_product_dev over as many elements."""
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
from halo2_lib_amd import halo2_proofs as HP  # noqa: E402
from halo2_lib_amd import plonk as PL  # noqa: E402
from tests import rlc_checks as RC  # noqa: E402
from tests.util import fr  # noqa: E402

a = [int(v) for v in sys.argv[1:]]
k, reps, runs, lb = (a + [19, 7, 3, 18][len(a):])[:4]
_vp = C.c_void_p


def host_helper():
    src, lib = os.path.join(ROOT, "tools", "rlc_host_fill.cpp"), os.path.join(ROOT, "tools", "rlc_host_fill.so")
    deps = [src, os.path.join(ROOT, "include", "h2hip.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-shared", "-fPIC",
                               "-Wno-unused-value", "-o", lib, src])
    h = C.CDLL(lib)
    h.rlc_host_fill_chains.restype = None
    h.rlc_host_fill_chains.argtypes = [C.POINTER(_vp), _vp, _vp, C.c_size_t, _vp]
    return h


helper = host_helper()
ctx = H.Context()
t0 = time.time()
params, _ = RC.shape_a(k, lb)
circ = RC.RlcCircuit(params, 5)
kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF, precompute=True)
pk = PL.keygen(kzg, params, circ.fixed, circ.copies)
n, u = circ.n, circ.u
nvals = len(circ.values)
values = np.ascontiguousarray(fr(circ.values))
chains = (PL.RlcChainStruct * len(circ.pieces))(*[PL.RlcChainStruct(*[int(x) for x in p]) for p in circ.pieces])
cells = sum(2 * p[2] + 1 if p[3] else 2 * p[2] - 1 for p in circ.pieces)
print("k=%d: %d values in %d pieces, %d of %d usable rows written; circuit + keygen %.1f s" % (k, nvals, len(circ.pieces), cells, u, time.time() - t0), flush=True)
d_adv0 = [ctx.to_device(np.ascontiguousarray(c)) for c in circ.advice0()]
d_vals = ctx.to_device(values)
assert len(circ.phase_cols[1]) == 1, "shape A: phase 1 is the RLC column alone"
cb_ms = []


def on_device(phase, challenges, ptrs):
    t = time.perf_counter()
    PL.rlc_fill_chains(ctx, ptrs, u, d_vals, circ.pieces, challenges[0], num_values=nvals)
    ctx.sync()
    cb_ms.append((time.perf_counter() - t) * 1e3)


host_col = np.zeros((n, 4), dtype=np.uint64)


def on_host(phase, challenges, ptrs):
    t = time.perf_counter()
    g = PL.fr_limbs(challenges[0])
    cols = (_vp * 1)(_vp(host_col.ctypes.data))
    helper.rlc_host_fill_chains(cols, _vp(values.ctypes.data), C.cast(chains, _vp), len(circ.pieces), _vp(g.ctypes.data))
    ctx.upload(ptrs[0], host_col[:u])
    ctx.sync()
    cb_ms.append((time.perf_counter() - t) * 1e3)


def prove(cb):
    return PL.create_proof(pk, d_adv0, [], PL.ChaChaRng(ctx.lib, 1234), advice_on_device=True, phase_witness_dev=cb)


ref = prove(on_device)
assert prove(on_host) == ref and PL.verify_proof(pk, [], ref), "the two witnesses give different proofs / the proof does not verify"
out = {"k": k, "values": nvals, "cells": cells, "device": [], "host": []}
for run in range(runs):
    for name, cb in (("device", on_device), ("host", on_host)):
        del cb_ms[:]
        proofs = []
        for _ in range(reps):
            t = time.perf_counter()
            p = prove(cb)
            proofs.append((time.perf_counter() - t) * 1e3)
            assert p == ref
        rec = {"callback_ms": round(float(np.median(cb_ms)), 3), "proof_ms": round(float(np.median(proofs)), 3),
               "proof_min_ms": round(min(proofs), 3), "proof_max_ms": round(max(proofs), 3)}
        out[name].append(rec)
        print("run %d %-6s callback median %.3f ms, proof median %.3f ms (min %.3f, max %.3f) over %d proofs" % (
            run, name, rec["callback_ms"], rec["proof_ms"], rec["proof_min_ms"], rec["proof_max_ms"], reps), flush=True)

# ---- the lone fill next to the prefix product over as many elements
d_col = ctx.to_device(host_col)
d_in, d_out = ctx.to_device(np.ascontiguousarray(values)), ctx.malloc(32 * nvals)
gamma = 0x1234567890ABCDEF1234567890ABCDEF


def timed(fn):
    ms = []
    for i in range(reps + 2):
        ctx.timer_start()
        fn()
        t = ctx.timer_stop()
        if i >= 2:
            ms.append(t)
    return float(np.median(ms))


fill_ms = timed(lambda: PL.rlc_fill_chains(ctx, [d_col], u, d_vals, circ.pieces, gamma, num_values=nvals))
prod_ms = timed(lambda: ctx._chk(ctx.lib.h2hip_fr_prefix_product_dev(ctx.handle, _vp(d_out), _vp(d_in), nvals)))
out["fill_alone_ms"], out["fill_elements_per_s"] = round(fill_ms, 4), round(nvals / fill_ms * 1e3)
out["prefix_product_ms"], out["prefix_product_elements_per_s"] = round(prod_ms, 4), round(nvals / prod_ms * 1e3)
print("fill alone: %.4f ms for %d values = %.3g elements/s; h2hip_fr_prefix_product_dev: %.4f ms = %.3g elements/s" % (
    fill_ms, nvals, nvals / fill_ms * 1e3, prod_ms, nvals / prod_ms * 1e3), flush=True)
print(json.dumps(out))
for p in d_adv0 + [d_vals, d_col, d_in, d_out]:
    ctx.free(p)
pk.free()
kzg.free()
ctx.close()
