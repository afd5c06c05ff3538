"""The phase-1 gate column of an RLC circuit filled on the device against the same cells computed on the host.
Usage: python tools/gate_chain_time.py [k] [reps] [runs] [lookup_bits] [max_len]     (defaults 19 7 3 18 30)

The circuit is tests/gate_chain_checks.py's SelectCircuit with one phase-1 gate column: one RLC column whose chains run down to the end of
the usable rows, and the gate column filled down to the usable rows with select_by_indicator chains of max_len pairs (variable-length
selections: chain c picks running sum len_c - 1 of its window of the long RLC chain), proven by h2hip_plonk_create_proof_phased with phase 0
resident on the device.  Two witness callbacks:
  (a) device   h2hip_rlc_fill_chains_dev, then h2hip_gate_fill_chains_dev with a_dev = the RLC column and b_dev = the phase-0 column;
  (b) host     what was possible before the gate fill: h2hip_rlc_fill_chains_dev, a download of the RLC column, the selection chains by
               tools/gate_host_fill.cpp — one host thread on the library's host field — and h2hip_upload of the gate column.
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
from tests import gate_chain_checks as GC  # noqa: E402
from tests.util import fr  # noqa: E402

a = [int(v) for v in sys.argv[1:]]
k, reps, runs, lb, max_len = (a + [19, 7, 3, 18, 30][len(a):])[:5]
_vp = C.c_void_p


def host_helper():
    src, lib = os.path.join(ROOT, "tools", "gate_host_fill.cpp"), os.path.join(ROOT, "tools", "gate_host_fill.so")
    deps = [src, os.path.join(ROOT, "include", "h2hip.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-shared", "-fPIC",
                               "-Wno-unused-value", "-o", lib, src])
    h = C.CDLL(lib)
    h.gate_host_fill_chains.restype = None
    h.gate_host_fill_chains.argtypes = [C.POINTER(_vp), _vp, _vp, _vp, C.c_size_t]
    return h


helper = host_helper()
ctx = H.Context()
t0 = time.time()
params = PL.RlcCircuitParams.new(k, [1, 1], [1, 0], 1, 0, lb, [1], 1)
u = (1 << k) - 7   # n minus the blinding rows and the row of l_last
g = np.random.default_rng(19)
# chain c: max_len pairs over the running sums at rows 28 + 2 max_len c ... of the long RLC chain (28: where tests/rlc_checks.py starts it)
nchains = (u - 8) // (3 * max_len + 1)
chains = [(max_len, int(ln), [(28 + 2 * max_len * c, max_len)]) for c, ln in enumerate(g.integers(1, max_len + 1, size=nchains))]
circ = GC.SelectCircuit(params, 5, chains=chains)
assert circ.u >= nchains * (3 * max_len + 1), (circ.u, u)
kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF, precompute=True)
pk = PL.keygen(kzg, params, circ.fixed, circ.copies)
n, u = circ.n, circ.u
nvals = len(circ.values)
values = np.ascontiguousarray(fr(circ.values))
pieces = circ.gate_pieces
pairs = sum(p[2] for p in pieces)
cells = sum(GC.cell_count(p[2], p[3]) for p in pieces)
gate_chains = (PL.GateChainStruct * len(pieces))(*[PL.GateChainStruct(*[int(x) for x in p]) for p in pieces])
print("k=%d: %d RLC values; %d pairs in %d select chains of %d, %d of %d usable rows of the gate column written; circuit + keygen %.1f s" % (
    k, nvals, pairs, len(pieces), max_len, cells, u, time.time() - t0), flush=True)
adv0 = [np.ascontiguousarray(c) for c in circ.advice0()]
d_adv0 = [ctx.to_device(c) for c in adv0]
d_vals = ctx.to_device(values)
assert len(circ.phase_cols[1]) == 2, "phase 1 is the gate column and the RLC column"
cb_ms = []


def on_device(phase, challenges, ptrs):
    t = time.perf_counter()
    PL.rlc_fill_chains(ctx, ptrs[1:], u, d_vals, circ.pieces, challenges[0], num_values=nvals)
    PL.gate_fill_chains(ctx, [d_adv0[0], ptrs[0]], u, ptrs[1], u, d_adv0[0], u, gate_chains)
    ctx.sync()
    cb_ms.append((time.perf_counter() - t) * 1e3)


host_col = np.zeros((n, 4), dtype=np.uint64)


def on_host(phase, challenges, ptrs):
    t = time.perf_counter()
    PL.rlc_fill_chains(ctx, ptrs[1:], u, d_vals, circ.pieces, challenges[0], num_values=nvals)
    rlc_col = ctx.download(ptrs[1], (u, 4))
    cols = (_vp * 2)(None, _vp(host_col.ctypes.data))
    helper.gate_host_fill_chains(cols, _vp(rlc_col.ctypes.data), _vp(adv0[0].ctypes.data), C.cast(gate_chains, _vp), len(pieces))
    ctx.upload(ptrs[0], host_col[:u])
    ctx.sync()
    cb_ms.append((time.perf_counter() - t) * 1e3)


def prove(cb):
    return PL.create_proof(pk, d_adv0, [], PL.ChaChaRng(ctx.lib, 1234), advice_on_device=True, phase_witness_dev=cb)


ref = prove(on_device)
assert prove(on_host) == ref and PL.verify_proof(pk, [], ref), "the two witnesses give different proofs / the proof does not verify"
out = {"k": k, "pairs": pairs, "cells": cells, "device": [], "host": []}
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
d_col, d_rlc = ctx.to_device(host_col), ctx.to_device(host_col)
d_in, d_out = ctx.to_device(np.ascontiguousarray(values[:pairs])), ctx.malloc(32 * pairs)
PL.rlc_fill_chains(ctx, [d_rlc], u, d_vals, circ.pieces, 0x1234567890ABCDEF1234567890ABCDEF, num_values=nvals)


def timed(fn):
    ms = []
    for i in range(reps + 2):
        ctx.timer_start()
        fn()
        t = ctx.timer_stop()
        if i >= 2:
            ms.append(t)
    return float(np.median(ms))


fill_ms = timed(lambda: PL.gate_fill_chains(ctx, [d_adv0[0], d_col], u, d_rlc, u, d_adv0[0], u, gate_chains))
prod_ms = timed(lambda: ctx._chk(ctx.lib.h2hip_fr_prefix_product_dev(ctx.handle, _vp(d_out), _vp(d_in), pairs)))
out["fill_alone_ms"], out["fill_pairs_per_s"] = round(fill_ms, 4), round(pairs / fill_ms * 1e3)
out["prefix_product_ms"], out["prefix_product_elements_per_s"] = round(prod_ms, 4), round(pairs / prod_ms * 1e3)
print("fill alone: %.4f ms for %d pairs = %.3g pairs/s; h2hip_fr_prefix_product_dev: %.4f ms = %.3g elements/s" % (
    fill_ms, pairs, pairs / fill_ms * 1e3, prod_ms, pairs / prod_ms * 1e3), flush=True)
print(json.dumps(out))
for p in d_adv0 + [d_vals, d_col, d_rlc, d_in, d_out]:
    ctx.free(p)
pk.free()
kzg.free()
ctx.close()
