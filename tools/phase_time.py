"""create_proof time of a multi-phase BaseConfig circuit against the single-phase BaseConfig with the same gate / lookup-advice column counts:
[1,1] gate columns / [1,1] lookup-advice columns with one challenge after phase 0 (tests/phases_util.py's RLC circuit) against 2 gate + 2
lookup-advice columns.  Usage: python tools/phase_time.py [k] [reps] [lookup_bits]
Prints the median proof time of each, the per-stage laps of one proof of each, and the MSM kernels' launches per proof (profiled run).
The later phase's witness is synthesised once (Python) and handed over again on every proof: its upload is timed, its synthesis is not."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_lib_amd as H  # noqa: E402
from halo2_lib_amd import halo2_proofs as HP  # noqa: E402
from halo2_lib_amd import plonk as PL  # noqa: E402
from halo2_lib_amd import testing as T  # noqa: E402
from tests.phases_util import PhasedCircuit  # noqa: E402

a = [int(v) for v in sys.argv[1:]]
k, reps, lb = (a + [17, 7, 16][len(a):])[:3]
ctx = H.Context()
kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF, precompute=True)


class _Backend:
    mul = staticmethod(ctx.fr_mul)
    add = staticmethod(ctx.fr_add)


class _ShapeView:
    pass


def base_circuit():
    bp = PL.BaseCircuitParams.new(k, 2, 2, 1, 0, lb)
    sh = PL.shape_of(ctx, bp)
    sv = _ShapeView()
    sv.k, sv.n, sv.usable_rows, sv.num_advice, sv.lookup_bits = k, 1 << k, sh.usable_rows, 2, lb
    sv.gate_advice, sv.lookup_advice = [0, 1], list(range(2, sh.num_advice_total))
    sv.table_col, sv.q_lookup_col = sh.table_col, sh.q_lookup_col
    sv.constant_cols = [sh.first_constant_col]
    sv.q_enable_cols = [sh.first_q_enable_col, sh.first_q_enable_col + 1]
    sv.num_fixed_total, sv.num_instance = sh.num_fixed_total, 0
    circ = T.build_circuit(sv, 5, _Backend)
    return PL.keygen(kzg, bp, circ.fixed, circ.copies), circ.advice, None


def phased_circuit():
    pp = PL.PhasedCircuitParams.new(k, [1, 1], [1, 1], 1, 0, lb, [1])
    circ = PhasedCircuit(pp, 5)
    cache = {}

    def witness(phase, challenges):   # the circuit's own synthesis (Python) is not the prover's time: one per challenge, then reused
        key = (phase, tuple(challenges))
        if key not in cache:
            cache[key] = [np.ascontiguousarray(c) for c in circ.witness(phase, challenges)]
        return cache[key]

    return PL.keygen(kzg, pp, circ.fixed, circ.copies), circ.advice0(), witness


def run(name, make):
    t = time.time()
    pk, advice, witness = make()
    print("%s: %d advice columns, %d lookups; circuit + keygen %.1f s" % (name, pk.shape.num_advice_total, pk.shape.num_lookups, time.time() - t), flush=True)
    times, proof = [], None
    for rep in range(-1, reps):   # rep -1: warm-up (and the phase witness of this RNG stream's challenge)
        rng = PL.ChaChaRng(ctx.lib, 1234)
        t = time.time()
        proof = PL.create_proof(pk, advice, [], rng, phase_witness=witness) if witness else PL.create_proof(pk, advice, [], rng)
        if rep >= 0:
            times.append((time.time() - t) * 1e3)
    print("  create_proof: median %.2f ms over %d proofs (min %.2f, max %.2f)" % (float(np.median(times)), reps, min(times), max(times)), flush=True)
    tm = {}
    rng = PL.ChaChaRng(ctx.lib, 1234)
    again = PL.create_proof(pk, advice, [], rng, tm, phase_witness=witness) if witness else PL.create_proof(pk, advice, [], rng, tm)
    assert again == proof and PL.verify_proof(pk, [], proof), "the proof does not verify / is not reproducible"
    for st, ms in tm.items():
        print("    %-48s %8.2f ms" % (st, ms))
    ctx.profile_reset()
    ctx.profile_enable(True)
    rng = PL.ChaChaRng(ctx.lib, 1234)
    PL.create_proof(pk, advice, [], rng, phase_witness=witness) if witness else PL.create_proof(pk, advice, [], rng)
    ctx.profile_enable(False)
    prof = ctx.profile_dump()
    for kname in sorted(prof):
        if "msm" in kname.lower():
            print("    launches per proof: %-40s %5d" % (kname, prof[kname][1]))
    pk.free()
    return float(np.median(times))


base = run("BaseConfig 2 gate + 2 lookup-advice columns", base_circuit)
ph = run("two phases [1,1] / [1,1], one challenge", phased_circuit)
print("k=%d: multi-phase %.2f ms, BaseConfig %.2f ms, difference %+.2f ms" % (k, ph, base, ph - base))
kzg.free()
ctx.close()
