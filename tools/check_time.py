"""h2hip_plonk_check_witness time next to one create_proof of the same witness, advice resident on the device.
Usage: python tools/check_time.py [reps] [shape ...]   shapes: ecdsa19 pairing21 ecdsa11 dyn14 phased17 (default: all)
Per shape: the median of `reps` checks (after two warm-up calls; each timed call ends with the device synchronised, which the call does itself),
one create_proof of the same witness (after one warm-up proof), their ratio, and the failure count (0: the witnesses are honest).
Prints one JSON line per shape."""
import json
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
from oracle import plonk as P  # noqa: E402

TOXIC = 0x1D0C0FFEE1234567890ABCDEF
args = sys.argv[1:]
reps = int(args[0]) if args and args[0].isdigit() else 20
names = [a for a in args if not a.isdigit()] or ["ecdsa19", "pairing21", "ecdsa11", "dyn14", "phased17"]
ctx = H.Context()


class _Backend:
    mul = staticmethod(ctx.fr_mul)
    add = staticmethod(ctx.fr_add)


def base(k, na, nl, nf, ni, lb):
    kzg = HP.ParamsKZG.setup(ctx, k, TOXIC, precompute=True)
    sh = P.Shape(k, na, nl, nf, ni, lb)
    circ = T.build_circuit(sh, 5, _Backend)
    pk = PL.keygen(kzg, PL.BaseCircuitParams.new(k, na, nl, nf, ni, lb), circ.fixed, circ.copies)
    return kzg, pk, circ.advice, circ.instances, None


def dyn(k):
    from tests.dyn_lookup_util import ram_circuit

    _, dp, advice, fixed, copies = ram_circuit(k, (1 << k) // 2, 1 << (k - 3), 2, 2, seed=3)
    kzg = HP.ParamsKZG.setup(ctx, k, TOXIC, precompute=True)
    return kzg, PL.keygen(kzg, dp, fixed, copies), advice, [], None


def phased(k):
    from tests.phases_util import PhasedCircuit, shape_params

    params, _ = shape_params("a", k, k - 1)
    circ = PhasedCircuit(params, 7)
    kzg = HP.ParamsKZG.setup(ctx, k, TOXIC, precompute=True)
    pk = PL.keygen(kzg, params, circ.fixed, circ.copies)
    adv = [None] * circ.sh.num_advice_total
    for p, idx in enumerate(circ.phase_cols):
        for c, v in zip(idx, circ.witness(p, [11] * circ._ch_before(p))):
            adv[c] = v
    return kzg, pk, adv, [], circ


SHAPES = {"ecdsa19": lambda: base(19, 1, 1, 1, 0, 18), "pairing21": lambda: base(21, 2, 1, 1, 0, 20), "ecdsa11": lambda: base(11, 291, 53, 1, 0, 10),
          "dyn14": lambda: dyn(14), "phased17": lambda: phased(17)}

for name in names:
    kzg, pk, advice, instances, circ = SHAPES[name]()
    dev = [ctx.to_device(np.ascontiguousarray(c)) for c in advice]
    for _ in range(2):
        total, _f = PL.check_witness(pk, dev, instances, 16, advice_on_device=True)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        PL.check_witness(pk, dev, instances, 16, advice_on_device=True)
        ts.append(time.perf_counter() - t0)
    rng = lambda: PL.ChaChaRng(ctx.lib, 1)
    if circ is None:
        prove = lambda: PL.create_proof(pk, dev, instances, rng(), advice_on_device=True)
    else:   # phased: phase 0 on the device, the later phases from the host (the witness callback)
        p0 = [dev[c] for c in circ.phase_cols[0]]
        prove = lambda: PL.create_proof(pk, p0, instances, rng(), advice_on_device=True,
                                        phase_witness=lambda p, ch: [advice[c] for c in circ.phase_cols[p]])
    prove()
    ctx.sync()
    t0 = time.perf_counter()
    prove()
    ctx.sync()
    tp = time.perf_counter() - t0
    tc = float(np.median(ts))
    print(json.dumps({"shape": name, "k": pk.params.k, "advice_columns": pk.shape.num_advice_total, "failures": total,
                      "check_ms_median": round(tc * 1e3, 3), "check_ms_min": round(min(ts) * 1e3, 3), "create_proof_ms": round(tp * 1e3, 2),
                      "check_over_proof": round(tc / tp, 4)}), flush=True)
    for p in dev:
        ctx.free(p)
    pk.free()
    kzg.free()
ctx.close()
