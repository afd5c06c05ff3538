"""One proof over a caller-supplied transcript next to the built-in entry.
Usage: python tools/transcript_time.py [k] [reps]     (defaults 19 7)

The benchmark's shape (one gate column with q_lookup, lookup_bits = k - 1), the advice column resident on the device, libh2hip's seeded
ChaCha generator: host clock around whole create_proof calls (each ends synchronised), two warm-up proofs, then the median of `reps`, for
  (a) the built-in Blake2b entry,
  (b) h2hip_plonk_create_proof_transcript over a PYTHON object: oracle/transcript.py's Blake2bWrite behind ctypes trampolines.
One JSON line at the end.  The same proof over a native C++ transcript: halo2-lib_amd/host/transcript_selftest <k> --time."""
import json
import os
import statistics
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
from oracle.transcript import Blake2bWrite  # noqa: E402

a = [int(v) for v in sys.argv[1:]]
k, reps = (a + [19, 7][len(a):])[:2]
ctx = H.Context()


class Backend:
    mul = staticmethod(ctx.fr_mul)
    add = staticmethod(ctx.fr_add)


sh = P.Shape(k, 1, 1, 1, 0, k - 1)
kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF, precompute=True)
circ = T.build_circuit(sh, 19, Backend)
pk = PL.keygen(kzg, PL.BaseCircuitParams.new(k, 1, 1, 1, 0, k - 1), circ.fixed, circ.copies)
adv = [ctx.to_device(np.ascontiguousarray(c)) for c in circ.advice]


def median_ms(prove):
    for _ in range(2):
        prove()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        prove()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


builtin = lambda: PL.create_proof(pk, adv, circ.instances, PL.ChaChaRng(ctx.lib, 0, 12), advice_on_device=True)
python_t1 = lambda: PL.create_proof(pk, adv, circ.instances, PL.ChaChaRng(ctx.lib, 0, 12), advice_on_device=True, transcript=Blake2bWrite())
assert builtin() == python_t1()
out = {"k": k, "reps": reps, "builtin_ms": round(median_ms(builtin), 3), "python_t1_ms": round(median_ms(python_t1), 3)}
for p in adv:
    ctx.free(p)
pk.free()
kzg.free()
ctx.close()
print(json.dumps(out))
