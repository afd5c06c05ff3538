"""create_proof time of a circuit with a dynamic lookup table (BasicDynLookupConfig): a RAMCircuit (halo2_lib_amd.virtual_region) whose memory
table fills the usable rows, `lu_sets` lookup sets, 2^k accesses.  Usage: python tools/dyn_lookup_time.py [k] [reps] [lu_sets] [key_cols]
Prints the proof time per repetition and the per-stage laps of the last one."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import halo2_lib_amd as H  # noqa: E402
from halo2_lib_amd import halo2_proofs as HP  # noqa: E402
from halo2_lib_amd import plonk as PL  # noqa: E402
from halo2_lib_amd import virtual_region as V  # noqa: E402

a = [int(v) for v in sys.argv[1:]]
k, reps, sets, key_cols = (a + [17, 5, 4, 2][len(a):])[:4]
ctx = H.Context()
t = time.time()
g = np.random.default_rng(7)
mem_len = (1 << k) - 9 - 2
memory = [int(v) for v in g.integers(1, 2**62, size=mem_len)]
ptrs = [int(v) for v in g.integers(0, mem_len, size=1 << k)]
circ = V.RAMCircuit(memory, ptrs, key_cols)
dp = PL.DynLookupCircuitParams.new(k, circ.num_advice_needed(k), 1, key_cols, sets)
advice, fixed, copies = circ.synthesize(dp)
print("k=%d table=%d accesses=%d lu_sets=%d key_cols=%d gate columns=%d: circuit %.1f s" % (k, mem_len, len(ptrs), sets, key_cols, dp.num_advice,
                                                                                          time.time() - t), flush=True)
kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF, precompute=True)
t = time.time()
pk = PL.keygen(kzg, dp, fixed, copies)
print("keygen %.2f s" % (time.time() - t), flush=True)
vals = g.integers(0, 2**63, size=((1 << k) + 4096 * (1 + sets), 4), dtype=np.uint64)
vals[:, 3] &= np.uint64((1 << 60) - 1)
times = []
for rep in range(reps):
    tm = {} if rep == reps - 1 else None
    t = time.time()
    proof = PL.create_proof(pk, advice, [], PL.ArrayRng(vals), tm)
    times.append((time.time() - t) * 1e3)
    print("create_proof rep %d: %.2f ms (%d bytes)" % (rep, times[-1], len(proof)), flush=True)
print("median %.2f ms over %d proofs (the last one with per-stage laps: synchronising, slower)" % (float(np.median(times[:-1] or times)), len(times)))
for name, ms in tm.items():
    print("  %-48s %8.2f ms" % (name, ms))
assert PL.verify_proof(pk, [], proof), "the proof does not verify"
print("verified")
# the per-proof table sort alone (h2hip_lookup_table_sort_dev): the compressed table is a full-width field element per row, so the sort takes the
# 256-bit bitonic network (a range table's small keys take the counting sort instead)
u = pk.shape.usable_rows
col = g.integers(0, 2**63, size=(1 << k, 4), dtype=np.uint64)
col[:, 3] &= np.uint64((1 << 60) - 1)
dcol, dsorted = ctx.to_device(col), ctx.malloc(ctx.lib.h2hip_lookup_sorted_table_bytes(u))
sort_ms = []
for _ in range(6):
    ctx.sync()
    t = time.time()
    ctx._chk(ctx.lib.h2hip_lookup_table_sort_dev(ctx.handle, dcol, u, dsorted))
    ctx.sync()
    sort_ms.append((time.time() - t) * 1e3)
print("table sort (%d rows, 256-bit keys): median %.2f ms over %d (first %.2f ms)" % (u, float(np.median(sort_ms[1:])), len(sort_ms) - 1, sort_ms[0]))
ctx.free(dcol)
ctx.free(dsorted)
pk.free()
kzg.free()
ctx.close()
