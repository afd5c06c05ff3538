#!/usr/bin/env python3
"""Times verification of N proofs of one key on the GPU box: (a) N calls of the single verifier h2hip_plonk_verify_proof (host code, the
baseline) against (b) ONE h2hip_plonk_verify_batch, with (b)'s split into upload + decompress, host derive, MSM and pairing.

Shapes: the k = 12 two-column BaseConfig shape and the 70-column wide shape of tests/test_plonk_prover.py; N = 1, 8, 64.  Every timed call is
a host clock around a call that ends synchronised (both verifiers return a verdict).  One warm-up call per (shape, N, verifier), then `--reps`
timed repetitions with (a) and (b) alternating; the table gives the median and the min .. max spread.  The stage split comes from a separate
pass with the context's profile on (h2hip_plonk_verify_batch adds its stages' wall times to the profile), not from the timed calls.

usage: python tools/verify_batch_times.py [--reps 5] [--counts 1,8,64] [--out profiles/verify_batch_times.log]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"k12_two_columns": (12, 2, 1, 1, 1, 11), "k8_wide_70_columns": (8, 70, 34, 2, 1, 5)}
STAGES = ["upload_decompress", "derive", "msm", "pairing"]


def main():
    import halo2_lib_amd as H
    from halo2_lib_amd import halo2_proofs as HP
    from halo2_lib_amd import plonk as PL
    from halo2_lib_amd import testing as T
    from oracle import plonk as P

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", default="1,8,64")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_times.log"))
    args = ap.parse_args()
    counts = [int(v) for v in args.counts.split(",")]
    ctx = H.Context(device=0)

    class Backend:
        mul = staticmethod(ctx.fr_mul)
        add = staticmethod(ctx.fr_add)

    lines = ["# verify N proofs of one key: N x h2hip_plonk_verify_proof (host) vs one h2hip_plonk_verify_batch; ms, median of %d (min .. max)" % args.reps,
             "# stage columns: one profiled batch call, wall time per stage (they add up to that call, not to the median)",
             "%-20s %3s %6s | %24s | %24s | %6s | %8s %8s %8s %8s" % ("shape", "N", "points", "N singles", "one batch", "ratio", *STAGES)]
    for name in args.shapes.split(","):
        k, na, nl, nf, ni, lb = SHAPES[name]
        sh = P.Shape(k, na, nl, nf, ni, lb)
        kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF)
        circ = T.build_circuit(sh, 3, Backend)
        pk = PL.keygen(kzg, PL.BaseCircuitParams.new(k, na, nl, nf, ni, lb), circ.fixed, circ.copies)
        proofs = [PL.create_proof(pk, circ.advice, circ.instances, PL.ChaChaRng(ctx.lib, seed=100 + i)) for i in range(max(counts))]
        points = pk.shape.num_commitments
        for count in counts:
            insts, batch = [circ.instances] * count, proofs[:count]
            rho = lambda: PL.ChaChaRng(ctx.lib, seed=7, device=False)

            def singles():
                t0 = time.perf_counter()
                ok = all(PL.verify_proof(pk, circ.instances, p) for p in batch)
                return ok, (time.perf_counter() - t0) * 1e3

            def one_batch():
                t0 = time.perf_counter()
                ok = PL.verify_proofs(pk, insts, batch, rho())
                return ok, (time.perf_counter() - t0) * 1e3

            assert singles()[0] and one_batch()[0], "a proof does not verify"   # warm-up, and the verdicts
            ta, tb = [], []
            for _ in range(args.reps):
                ta.append(singles()[1])
                tb.append(one_batch()[1])
            ctx.profile_reset()
            ctx.profile_enable(True)
            assert one_batch()[0]
            stage = [ctx.profile_get("verify_batch_stage:" + s)[0] for s in STAGES]
            ctx.profile_enable(False)
            fmt = lambda t: "%8.2f (%7.2f ..%8.2f)" % (statistics.median(t), min(t), max(t))
            lines.append("%-20s %3d %6d | %s | %s | %6.2f | %8.2f %8.2f %8.2f %8.2f" % (
                name, count, count * points, fmt(ta), fmt(tb), statistics.median(ta) / statistics.median(tb), *stage))
            print(lines[-1], flush=True)
        pk.free()
        kzg.free()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
