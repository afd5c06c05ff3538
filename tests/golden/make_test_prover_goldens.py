"""Generator of tests/golden/test_prover_proof_digests.json (TEST INFRASTRUCTURE; CPU only, no GPU library is loaded).

The test-side CPU prover (tests/shape_oracle.py) replaced three provers, one per circuit kind, each a copy of the one before it with a few
lines changed.  This file recorded what those three computed, at the commit the JSON names, before they were deleted: for every case below

    sha256(proof), len(proof), vk.transcript_repr

from a CPU-made SRS (P.Params.setup), the circuits the proof tests use and a pre-drawn RNG stream.  It now runs the cases through the one
prover, and rerunning it reproduces the file byte for byte; tests/test_shape_oracle.py recomputes every case and compares.

  dyn     ram_circuit(5, 50, 16, key_cols, 3, seed = key_cols), key_cols = 1, 2, 3 (test_ram_circuit_proof_emulated's arguments)
  phased  shapes a .. e of phases_util.SHAPES at k = 6, lookup_bits 4 (e with its instance column).  Shape a with these seeds is the case on
          which the RLC prover was asserted byte-equal to the multi-phase prover when both existed: its digest records that reduction
  rlc     rlc_checks.shape_a, shape_b at k = 6, lookup_bits 4

usage (from the repo root): python tests/golden/make_test_prover_goldens.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import plonk as P                                     # noqa: E402
from tests import shape_oracle as SO                              # noqa: E402
from tests.dyn_lookup_util import oracle_pk, oracle_shape, ram_circuit, rng_budget   # noqa: E402
from tests.util import PreDrawnRng                                # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "test_prover_proof_digests.json")
MADE_AT = "76497df"   # the last commit with the three provers: the digests are theirs
TOXIC_S = 0xBEEF12345   # + k
K, LOOKUP_BITS, CIRCUIT_SEED, RNG_SEED, THREADS = 6, 4, 17, 4, 2
DYN = dict(k=5, accesses=50, mem_len=16, lu_sets=3)   # circuit seed = key_cols, rng seed = 1000 + key_cols


def case_names():
    return ["dyn-%d" % m for m in (1, 2, 3)] + ["phased-%s" % s for s in "abcde"] + ["rlc-a", "rlc-b"]


def build_case(name):
    """-> (k, shape, fixed, copies, phase-0 advice, instances, phase_witness, seeds)"""
    kind, which = name.split("-")
    if kind == "dyn":
        m = int(which)
        _, dp, advice, fixed, copies = ram_circuit(DYN["k"], DYN["accesses"], DYN["mem_len"], m, DYN["lu_sets"], seed=m)
        return DYN["k"], oracle_shape(dp), fixed, copies, advice, [], None, dict(circuit_seed=m, rng_seed=1000 + m)
    if kind == "phased":
        from tests import phases_util as PU

        params, inst = PU.shape_params(which, K, LOOKUP_BITS)
        circ = PU.PhasedCircuit(params, CIRCUIT_SEED, instance=inst)
    else:
        from tests import rlc_checks as RC

        params, inst = (RC.shape_a if which == "a" else RC.shape_b)(K, LOOKUP_BITS)
        circ = RC.RlcCircuit(params, CIRCUIT_SEED, instance=inst)
    return K, circ.sh, circ.fixed, circ.copies, circ.advice0(), circ.instances, circ.witness, dict(circuit_seed=CIRCUIT_SEED, rng_seed=RNG_SEED)


def prove_case(name):
    """-> (SRS, verifying key, instances, proof, the fixture's record)"""
    k, sh, fixed, copies, advice, instances, witness, seeds = build_case(name)
    sp = P.Params.setup(k, TOXIC_S + k)
    pk = oracle_pk(sh, sp, fixed, copies, THREADS)
    proof = SO.create_proof(sp, pk, advice, instances, PreDrawnRng(rng_budget(sh), seeds["rng_seed"]), THREADS, phase_witness=witness)
    rec = dict(seeds, k=k, toxic_s=hex(TOXIC_S + k), proof_sha256=hashlib.sha256(proof).hexdigest(), proof_len=len(proof),
               transcript_repr=hex(pk.vk.transcript_repr))
    return sp, pk.vk, instances, proof, rec


def main():
    doc = {"what": "proof digests of the three test-side CPU provers that stood under tests/ at made_at, one per circuit kind (dyn-*: dynamic "
                   "lookup, phased-*: multi-phase, rlc-*: RLC), which tests/shape_oracle.py replaced; generator: "
                   "tests/golden/make_test_prover_goldens.py",
           "made_at": MADE_AT, "lookup_bits": LOOKUP_BITS, "threads": THREADS, "cases": {}}
    for name in case_names():
        sp, vk, instances, proof, rec = prove_case(name)
        assert SO.verify_proof(sp, vk, instances, proof), name
        doc["cases"][name] = rec
        print("%s: %d bytes" % (name, len(proof)), flush=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
