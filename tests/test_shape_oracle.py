"""The test-side CPU prover and verifier (tests/shape_oracle.py) pinned on the CPU: against the established oracle on BaseConfig shapes, and
against the recorded digests of the three per-kind provers it replaced (tests/golden/test_prover_proof_digests.json, generator
tests/golden/make_test_prover_goldens.py) on dynamic-lookup, multi-phase and RLC circuits."""
import hashlib
import json
import os

import numpy as np
import pytest

from halo2_lib_amd import testing as T
from oracle import bn254 as O
from oracle import c_oracle as CO
from oracle import plonk as P
from tests import shape_oracle as SO
from tests.dyn_lookup_util import rng_budget
from tests.golden import make_test_prover_goldens as M
from tests.util import PreDrawnRng, R


class _OracleBackend:
    mul = staticmethod(CO.fr_mul)
    add = staticmethod(CO.fr_add)


# ---- 1. the test prover is the oracle for BaseConfig shapes (the shapes tests/test_dyn_lookup.py and tests/test_phases.py both listed)
@pytest.mark.parametrize("shape", [(6, 1, 0, 1, 0, None), (6, 1, 1, 1, 0, 4), (7, 2, 1, 1, 1, 5), (5, 6, 4, 1, 1, 3)],
                         ids=["no_lookups", "q_lookup", "lookup_advice", "k5_wide"])
def test_test_prover_reproduces_oracle_on_base_shapes(shape):
    k = shape[0]
    sh = P.Shape(*shape)
    params = P.Params.setup(k, 0xABCDEF12345 + k)
    circ = T.build_circuit(sh, 5, _OracleBackend)
    asm = P.PermutationAssembly(sh)
    for l, r in circ.copies:
        asm.copy(l, r)
    pk = P.keygen(params, sh, circ.fixed, asm, 2)
    inst = [O.limbs_to_ints(np.ascontiguousarray(c, dtype=np.uint64).reshape(-1, 4), R) for c in circ.instances]
    budget = rng_budget(sh)
    want = P.create_proof(params, pk, circ.advice, inst, PreDrawnRng(budget, 77), 2)
    pk.vk.shape = SO.Shape.from_base(sh)
    got = SO.create_proof(params, pk, circ.advice, inst, PreDrawnRng(budget, 77), 2)
    assert got == want
    assert SO.verify_proof(params, pk.vk, inst, got)


# ---- 2. the one prover computes what the three per-kind provers computed
@pytest.mark.parametrize("name", M.case_names())
def test_test_prover_reproduces_the_recorded_digests(name):
    """Recomputes a case of the fixture and compares sha256(proof), len(proof) and vk.transcript_repr; the verifier accepts the proof and
    rejects it with one bit of the first commitment flipped.  Case phased-a replaces the test of tests/test_rlc.py (and its check in tests/rlc_checks.py) that pinned the RLC prover to the multi-phase
    prover: it asserted, on this circuit and these seeds, that the RLC prover without RLC gates gave the multi-phase prover's bytes, so the
    one recorded digest is both provers'."""
    doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_prover_proof_digests.json")))
    assert sorted(doc["cases"]) == sorted(M.case_names())
    sp, vk, instances, proof, rec = M.prove_case(name)
    assert rec == doc["cases"][name]
    assert (hashlib.sha256(proof).hexdigest(), len(proof), hex(vk.transcript_repr)) == tuple(doc["cases"][name][f] for f in ("proof_sha256", "proof_len", "transcript_repr"))
    assert SO.verify_proof(sp, vk, instances, proof), "the test verifier rejects the proof"
    bad = bytearray(proof)
    bad[3] ^= 1
    assert not SO.oracle_verify(sp, vk, instances, bytes(bad)), "the test verifier accepts a flipped bit in the first commitment"
