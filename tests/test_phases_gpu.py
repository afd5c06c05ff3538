"""Multi-phase BaseConfig proofs on the GPU: shape (a) at k = 10 against the test-side prover (tests/shape_oracle.py) with phase-0 advice on
the host and on the device and later phases written by h2hip_upload and from a device tensor, a k = 17 two-phase circuit with range lookups
in both phases, and a BaseConfig k = 19 proof before and after multi-phase proofs on the same context."""
import numpy as np
import pytest

from halo2_lib_amd import halo2_proofs as HP
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import testing as T
from tests.dyn_lookup_util import rng_budget, srs
from tests.phases_util import PhasedCircuit, PreDrawnRng, first_phase1_commitment, oracle_verify, prove_both, shape_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import halo2_lib_amd as H

    c = H.Context()
    yield c
    c.close()


def test_shape_a_k10_host_and_device_advice(ctx):
    import torch

    params, _ = shape_params("a", 10, 8)
    r = prove_both(ctx, params, seed=61, threads=8)
    gpk, circ, want = r["gpk"], r["circ"], r["want"]
    dev = []
    try:
        assert r["got"] == want, "proof bytes differ from the test prover's (host advice)"
        assert PL.verify_proof(gpk, [], want) and oracle_verify(r["params"], r["vk"], [], want)
        bad = bytearray(want)
        bad[first_phase1_commitment(circ) + 5] ^= 2
        assert not PL.verify_proof(gpk, [], bytes(bad)) and not oracle_verify(r["params"], r["vk"], [], bytes(bad))
        # phase 0 on the device; phase 1 through h2hip_upload (host arrays) ...
        dev = [ctx.to_device(np.ascontiguousarray(c)) for c in circ.advice0()]
        budget = r["budget"]
        got = PL.create_proof(gpk, dev, [], PreDrawnRng(budget, 1000 + 61), advice_on_device=True, phase_witness=circ.witness)
        assert got == want, "device advice, host phase-1 witness"
        # ... and from torch tensors on the device
        keep = []

        def from_torch(phase, challenges):
            cols = circ.witness(phase, challenges)
            ts = [torch.from_numpy(np.ascontiguousarray(c).view(np.int64)).to("cuda:0") for c in cols]
            torch.cuda.synchronize()
            keep.extend(ts)
            return [t.data_ptr() for t in ts]

        got = PL.create_proof(gpk, dev, [], PreDrawnRng(budget, 1000 + 61), advice_on_device=True, phase_witness=from_torch)
        assert got == want, "device advice, device phase-1 witness"
        assert keep, "the witness callback did not run"
    finally:
        for p in dev:
            ctx.free(p)
        gpk.free()
        r["kzg"].free()


def test_two_phases_k17(ctx):
    """k = 17, [4,2] gate / [1,1] lookup-advice columns, lookup_bits 16: verified by both verifiers, reproducible from one RNG stream"""
    params = PL.PhasedCircuitParams.new(17, [4, 2], [1, 1], 1, 0, 16, [1])
    r = prove_both(ctx, params, seed=71, oracle_prover=False)
    gpk, circ = r["gpk"], r["circ"]
    try:
        got = r["got"]
        assert PL.verify_proof(gpk, [], got) and oracle_verify(r["params"], r["vk"], [], got)
        again = PL.create_proof(gpk, circ.advice0(), [], PreDrawnRng(r["budget"], 1000 + 71), phase_witness=circ.witness)
        assert again == got
    finally:
        gpk.free()
        r["kzg"].free()


def test_base_config_k19_undisturbed_by_phased_proofs(ctx):
    """a BaseConfig k = 19 proof before and after multi-phase proofs (one failing in its callback) on the same context: same bytes, verified"""
    k, na, nl, nf, lb = 19, 1, 1, 1, 18

    class Backend:
        mul = staticmethod(ctx.fr_mul)
        add = staticmethod(ctx.fr_add)

    class ShapeView:
        pass

    bp = PL.BaseCircuitParams.new(k, na, nl, nf, 0, lb)
    sh = PL.shape_of(ctx, bp)
    sv = ShapeView()
    sv.k, sv.n, sv.usable_rows, sv.num_advice, sv.lookup_bits = k, 1 << k, sh.usable_rows, na, lb
    sv.gate_advice, sv.lookup_advice = [0], list(range(na, sh.num_advice_total))
    sv.table_col, sv.q_lookup_col = sh.table_col, sh.q_lookup_col
    sv.constant_cols = [sh.first_constant_col]
    sv.q_enable_cols = [sh.first_q_enable_col]
    sv.num_fixed_total, sv.num_instance = sh.num_fixed_total, 0
    circ = T.build_circuit(sv, 5, Backend)
    kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF)
    pk = PL.keygen(kzg, bp, circ.fixed, circ.copies)
    g = np.random.default_rng(1)
    vals = g.integers(0, 2**63, size=((1 << k) + 4096, 4), dtype=np.uint64)
    vals[:, 3] &= np.uint64((1 << 60) - 1)
    try:
        before = PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(vals))
        assert PL.verify_proof(pk, circ.instances, before)
        params, _ = shape_params("c", 10, 8)
        r = prove_both(ctx, params, seed=81, oracle_prover=False)
        try:
            assert PL.verify_proof(r["gpk"], [], r["got"])

            def fail(_p, _c):
                raise RuntimeError("witness unavailable")

            with pytest.raises(RuntimeError, match="witness unavailable"):
                PL.create_proof(r["gpk"], r["circ"].advice0(), [], PreDrawnRng(r["budget"], 3), phase_witness=fail)
        finally:
            r["gpk"].free()
            r["kzg"].free()
        after = PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(vals))
        assert after == before
    finally:
        pk.free()
        kzg.free()
