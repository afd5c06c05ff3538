"""Proofs with a dynamic lookup table (BasicDynLookupConfig) on the GPU: reference-sized RAM circuits against the test-side prover
(tests/shape_oracle.py), a table near the usable rows (the bitonic sort's global passes), the failed-access error, and a BaseConfig
proof before and after a dynamic one on the same context."""
import numpy as np
import pytest

from halo2_lib_amd import halo2_proofs as HP
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import testing as T
from tests.dyn_lookup_util import PreDrawnRng, oracle_shape, oracle_verify, prove_both, ram_circuit, rng_budget, srs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import halo2_lib_amd as H

    c = H.Context()
    yield c
    c.close()


def test_ram_prover_shape(ctx):
    """test_ram_prover (memory.rs:184-253): k = 10, 2000 accesses, 500 memory cells, 2 lookup sets"""
    gpk, kzg, params, vk, got, want, _, _ = prove_both(ctx, 10, 2000, 500, 2, 2, seed=21, threads=8)
    try:
        assert got == want, "proof bytes differ from the test prover's"
        assert PL.verify_proof(gpk, [], got) and oracle_verify(params, vk, got)
        bad = bytearray(got)
        bad[len(got) // 2] ^= 4
        assert not PL.verify_proof(gpk, [], bytes(bad))
    finally:
        gpk.free()
        kzg.free()


@pytest.mark.parametrize("k", [12, 13])
def test_multi_tile_sort_against_test_prover(ctx, k):
    """a table of 2^k - 11 rows and 2^k accesses over 2 lookup sets, 2 key columns: the theta-compressed keys are full-width, and their sort
    spans 4 (k = 12) and 8 (k = 13) LDS tiles with two and three merge steps of global stages.  Byte for byte against the test-side prover,
    whose time was measured on a CPU at 1.7 s (k = 12) and 2.7 s (k = 13) for keygen and proof together."""
    from tests.lookup_key_checks import MIN_TILE, padded_keys

    gpk, kzg, params, vk, got, want, sh, _ = prove_both(ctx, k, 1 << k, (1 << k) - 9 - 2, 2, 2, seed=60 + k, threads=8)
    try:
        assert padded_keys(sh.usable_rows) == (1 << k) >= 4 * MIN_TILE
        assert got == want, "proof bytes differ from the test prover's"
        assert PL.verify_proof(gpk, [], got) and oracle_verify(params, vk, got)
    finally:
        gpk.free()
        kzg.free()


def test_large_table_k17(ctx):
    """k = 17, a table of 2^17 - 11 rows (the last usable row holds the disabled zero row) and 4 lookup sets: the per-proof sort of the
    compressed table runs the bitonic network's global passes.  Verified by both verifiers; two proofs from one RNG stream are identical."""
    k, sets = 17, 4
    mem_len = (1 << k) - 9 - 2   # gate.max_rows = 2^k - 9; the table and its zero row must fit
    gpk, kzg, params, vk, got, _, sh, advice = prove_both(ctx, k, 60000, mem_len, 2, sets, seed=31, oracle_prover=False)
    try:
        assert PL.verify_proof(gpk, [], got) and oracle_verify(params, vk, got)
        again = PL.create_proof(gpk, advice, [], PreDrawnRng(rng_budget(sh), 1000 + 31))
        assert again == got
    finally:
        gpk.free()
        kzg.free()


def test_failed_access_is_an_error(ctx):
    import halo2_lib_amd as H

    circ, dp, advice, fixed, copies = ram_circuit(10, 2000, 500, 2, 2, seed=41, prank=True)
    sh = oracle_shape(dp)
    kzg, _ = srs(ctx, 10, 41)
    gpk = PL.keygen(kzg, dp, fixed, copies)
    try:
        with pytest.raises(H.H2HipError, match="missing from the table"):
            PL.create_proof(gpk, advice, [], PreDrawnRng(rng_budget(sh), 5))
        gpk2, kzg2, params2, vk2, got, want, _, _ = prove_both(ctx, 10, 2000, 500, 2, 2, seed=41, threads=8)
        try:
            assert got == want and PL.verify_proof(gpk2, [], got)
        finally:
            gpk2.free()
            kzg2.free()
    finally:
        gpk.free()
        kzg.free()


def test_base_config_k19_undisturbed_by_a_dyn_proof(ctx):
    """a BaseConfig k = 19 proof (one gate column, range lookups on it) before and after a dynamic-lookup proof on the same context: same bytes, verified"""
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
        gpk, kzg2, _, _, got, _, _, _ = prove_both(ctx, 10, 2000, 500, 2, 2, seed=51, oracle_prover=False)
        try:
            assert PL.verify_proof(gpk, [], got)
        finally:
            gpk.free()
            kzg2.free()
        after = PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(vals))
        assert after == before
    finally:
        pk.free()
        kzg.free()
