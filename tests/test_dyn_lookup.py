"""Proofs of circuits with a dynamic lookup table (BasicDynLookupConfig, reference halo2-base/src/virtual_region/lookups/basic.rs:38-199) on the
CPU: libh2hip's emulated build against the test prover (itself pinned by tests/test_shape_oracle.py), and the host mirror's layout."""
import ctypes as C

import numpy as np
import pytest

from halo2_lib_amd import plonk as PL
from halo2_lib_amd import virtual_region as V
from tests import shape_oracle as SO
from tests.dyn_lookup_util import PreDrawnRng, R, oracle_verify, prove_both, ram_circuit, rng_budget, oracle_shape, srs


def CO_ints(col):
    from oracle import bn254 as O

    return O.limbs_to_ints(np.ascontiguousarray(col, dtype=np.uint64).reshape(-1, 4), R)


# ---- 2. libh2hip (emulated build) against the test prover: memory.rs's mock shape at key_cols 1, 2, 3
@pytest.mark.parametrize("key_cols", [2, 1, 3])
def test_ram_circuit_proof_emulated(key_cols):
    from tests.emu_util import emu_context

    ctx = emu_context()
    try:
        gpk, kzg, params, vk, got, want, sh, advice = prove_both(ctx, 5, 50, 16, key_cols, 3, seed=key_cols)
        try:
            assert got == want, "proof bytes differ from the test prover's"
            if key_cols == 1:   # a timed run (a stream synchronisation per stage) of the same RNG stream gives the same bytes
                assert PL.create_proof(gpk, advice, [], PreDrawnRng(rng_budget(sh), 1000 + key_cols), {}) == got, "the timed proof differs"
            assert oracle_verify(params, vk, got), "the test verifier rejects the proof"
            assert PL.verify_proof(gpk, [], got), "h2hip_plonk_verify_proof_dyn rejects the proof"
            first_eval = 32 * (sh.num_advice_total + 3 * len(sh.lookups) + sh.num_perm_sets + 1 + sh.quotient_poly_degree)
            for pos in (0, 32 * sh.num_advice_total + 3, first_eval + 1, len(got) - 1):
                bad = bytearray(got)
                bad[pos] ^= 1
                assert not oracle_verify(params, vk, bytes(bad)), pos
                assert not PL.verify_proof(gpk, [], bytes(bad)), pos
        finally:
            gpk.free()
            kzg.free()
    finally:
        ctx.close()


# ---- 2b. a sort over several tiles: full-width theta-compressed keys, a table that fills the usable rows.  k = 11 pads to 2048 keys (two LDS
# tiles and one global stage); k = 12 to 4096 keys (four tiles, global stages in two merge steps, the first of them with descending halves), and
# with lookup_big_tile_bits = 12 to one 4096-key tile.  Proof bytes against the test prover's
@pytest.mark.parametrize("k,tile_bits", [(11, 19), (12, 19), (12, 12)])
def test_ram_circuit_multi_tile_sort_emulated(k, tile_bits):
    """measured: 4.6 s at k = 11 (1.5 s setup and keygen, 0.7 s emulated proof, 0.9 s + 1.1 s test-side keygen and proof, 0.4 s verifiers),
    5.4 s at k = 12 (2.3 s, 1.1 s, 0.8 s + 0.9 s, 0.3 s)"""
    from tests.emu_util import emu_context
    from tests.lookup_key_checks import MIN_TILE, padded_keys

    ctx = emu_context()
    try:
        ctx.set_param("lookup_big_tile_bits", tile_bits)
        gpk, kzg, params, vk, got, want, sh, _ = prove_both(ctx, k, 1 << k, (1 << k) - 9 - 2, 2, 2, seed=60 + k)
        try:
            assert padded_keys(sh.usable_rows) == (1 << k) >= 2 * MIN_TILE
            assert got == want, "proof bytes differ from the test prover's"
            assert oracle_verify(params, vk, got), "the test verifier rejects the proof"
            assert PL.verify_proof(gpk, [], got), "h2hip_plonk_verify_proof_dyn rejects the proof"
        finally:
            gpk.free()
            kzg.free()
    finally:
        ctx.close()


# ---- 3. a key missing from the table (memory.rs:160-182's prank) is an error; the context and key stay usable
def test_failed_access_is_an_error_emulated():
    from tests.emu_util import emu_context
    import halo2_lib_amd as H

    ctx = emu_context()
    try:
        circ, dp, advice, fixed, copies = ram_circuit(5, 50, 16, 2, 3, seed=11, prank=True)
        sh = oracle_shape(dp)
        kzg, params = srs(ctx, 5, 11)
        gpk = PL.keygen(kzg, dp, fixed, copies)
        try:
            with pytest.raises(H.H2HipError, match="missing from the table"):
                PL.create_proof(gpk, advice, [], PreDrawnRng(rng_budget(sh), 5))
            # the context serves the next proof: the honest circuit of the same shape, byte-equal to the test prover's and accepted
            gpk2, kzg2, params2, vk2, got, want, _, _ = prove_both(ctx, 5, 50, 16, 2, 3, seed=11)
            try:
                assert got == want and PL.verify_proof(gpk2, [], got) and oracle_verify(params2, vk2, got)
            finally:
                gpk2.free()
                kzg2.free()
        finally:
            gpk.free()
            kzg.free()
    finally:
        ctx.close()


# ---- 4. parameters the configuration does not support, and sharding
@pytest.mark.parametrize("bad", [(3, 1, 1, 2, 1), (5, 0, 1, 2, 1), (5, 1, 1, 0, 1), (5, 1, 1, 5, 1), (5, 1, 1, 2, 0), (5, 1, 1, 2, 49),
                                 (5, 1, 17, 2, 1), (27, 1, 1, 2, 1)])
def test_shape_of_dyn_refuses_unsupported_params(bad):
    import halo2_lib_amd as H

    lib = H.load_library()
    out = PL.ConstraintSystemShape()
    assert lib.h2hip_plonk_shape_of_dyn(C.byref(PL.DynLookupCircuitParams.new(*bad)), C.byref(out)) == -1   # H2HIP_ERR_INVALID


def test_shape_of_dyn_layout():
    import halo2_lib_amd as H

    lib = H.load_library()
    out = PL.ConstraintSystemShape()
    assert lib.h2hip_plonk_shape_of_dyn(C.byref(PL.DynLookupCircuitParams.new(10, 3, 1, 2, 2)), C.byref(out)) == 0
    # advice: 2 table + 2 x 2 key + 3 gate; fixed: table_is_enabled, 2 key_is_enabled, 1 constant, 3 q_enable
    assert (out.num_advice_total, out.num_fixed_total, out.table_col, out.q_lookup_col, out.first_constant_col, out.first_q_enable_col) == (9, 7, -1, -1, 3, 4)
    assert (out.num_lookups, out.num_perm_columns, out.degree, out.blinding_factors, out.usable_rows, out.quotient_pieces) == (2, 10, 4, 6, 1017, 3)
    sh = SO.Shape.dyn(10, 3, 1, 2, 2)
    assert out.num_perm_sets == sh.num_perm_sets and out.extended_k == sh.extended_k
    evals = len(sh.advice_queries) + len(sh.fixed_queries) + 1 + len(sh.perm_columns) + 3 * sh.num_perm_sets - 1 + 5 * len(sh.lookups)
    assert out.num_evals == evals


def test_sharding_a_dyn_key_is_refused_emulated():
    from tests.emu_util import emu_context

    ctx = emu_context()
    try:
        _, dp, advice, fixed, copies = ram_circuit(5, 10, 4, 2, 1, seed=3)
        kzg, _ = srs(ctx, 5, 3)
        gpk = PL.keygen(kzg, dp, fixed, copies)

        def _allgather(_user, local, nbytes, out):
            C.memmove(out, local, nbytes)
            return 0

        cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(_allgather)
        h = C.c_void_p()
        ctx._chk(ctx.lib.h2hip_comm_init_callback(1, 0, C.cast(cb, C.c_void_p), None, C.byref(h)))
        try:
            rc = ctx.lib.h2hip_plonk_pk_set_sharding(gpk.handle, h, kzg.g.handle, kzg.g_lagrange.handle, 0, 32, 0xFFFF)
            assert rc == -1 and b"one GPU" in ctx.lib.h2hip_last_error()
        finally:
            ctx.lib.h2hip_comm_destroy(h)
            gpk.free()
            kzg.free()
    finally:
        ctx.close()


def test_dyn_params_struct_layout_agrees():
    """h2hip_dyn_circuit_params: the same fields in the header, the Rust repr(C) struct and ctypes"""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "h2hip.h")).read()
    body = re.search(r"typedef struct h2hip_dyn_circuit_params\s*\{(.*?)\}\s*h2hip_dyn_circuit_params\s*;", hdr, flags=re.S).group(1)
    c_fields = re.findall(r"uint32_t\s+([a-z_]+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    rs = open(os.path.join(root, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    rs_body = re.search(r"pub struct h2hip_dyn_circuit_params\s*\{(.*?)\}", rs, flags=re.S).group(1)
    rs_fields = re.findall(r"pub ([a-z_]+): u32", rs_body)
    py_fields = [n for n, t in PL.DynLookupCircuitParams._fields_ if t is C.c_uint32]
    assert c_fields == rs_fields == py_fields == ["k", "num_advice", "num_fixed", "key_cols", "lu_sets"]


# ---- 5. the host mirror's placement (basic.rs:115-198)
def test_virtual_region_table_and_lookup_placement():
    cm = V.CopyConstraintManager()
    ctx = V.Context(False, V.FIRST_PHASE_TYPE_ID, 0, cm)
    region = V.Region(32, 2 * (1 + 2) + 1)
    keys = []
    for i in range(5):
        keys.append([ctx.load_witness(i), ctx.load_witness(100 + i)])
    V.assign_with_constraints([ctx], [6], region, cm, 23)
    cfg = V.BasicDynLookupConfig(2, 2)
    assert cfg.table == [0, 1] and cfg.to_lookup == [([2, 3], 1), ([4, 5], 2)] and cfg.table_is_enabled == 0
    rows = [[V.AssignedValue(i, V.ContextCell(V.EXTERNAL_CELL_TYPE_ID, 0, i)), V.AssignedValue(100 + i, V.ContextCell(V.EXTERNAL_CELL_TYPE_ID, 1, i))]
            for i in range(3)]
    cfg.assign_virtual_table_to_raw(region, rows, cm)
    # three enabled rows, then the disabled all-zero row
    assert region.fixed[0] == {0: 1, 1: 1, 2: 1, 3: 0}
    assert region.advice[0] == {0: 0, 1: 1, 2: 2, 3: 0} and region.advice[1] == {0: 100, 1: 101, 2: 102, 3: 0}
    # external table cells are registered, not copied
    assert not region.copies and cm.assigned_advices[rows[2][1].cell] == (("advice", 1), 2)
    cfg.assign_virtual_to_lookup_to_raw(region, keys, cm)
    # left to right over the sets, then down: keys 0, 1 on row 0; 2, 3 on row 1; 4 wraps to set 0 of row 2
    assert region.advice[2] == {0: 0, 1: 2, 2: 4} and region.advice[3] == {0: 100, 1: 102, 2: 104}
    assert region.advice[4] == {0: 1, 1: 3} and region.advice[5] == {0: 101, 1: 103}
    assert region.fixed[1] == {0: 1, 1: 1, 2: 1} and region.fixed[2] == {0: 1, 1: 1}
    # each key cell is constrained equal to its gate cell: (gate cell, lookup cell)
    assert region.copies[0] == ((("advice", 6), 0), (("advice", 2), 0))
    assert region.copies[-1] == ((("advice", 6), 9), (("advice", 3), 2))
    assert len(region.copies) == 10


def test_ram_circuit_synthesis():
    circ, dp, advice, fixed, copies = ram_circuit(5, 50, 16, 2, 3, seed=2)
    n, L = 32, 3
    assert len(advice) == 2 * (1 + L) + dp.num_advice and len(fixed) == 1 + L + 1 + dp.num_advice
    vals = lambda col: CO_ints(col)
    assert vals(fixed[0])[:17] == [1] * 16 + [0]
    assert vals(advice[0])[:17] == list(range(16)) + [0] and vals(advice[1])[:16] == circ.memory
    rows = -(-50 // L)
    for s in range(L):
        used = len(range(s, 50, L))
        assert vals(fixed[1 + s])[:rows] == [1] * used + [0] * (rows - used)
        assert vals(advice[2 * (1 + s)])[:used] == circ.ptrs[s::L]
        assert vals(advice[2 * (1 + s) + 1])[:used] == [circ.memory[p] for p in circ.ptrs[s::L]]
    # every copy names a permutation column of the layout
    pcols = set(oracle_shape(dp).perm_columns)
    assert all(l[0] in pcols and r[0] in pcols for l, r in copies)
    assert all(r < n - 7 and q < n - 7 for (_, r), (_, q) in copies)
