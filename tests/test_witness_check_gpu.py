"""h2hip_plonk_check_witness on the GPU: the k = 19 ECDSA shape (host and device advice, one prank of each kind with the failures derived
locally from the pranked cell), the k = 11 ECDSA shape (291 + 53 advice columns), dynamic-lookup and multi-phase keys at k = 10 against the
test-side checker (tests/witness_check_oracle.py), and a k = 19 proof on the same context and key equal to its committed golden digest."""
import hashlib
import json
import os
from collections import defaultdict

import numpy as np
import pytest

from halo2_lib_amd import halo2_proofs as HP
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import testing as T
from oracle import bn254 as O
from oracle import plonk as P
from tests import witness_check_oracle as W
from tests import witness_edge_checks as WE
from tests.dyn_lookup_util import oracle_shape, ram_circuit, srs
from tests.golden import make_proof_goldens as M
from tests.phases_util import PhasedCircuit, shape_params
from tests.util import PreDrawnRng, R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_shapes_proof_digests.json")


@pytest.fixture(scope="module")
def ctx():
    import halo2_lib_amd as H

    c = H.Context()
    yield c
    c.close()


class _GpuBackend:
    def __init__(self, ctx):
        self.mul, self.add = ctx.fr_mul, ctx.fr_add


def _tuples(fails):
    kinds = {"gate": W.GATE, "lookup": W.LOOKUP, "copy": W.COPY}
    return [(kinds[f.kind], f.column, f.row, f.peer_column, f.peer_row) for f in fails]


def _with(col, row, v):
    col = np.array(col)
    col[row] = O.ints_to_limbs([v % R], R)[0]
    return col


def _local_expectation(sh, circ, advice, col, row):
    """the gate and lookup failures one changed cell (advice `col`, `row`) can cause — gates at rows row-3 .. row of its column, its own lookup
    row — and the component of its copy cycle (cells joined to it by the copy constraints)"""
    u = sh.usable_rows
    val = lambda c, r: O.limbs_to_ints(advice[c][r : r + 1], R)[0]
    fix = lambda c, r: O.limbs_to_ints(circ.fixed[c][r : r + 1], R)[0]
    out = []
    for q_col, a_col in sh.gates:
        if a_col != col:
            continue
        for s in range(max(row - 3, 0), row + 1):
            q = fix(q_col, s)
            if q and (s + 3 >= u or q * (val(col, s) + val(col, s + 1) * val(col, s + 2) - val(col, s + 3)) % R):
                out.append((W.GATE, col, s, 0, 0))
    for li, (q, a, _t) in enumerate(sh.lookups):
        if a == col:
            x = val(col, row) * (fix(q, row) if q is not None else 1) % R
            if x >= 1 << sh.lookup_bits:
                out.append((W.LOOKUP, li, row, 0, 0))
    adj = defaultdict(set)
    for l, r in circ.copies:
        adj[(l[0], l[1])].add((r[0], r[1]))
        adj[(r[0], r[1])].add((l[0], l[1]))
    comp, todo = set(), [(("advice", col), row)]
    while todo:
        c = todo.pop()
        if c not in comp:
            comp.add(c)
            todo.extend(adj[c])
    pidx = {c: i for i, c in enumerate(sh.perm_columns)}
    return out, {(pidx[c], r) for c, r in comp}, (sh.perm_columns.index(("advice", col)), row)


def _check_prank(pk, sh, circ, advice, col, row, value):
    adv = list(advice)
    adv[col] = _with(adv[col], row, value)
    total, fails = PL.check_witness(pk, adv, circ.instances, 64)
    got = _tuples(fails)
    want_gl, comp, cell = _local_expectation(sh, circ, adv, col, row)
    assert [f for f in got if f[0] != W.COPY] == want_gl
    copies = [f for f in got if f[0] == W.COPY]
    if len(comp) > 1:   # the cell disagrees with its successor, its predecessor with it
        assert len(copies) == 2 and copies == sorted(copies, key=lambda f: (f[1], f[2]))
        assert any((f[1], f[2]) == cell for f in copies) and any((f[3], f[4]) == cell for f in copies)
        assert all({(f[1], f[2]), (f[3], f[4])} <= comp for f in copies)
    else:
        assert copies == []
    assert total == len(got)
    return got


def test_k19_ecdsa_honest_pranks_then_golden_proof(ctx):
    e = json.load(open(GOLDEN))["shapes"]["ecdsa-19"]
    k, na, nl, nf, ni, lb = (e[f] for f in ("k", "num_advice", "num_lookup_advice", "num_fixed", "num_instance", "lookup_bits"))
    kzg = HP.ParamsKZG.setup(ctx, k, M.TOXIC_S, precompute=True)
    sh = P.Shape(k, na, nl, nf, ni, lb)
    circ = T.build_circuit(sh, M.CIRCUIT_SEED + k, _GpuBackend(ctx))
    pk = PL.keygen(kzg, PL.BaseCircuitParams.new(k, na, nl, nf, ni, lb), circ.fixed, circ.copies)
    dev = []
    try:
        assert PL.check_witness(pk, circ.advice, circ.instances) == (0, [])
        dev = [ctx.to_device(np.ascontiguousarray(c)) for c in circ.advice]
        assert PL.check_witness(pk, dev, circ.instances, advice_on_device=True) == (0, [])
        copied = sorted({l[1] for l, _ in circ.copies if l[0] == ("advice", 0)} | {r[1] for _, r in circ.copies if r[0] == ("advice", 0)})
        q_rows = np.flatnonzero(O.limbs_to_ints(circ.fixed[sh.q_lookup_col][:1 << 12], R))
        gate = _check_prank(pk, sh, circ, circ.advice, 0, 300001, 12345)                           # a gate cell
        assert any(f[0] == W.GATE for f in gate)
        lk_row = int(q_rows[len(q_rows) // 2])
        lk = _check_prank(pk, sh, circ, circ.advice, 0, lk_row, 1 << 40)                          # an input outside the table
        assert any(f[0] == W.LOOKUP for f in lk)
        cp = _check_prank(pk, sh, circ, circ.advice, 0, copied[len(copied) // 2], 99)             # a copied cell
        assert any(f[0] == W.COPY for f in cp)
        # the same context and key still prove the committed bytes
        proof = PL.create_proof(pk, circ.advice, circ.instances, PreDrawnRng(M.rng_budget(sh), M.RNG_SEED + k))
        assert (len(proof), hashlib.sha256(proof).hexdigest()) == (e["proof_len"], e["proof_sha256"])
    finally:
        for p in dev:
            ctx.free(p)
        pk.free()
        kzg.free()


def test_k11_ecdsa_wide_shape(ctx):
    k, na, nl, nf, ni, lb = 11, 291, 53, 1, 0, 10
    kzg = HP.ParamsKZG.setup(ctx, k, M.TOXIC_S, precompute=False)
    sh = P.Shape(k, na, nl, nf, ni, lb)
    circ = T.build_circuit(sh, M.CIRCUIT_SEED + k, _GpuBackend(ctx))
    pk = PL.keygen(kzg, PL.BaseCircuitParams.new(k, na, nl, nf, ni, lb), circ.fixed, circ.copies)
    try:
        assert sh.num_advice_total == 344 and PL.check_witness(pk, circ.advice, []) == (0, [])
        adv = list(circ.advice)
        adv[200] = _with(adv[200], 1001, 77777)              # a gate column far from the first
        adv[na + 40] = _with(adv[na + 40], 17, 1 << 11)      # a lookup-advice column: outside the 2^10 table
        want = W.check(sh, circ.fixed, adv, [], circ.copies)
        assert want[0] > 0 and any(f[0] == W.LOOKUP and f[1] == 40 for f in want[1])
        total, fails = PL.check_witness(pk, adv, [], 4096)
        assert (total, _tuples(fails)) == want
    finally:
        pk.free()
        kzg.free()


def test_dyn_k10_against_oracle(ctx):
    for prank in (False, True):
        circ, dp, advice, fixed, copies = ram_circuit(10, 2000, 500, 2, 2, seed=41, prank=prank)
        kzg, _ = srs(ctx, 10, 41)
        pk = PL.keygen(kzg, dp, fixed, copies)
        try:
            want = W.check(oracle_shape(dp), fixed, advice, [], copies)
            assert (want[0] > 0) == prank
            total, fails = PL.check_witness(pk, advice, [], 4096)
            assert (total, _tuples(fails)) == want
        finally:
            pk.free()
            kzg.free()


def test_phased_k10_against_oracle(ctx):
    params, _ = shape_params("c", 10, 8)
    circ = PhasedCircuit(params, 61)
    kzg, _ = srs(ctx, 10, 61)
    pk = PL.keygen(kzg, params, circ.fixed, circ.copies)
    try:
        adv = [None] * circ.sh.num_advice_total
        for p, idx in enumerate(circ.phase_cols):
            for c, v in zip(idx, circ.witness(p, [777 + i for i in range(circ._ch_before(p))])):
                adv[c] = v
        assert PL.check_witness(pk, adv, []) == (0, [])
        bad = list(adv)
        last = circ.phase_cols[-1][0]
        bad[last] = _with(bad[last], 101, 5)
        want = W.check(circ.sh, circ.fixed, bad, [], circ.copies)
        total, fails = PL.check_witness(pk, bad, [], 4096)
        assert want[0] > 0 and (total, _tuples(fails)) == want
    finally:
        pk.free()
        kzg.free()


# ---- the kernels' edges (tests/witness_edge_checks.py, shared with the CPU-emulated suite)
@pytest.mark.parametrize("k, lb", [(8, 6), (12, 11)])
@pytest.mark.parametrize("single", [False, True], ids=["lookup_advice", "q_lookup"])
def test_range_membership_whole_field(ctx, k, lb, single):
    WE.check_range_membership(ctx, k, lb, single)


@pytest.fixture(scope="module", params=[(10, 6, 3, 1, 1, 8), (14, 1, 1, 1, 1, 8)], ids=["20_columns_k10", "5_columns_k14"])
def mask_case(request, ctx):
    c = WE.MaskBlockCase(ctx, request.param)   # two and a half blocks with the lookups across a boundary; two blocks per column
    yield c
    c.free()


@pytest.mark.parametrize("pattern", ["a", "b", "c", "d", "e"])
def test_failure_list_across_mask_blocks(ctx, mask_case, pattern):
    assert mask_case.blocks == (3 if mask_case.sh.k == 10 else 10)
    WE.check_mask_blocks(ctx, mask_case, pattern)


@pytest.mark.parametrize("key_cols", [1, 2, 3])
def test_dyn_equal_key_neighbours(ctx, key_cols):
    WE.check_dyn_neighbours(ctx, key_cols)


@pytest.mark.parametrize("key_cols", [1, 2, 3])
def test_dyn_equal_key_runs(ctx, key_cols):
    WE.check_dyn_runs(ctx, key_cols)


def test_copy_peers_above_255(ctx):
    WE.check_wide_copy_peers(ctx, (11, 291, 53, 1, 0, 10))   # the wide k = 11 shape: 345 permutation columns


def test_hand_built_key_gates_at_the_last_rows(ctx):
    WE.check_hand_built_key(ctx)


def test_device_advice_garbage_behind_usable_rows(ctx):
    WE.check_device_advice_garbage(ctx)


def test_rlc_gate_at_the_last_rows(ctx):
    WE.check_rlc_gate_edge(ctx, 7, 4)
