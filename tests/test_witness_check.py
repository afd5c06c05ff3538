"""h2hip_plonk_check_witness (MockProver's verdict, halo2-base/src/utils/testing.rs:183-188) on the CPU-emulated build: honest witnesses of the
three configurations give no failure, seeded pranks give exactly the failure list of the test-side checker (tests/witness_check_oracle.py),
truncation, argument errors, agreement with create_proof / verify_proof, and the struct layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import halo2_lib_amd as H
from halo2_lib_amd import h2hip as B
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import testing as T
from oracle import bn254 as O
from oracle import c_oracle as CO
from oracle import plonk as P
from tests import witness_check_oracle as W
from tests import witness_edge_checks as WE
from tests.dyn_lookup_util import oracle_shape, ram_circuit, rng_budget, srs
from tests.phases_util import PhasedCircuit, shape_params
from tests.util import PreDrawnRng, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _OracleBackend:
    mul = staticmethod(CO.fr_mul)
    add = staticmethod(CO.fr_add)


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def _bump(col, row, by=1):
    col = np.array(col)
    col[row] = CO.fr_add(col[row : row + 1], O.ints_to_limbs([by], R))[0]
    return col


def _set(col, row, v):
    col = np.array(col)
    col[row] = O.ints_to_limbs([v % R], R)[0]
    return col


def _lib(pk, advice, instances, max_failures=1 << 12):
    total, fails = PL.check_witness(pk, advice, instances, max_failures)
    return total, [(B.WITNESS_GATE if f.kind == "gate" else B.WITNESS_LOOKUP if f.kind == "lookup" else B.WITNESS_COPY, f.column, f.row,
                    f.peer_column, f.peer_row) for f in fails]


class Base:
    """a BaseConfig circuit (testing.build_circuit) with its key on `ctx`"""

    def __init__(self, ctx, shape, seed=3):
        self.sh = P.Shape(*shape)
        self.kzg, self.params = srs(ctx, shape[0], seed)
        self.circ = T.build_circuit(self.sh, seed, _OracleBackend)
        self.bp = PL.BaseCircuitParams.new(*shape)
        self.pk = PL.keygen(self.kzg, self.bp, self.circ.fixed, self.circ.copies)
        self.advice, self.instances = [np.array(c) for c in self.circ.advice], [np.array(c) for c in self.circ.instances]

    def oracle(self, advice=None, instances=None):
        return W.check(self.sh, self.circ.fixed, self.advice if advice is None else advice, self.instances if instances is None else instances,
                       self.circ.copies)

    def free(self):
        self.pk.free()
        self.kzg.free()


# ---- the test-side checker's own known answers (k = 5: 25 usable rows)
def test_oracle_known_answers():
    sh = P.Shape(5, 2, 1, 1, 1, 3)   # two gate columns, one lookup-advice column (table 0..7), one constant, one instance
    u = sh.usable_rows
    assert u == 25
    z = lambda: [0] * sh.n
    fixed = [z() for _ in range(sh.num_fixed_total)]
    fixed[sh.table_col][:8] = list(range(8))
    fixed[sh.constant_cols[0]][0] = 5
    adv = [z() for _ in range(sh.num_advice_total)]
    q0, q1 = sh.q_enable_cols
    adv[0][0:4] = [2, 3, 4, 14]          # 2 + 3 * 4 = 14: holds
    fixed[q0][0] = 1
    adv[0][4:8] = [1, 1, 1, 3]           # 1 + 1 = 2 != 3: gate column 0 fails at row 4
    fixed[q0][4] = 1
    fixed[q1][u - 2] = 1                 # reaches the blinding rows: fails whatever the values
    adv[2][:3] = [7, 8, 5]               # 8 is outside the table: lookup 0 fails at row 1
    adv[1][0] = 5                        # copied from the constant 5: holds
    adv[1][1] = 6                        # copied to instance row 0 = 9: fails both ways
    copies = [((("fixed", sh.constant_cols[0]), 0), (("advice", 1), 0)), ((("advice", 1), 1), (("instance", 0), 0))]
    limbs = lambda cols: [O.ints_to_limbs(c, R) for c in cols]
    total, got = W.check(sh, limbs(fixed), limbs(adv), [[9]], copies)
    p_adv1, p_inst = 1 + 1, 1 + sh.num_advice_total   # permutation columns: constant, advice 0, advice 1, advice 2, instance
    assert got == [(W.GATE, 0, 4, 0, 0), (W.GATE, 1, u - 2, 0, 0), (W.LOOKUP, 0, 1, 0, 0), (W.COPY, p_adv1, 1, p_inst, 0),
                   (W.COPY, p_inst, 0, p_adv1, 1)]
    assert total == 5
    adv[1][1], adv[0][7], fixed[q1][u - 2], adv[2][1] = 9, 2, 0, 1
    assert W.check(sh, limbs(fixed), limbs(adv), [[9]], copies) == (0, [])


# ---- honest witnesses: no failure in any configuration
@pytest.mark.parametrize("shape", [(6, 1, 1, 1, 0, 4), (7, 2, 2, 1, 1, 5)], ids=["q_lookup", "lookup_advice_instance"])
def test_honest_base(ctx, shape):
    b = Base(ctx, shape)
    try:
        assert b.oracle() == (0, [])
        assert PL.check_witness(b.pk, b.advice, b.instances) == (0, [])
        PL.assert_satisfied(b.pk, b.advice, b.instances)
    finally:
        b.free()


@pytest.mark.parametrize("key_cols", [1, 2, 3])
def test_honest_and_pranked_dyn(ctx, key_cols):
    for prank in (False, True):
        circ, dp, advice, fixed, copies = ram_circuit(5, 50, 16, key_cols, 3, 40 + key_cols, prank=prank)
        sh = oracle_shape(dp)
        kzg, _ = srs(ctx, 5, key_cols)
        pk = PL.keygen(kzg, dp, fixed, copies)
        try:
            want = W.check(sh, fixed, advice, [], copies)
            assert (want[0] == 0) != (prank and key_cols > 1)   # key_cols 1 looks up the index alone: (0, 0) is then a member
            assert _lib(pk, advice, []) == want
        finally:
            pk.free()
            kzg.free()


def _phased_advice(circ):
    """every phase's columns in advice index order (a challenge value stands in for the squeezed ones: the chains hold for any)"""
    cols = [None] * circ.sh.num_advice_total
    for p, idx in enumerate(circ.phase_cols):
        ch = [12345 + i for i in range(circ._ch_before(p))]
        for c, v in zip(idx, circ.witness(p, ch)):
            cols[c] = v
    return cols


@pytest.mark.parametrize("name", ["a", "c", "e"], ids=["2_phases", "3_phases", "2_phases_instance"])
def test_honest_and_pranked_phased(ctx, name):
    params, inst = shape_params(name, 6, 4)
    circ = PhasedCircuit(params, 9, instance=inst)
    kzg, _ = srs(ctx, 6, 9)
    pk = PL.keygen(kzg, params, circ.fixed, circ.copies)
    try:
        adv = _phased_advice(circ)
        insts = circ.instance_arrays()
        assert W.check(circ.sh, circ.fixed, adv, insts, circ.copies) == (0, [])
        assert _lib(pk, adv, insts) == (0, [])
        last = circ.phase_cols[-1][0]   # a later-phase gate column: its chain breaks at row 5
        bad = list(adv)
        bad[last] = _bump(bad[last], 5)
        want = W.check(circ.sh, circ.fixed, bad, insts, circ.copies)
        assert want[0] > 0 and _lib(pk, bad, insts) == want
    finally:
        pk.free()
        kzg.free()


# ---- seeded pranks of every kind: the library's list is the checker's, order included
def test_pranks_base(ctx):
    b = Base(ctx, (7, 2, 2, 1, 1, 5))
    try:
        sh, u = b.sh, b.sh.usable_rows
        la = sh.lookup_advice[0]
        inst0 = sh.num_fixed + sh.num_advice_total   # permutation column of instance 0
        copied = [(l, r) for l, r in b.circ.copies if l[0][0] == "advice" and r[0][0] == "advice"]
        (cl, rl), _ = copied[0]
        pranks = {
            "gate": lambda a, i: (a[:0] + [_bump(a[0], 9)] + a[1:], i),
            "lookup": lambda a, i: (a[:la] + [_set(a[la], 3, 1 << 20)] + a[la + 1:], i),
            "copy": lambda a, i: (a[:cl[1]] + [_bump(a[cl[1]], rl, 5)] + a[cl[1] + 1:], i),
            "instance": lambda a, i: (a, [_bump(i[0], 0)] + i[1:]),
            "all_rows": lambda a, i: (a[:la] + [np.array(O.ints_to_limbs([1 << 30] * sh.n, R))] + a[la + 1:], i),
        }
        for name, f in pranks.items():
            adv, inst = f(list(b.advice), list(b.instances))
            want = b.oracle(adv, inst)
            assert want[0] > 0, name
            assert _lib(b.pk, adv, inst) == want, name
            if name == "instance":
                assert any(w[0] == W.COPY and inst0 in (w[1], w[3]) for w in want[1])
            if name == "all_rows":   # every usable row of the lookup-advice column: the exact total
                assert sum(1 for w in want[1] if w[0] == W.LOOKUP and w[1] == 0) == u
    finally:
        b.free()


def test_truncation(ctx):
    b = Base(ctx, (6, 2, 1, 1, 0, 3))
    try:
        adv = list(b.advice)
        for c in range(len(adv)):   # many failures of every kind
            adv[c] = np.array(O.ints_to_limbs([(3 * r + c) % 97 + 9 for r in range(b.sh.n)], R))
        total, want = b.oracle(adv)
        assert total > 40
        for mx in [0, 1, 2, 7, total - 1, total, total + 5]:
            got_total, got = _lib(b.pk, adv, [], mx)
            assert got_total == total and got == want[: min(mx, total)], mx
    finally:
        b.free()


def test_argument_errors_then_proof_bytes(ctx):
    b = Base(ctx, (6, 1, 1, 1, 1, 4))
    try:
        lib, pk = ctx.lib, b.pk
        n = C.c_size_t(0)
        keep = [np.ascontiguousarray(c) for c in b.advice]
        adv = (C.c_void_p * len(keep))(*[c.ctypes.data for c in keep])
        inst = np.ascontiguousarray(b.instances[0])
        ip = (C.c_void_p * 1)(inst.ctypes.data)
        il = (C.c_size_t * 1)(len(inst))
        assert lib.h2hip_plonk_check_witness(ctx.handle, pk.handle, adv, 0, ip, il, None, 0, C.byref(n)) == 0 and n.value == 0
        nul = (C.c_void_p * len(keep))(*([None] + [c.ctypes.data for c in keep[1:]]))
        assert lib.h2hip_plonk_check_witness(ctx.handle, pk.handle, nul, 0, ip, il, None, 0, C.byref(n)) == -1
        assert b"NULL advice column" in lib.h2hip_last_error()
        long_l = (C.c_size_t * 1)(b.sh.usable_rows + 1)
        big = np.zeros((b.sh.usable_rows + 1, 4), dtype=np.uint64)
        assert lib.h2hip_plonk_check_witness(ctx.handle, pk.handle, adv, 0, (C.c_void_p * 1)(big.ctypes.data), long_l, None, 0, C.byref(n)) == -1
        assert lib.h2hip_plonk_check_witness(ctx.handle, pk.handle, adv, 0, ip, il, None, 0, None) == -1
        assert lib.h2hip_plonk_check_witness(ctx.handle, pk.handle, adv, 0, ip, il, None, 3, C.byref(n)) == -1
        assert lib.h2hip_plonk_check_witness(ctx.handle, pk.handle, adv, 0, None, None, None, 0, C.byref(n)) == -1   # instance_lens missing
        with pytest.raises(ValueError):
            PL.check_witness(pk, keep[:-1], b.instances)
        # the context and the key still prove the same bytes as the oracle prover
        budget = rng_budget(b.sh)
        asm = P.PermutationAssembly(b.sh)
        for l, r in b.circ.copies:
            asm.copy(l, r)
        opk = P.keygen(b.params, b.sh, b.circ.fixed, asm, 2)
        got = PL.create_proof(pk, b.advice, b.instances, PreDrawnRng(budget, 5))
        want = P.create_proof(b.params, opk, b.advice, [O.limbs_to_ints(i, R) for i in b.instances], PreDrawnRng(budget, 5), 2)
        assert got == want
    finally:
        b.free()


def test_agreement_with_prover(ctx):
    """0 failures <=> create_proof succeeds and verify_proof accepts; a lookup prank fails create_proof, a gate or copy prank gives a rejected proof"""
    b = Base(ctx, (6, 2, 1, 1, 1, 4), seed=11)
    try:
        budget = rng_budget(b.sh)
        la = b.sh.lookup_advice[0]
        g = np.random.default_rng(123)
        cases = [("honest", list(b.advice), list(b.instances))]
        for i in range(3):
            col, row = int(g.integers(0, 2)), int(g.integers(0, b.sh.usable_rows))
            a = list(b.advice)
            a[col] = _bump(a[col], row, int(g.integers(1, 1000)))
            cases.append(("advice%d" % i, a, list(b.instances)))
        a = list(b.advice)
        a[la] = _set(a[la], int(g.integers(0, b.sh.usable_rows)), 1 << 33)
        cases.append(("lookup", a, list(b.instances)))
        cases.append(("instance", list(b.advice), [_bump(b.instances[0], 1)]))
        for name, adv, inst in cases:
            total, fails = PL.check_witness(b.pk, adv, inst)
            try:
                proof = PL.create_proof(b.pk, adv, inst, PreDrawnRng(budget, 9))
            except H.H2HipError:
                proof = None
            if proof is None:
                assert any(f.kind == "lookup" for f in fails), name
                continue
            assert (total == 0) == PL.verify_proof(b.pk, inst, proof), (name, total)
    finally:
        b.free()


def test_struct_layout_and_messages(ctx):
    assert C.sizeof(B.WitnessFailureStruct) == 20 and [f[0] for f in B.WitnessFailureStruct._fields_] == ["kind", "column", "row", "peer_column",
                                                                                                           "peer_row"]
    hdr = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    m = re.search(r"typedef struct h2hip_witness_failure \{\s*uint32_t kind, column, row, peer_column, peer_row;\s*\} h2hip_witness_failure;", hdr)
    assert m
    assert re.search(r"#define H2HIP_WITNESS_GATE 1\b", hdr) and re.search(r"#define H2HIP_WITNESS_LOOKUP 2\b", hdr) and re.search(
        r"#define H2HIP_WITNESS_COPY 3\b", hdr)
    rs = open(os.path.join(ROOT, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    assert re.search(r"#\[repr\(C\)\]\s*(#\[derive[^\]]*\]\s*)?pub struct h2hip_witness_failure \{\s*pub kind: u32,\s*pub column: u32,\s*pub row: u32,"
                     r"\s*pub peer_column: u32,\s*pub peer_row: u32,?\s*\}", rs)
    for name, v in (("GATE", 1), ("LOOKUP", 2), ("COPY", 3)):
        assert re.search(r"pub const H2HIP_WITNESS_%s: u32 = %d;" % (name, v), rs)
    b = Base(ctx, (6, 1, 1, 1, 0, 4))
    try:
        adv = list(b.advice)
        adv[0] = _bump(adv[0], 13)
        with pytest.raises(AssertionError, match=r"gate column 0 not satisfied at row 1[0-3]"):
            PL.assert_satisfied(b.pk, adv)
        total, fails = PL.check_witness(b.pk, adv, max_failures=0)
        assert total > 0 and fails == []
    finally:
        b.free()


# ---- the kernels' edges (tests/witness_edge_checks.py, shared with the GPU suite)
@pytest.mark.parametrize("single", [False, True], ids=["lookup_advice", "q_lookup"])
def test_range_membership_whole_field(ctx, single):
    WE.check_range_membership(ctx, 8, 6, single)


@pytest.fixture(scope="module")
def mask_case(ctx):
    c = WE.MaskBlockCase(ctx, (10, 6, 3, 1, 1, 8))   # 20 mask columns of 1024 units: two and a half blocks
    yield c
    c.free()


@pytest.mark.parametrize("pattern", ["a", "b", "c", "d", "e"])
def test_failure_list_across_mask_blocks(ctx, mask_case, pattern):
    assert mask_case.blocks == 3
    WE.check_mask_blocks(ctx, mask_case, pattern)


@pytest.mark.parametrize("key_cols", [1, 2, 3])
def test_dyn_equal_key_neighbours(ctx, key_cols):
    WE.check_dyn_neighbours(ctx, key_cols)


@pytest.mark.parametrize("key_cols", [1, 2, 3])
def test_dyn_equal_key_runs(ctx, key_cols):
    WE.check_dyn_runs(ctx, key_cols)


def test_copy_peers_above_255(ctx):
    WE.check_wide_copy_peers(ctx, (6, 200, 60, 1, 0, 4))   # 261 permutation columns


def test_hand_built_key_gates_at_the_last_rows(ctx):
    WE.check_hand_built_key(ctx)


def test_device_advice_garbage_behind_usable_rows(ctx):
    WE.check_device_advice_garbage(ctx)


def test_rlc_gate_at_the_last_rows(ctx):
    from tests import rlc_checks as RC

    WE.check_rlc_gate_edge(ctx, RC.EMU_K, 4)
