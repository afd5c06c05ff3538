"""Multi-phase BaseConfig circuits (SecondPhase / ThirdPhase gate and lookup-advice columns, challenges; reference
halo2-base/src/gates/flex_gate/mod.rs:62-70,121-137, gates/range/mod.rs:87-108) on the CPU: libh2hip's emulated build
against the test prover (itself pinned by tests/test_shape_oracle.py), the layout, the refusals and the error paths."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from halo2_lib_amd import plonk as PL
from halo2_lib_amd import testing as T
from oracle import c_oracle as CO
from oracle import plonk as P
from tests import shape_oracle as SO
from tests.dyn_lookup_util import rng_budget
from tests.phases_util import PhasedCircuit, PreDrawnRng, R, first_phase1_commitment, oracle_verify, prove_both, shape_params


class _OracleBackend:
    mul = staticmethod(CO.fr_mul)
    add = staticmethod(CO.fr_add)


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def _free(r):
    r["gpk"].free()
    r["kzg"].free()


# ---- 2. libh2hip (emulated build) against the test prover
@pytest.mark.parametrize("name,k", [("a", 5), ("b", 6), ("c", 7), ("d", 5), ("e", 6)])
def test_phased_proof_emulated(ctx, name, k):
    params, inst = shape_params(name, k, 4)
    r = prove_both(ctx, params, seed=k + ord(name), instance=inst)
    try:
        circ, got = r["circ"], r["got"]
        assert got == r["want"], "proof bytes differ from the test prover's"
        if name == "a":   # a timed run (a stream synchronisation per stage) of the same RNG stream gives the same bytes
            timed = PL.create_proof(r["gpk"], circ.advice0(), circ.instance_arrays(), PreDrawnRng(r["budget"], 1000 + k + ord(name)), {},
                                    phase_witness=circ.witness)
            assert timed == got, "the timed proof differs"
        if params.num_challenges_per_phase[0]:
            assert r["seen"][0][0] == 1 and len(r["seen"][0][1]) == 1   # phase 1 received the challenge squeezed after phase 0
        instances = circ.instances
        inst_arr = circ.instance_arrays()
        assert oracle_verify(r["params"], r["vk"], instances, got), "the test verifier rejects the proof"
        assert PL.verify_proof(r["gpk"], inst_arr, got), "h2hip_plonk_verify_proof_phased rejects the proof"
        bad = bytearray(got)
        bad[first_phase1_commitment(circ) + 3] ^= 1
        assert not oracle_verify(r["params"], r["vk"], instances, bytes(bad))
        assert not PL.verify_proof(r["gpk"], inst_arr, bytes(bad))
    finally:
        _free(r)


# ---- 3. one phase without challenges IS the BaseConfig
@pytest.mark.parametrize("base", [(6, 1, 1, 1, 0, 4), (6, 3, 2, 1, 1, 4), (5, 2, 0, 0, 0, None)], ids=["q_lookup", "lookup_advice", "no_lookups"])
def test_one_phase_is_base_config(ctx, base):
    from tests.dyn_lookup_util import srs

    k, na, nla, nf, ni, lb = base
    bp = PL.BaseCircuitParams.new(k, na, nla, nf, ni, lb)
    pp = PL.PhasedCircuitParams.new(k, [na], [nla], nf, ni, lb)
    bs, ps = PL.shape_of(ctx, bp), PL.shape_of(ctx, pp)
    assert bytes(bs) == bytes(ps)
    assert PL.describe(pp) == PL.describe(bp)
    sh = P.Shape(k, na, nla, nf, ni, lb)
    circ = T.build_circuit(sh, 9, _OracleBackend)
    kzg, _ = srs(ctx, k, 9)
    gb = PL.keygen(kzg, bp, circ.fixed, circ.copies)
    gp = PL.keygen(kzg, pp, circ.fixed, circ.copies)
    try:
        assert np.array_equal(gb.fixed_commitments, gp.fixed_commitments) and np.array_equal(gb.permutation_commitments, gp.permutation_commitments)
        assert gb.transcript_repr == gp.transcript_repr
        budget = rng_budget(sh)
        inst = [np.ascontiguousarray(c) for c in circ.instances]
        want = PL.create_proof(gb, circ.advice, inst, PreDrawnRng(budget, 5))
        got = PL.create_proof(gp, circ.advice, inst, PreDrawnRng(budget, 5))
        assert got == want
        assert PL.verify_proof(gp, inst, got)
    finally:
        gb.free()
        gp.free()
        kzg.free()


# ---- 4. the device-ChaCha path equals the pre-drawn array of the same stream
def test_chacha_device_path_equals_predrawn_array(ctx):
    from tests.dyn_lookup_util import srs

    params, _ = shape_params("a", 6, 4)
    circ = PhasedCircuit(params, 21)
    kzg, _ = srs(ctx, 6, 21)
    gpk = PL.keygen(kzg, params, circ.fixed, circ.copies)
    try:
        dev = PL.create_proof(gpk, circ.advice0(), [], PL.ChaChaRng(ctx.lib, 99), phase_witness=circ.witness)
        budget = rng_budget(circ.sh)
        arr = PL.ChaChaRng(ctx.lib, 99).fill(budget)
        pre = PL.create_proof(gpk, circ.advice0(), [], PL.ArrayRng(arr), phase_witness=circ.witness)
        host = PL.create_proof(gpk, circ.advice0(), [], PL.ChaChaRng(ctx.lib, 99, device=False), phase_witness=circ.witness)
        assert dev == pre == host
        assert PL.verify_proof(gpk, [], dev)
    finally:
        gpk.free()
        kzg.free()


# ---- 5. every schedule switch gives the same bytes
KNOBS = ["plonk_tail_overlap", "plonk_permute_in_commit", "plonk_lazy_upload", "plonk_early_intt", "plonk_side_on_lanes", "plonk_warm_keygen",
         "plonk_merge_products", "plonk_gate_before_join"]


def test_schedule_switches_give_identical_bytes(ctx):
    params, _ = shape_params("a", 5, 4)
    ref = prove_both(ctx, params, seed=31, oracle_prover=True)
    try:
        want = ref["want"]
        assert ref["got"] == want
    finally:
        _free(ref)
    for knob in KNOBS:
        saved = ctx.get_param(knob)
        try:
            for v in (0, 1):
                ctx.set_param(knob, v)
                r = prove_both(ctx, params, seed=31, oracle_prover=False)
                try:
                    assert r["got"] == want, (knob, v)
                finally:
                    _free(r)
        finally:
            ctx.set_param(knob, saved)


# ---- 6. errors leave the key and the context usable
def _base_proof(ctx):
    """a BaseConfig proof on the same context: (libh2hip bytes, oracle bytes)"""
    from tests.dyn_lookup_util import srs

    sh = P.Shape(5, 1, 1, 1, 0, 4)
    circ = T.build_circuit(sh, 3, _OracleBackend)
    kzg, params = srs(ctx, 5, 3)
    gpk = PL.keygen(kzg, PL.BaseCircuitParams.new(5, 1, 1, 1, 0, 4), circ.fixed, circ.copies)
    try:
        budget = rng_budget(sh)
        got = PL.create_proof(gpk, circ.advice, [], PreDrawnRng(budget, 8))
        asm = P.PermutationAssembly(sh)
        for l, r in circ.copies:
            asm.copy(l, r)
        pk = P.keygen(params, sh, circ.fixed, asm, 2)
        pk.vk.transcript_repr = gpk.transcript_repr
        want = P.create_proof(params, pk, circ.advice, [], PreDrawnRng(budget, 8), 2)
        return got, want
    finally:
        gpk.free()
        kzg.free()


def test_errors_leave_things_usable(ctx):
    import halo2_lib_amd as H
    from tests.dyn_lookup_util import srs

    params, _ = shape_params("a", 5, 4)
    ref = prove_both(ctx, params, seed=41)
    _free(ref)
    circ = PhasedCircuit(params, 41)
    kzg, _ = srs(ctx, 5, 41)
    gpk = PL.keygen(kzg, params, circ.fixed, circ.copies)
    budget = rng_budget(circ.sh)

    def again():
        got = PL.create_proof(gpk, circ.advice0(), [], PreDrawnRng(budget, 1041), phase_witness=circ.witness)
        assert got == ref["want"]
        b, bw = _base_proof(ctx)
        assert b == bw

    try:
        # a callback returning non-zero (the raw C ABI)
        cb = PL._PHASE_FN(lambda *_a: 3)
        wit = PL._PhaseWitness(C.cast(cb, C.c_void_p), None)
        adv = [np.ascontiguousarray(c) for c in circ.advice0()]
        arr = (C.c_void_p * len(adv))(*[a.ctypes.data for a in adv])
        proof = np.zeros(gpk.proof_size(), dtype=np.uint8)
        plen = C.c_size_t(0)
        rng = PreDrawnRng(budget, 1)
        fill = PL._RNG_FN(lambda _u, out, m: rng.fill_into(out, m))
        rc = ctx.lib.h2hip_plonk_create_proof_phased(ctx.handle, gpk.handle, arr, 0, None, None, C.cast(fill, C.c_void_p), None, C.byref(wit),
                                                    proof.ctypes.data, proof.nbytes, C.byref(plen), None)
        assert rc == -1 and b"phase 1" in ctx.lib.h2hip_last_error()
        again()
        # a Python exception in phase_witness
        def boom(_p, _c):
            raise KeyError("no witness today")
        with pytest.raises(KeyError, match="no witness today"):
            PL.create_proof(gpk, circ.advice0(), [], PreDrawnRng(budget, 2), phase_witness=boom)
        again()
        # a phase-1 lookup value outside the table
        bad = PhasedCircuit(params, 41, bad_lookup=True)
        with pytest.raises(H.H2HipError, match="missing from the table"):
            PL.create_proof(gpk, bad.advice0(), [], PreDrawnRng(budget, 3), phase_witness=bad.witness)
        again()
        # the single-phase entry on a multi-phase key
        rc = ctx.lib.h2hip_plonk_create_proof(ctx.handle, gpk.handle, arr, 0, None, None, C.cast(fill, C.c_void_p), None, proof.ctypes.data,
                                              proof.nbytes, C.byref(plen), None)
        assert rc == -1 and b"more than one phase" in ctx.lib.h2hip_last_error()
        again()
        # and the phased entry on a BaseConfig key
        sh = P.Shape(5, 1, 1, 1, 0, 4)
        bcirc = T.build_circuit(sh, 3, _OracleBackend)
        bk = PL.keygen(kzg, PL.BaseCircuitParams.new(5, 1, 1, 1, 0, 4), bcirc.fixed, bcirc.copies)
        try:
            rc = ctx.lib.h2hip_plonk_create_proof_phased(ctx.handle, bk.handle, arr, 0, None, None, C.cast(fill, C.c_void_p), None, None,
                                                        proof.ctypes.data, proof.nbytes, C.byref(plen), None)
            assert rc == -1 and b"multi-phase" in ctx.lib.h2hip_last_error()
        finally:
            bk.free()
    finally:
        gpk.free()
        kzg.free()


# ---- 7. the layout and the refusals
def _shape(lib, *a, **kw):
    out = PL.ConstraintSystemShape()
    rc = lib.h2hip_plonk_shape_of_phased(C.byref(PL.PhasedCircuitParams.new(*a, **kw)), C.byref(out))
    return rc, out


@pytest.mark.parametrize("bad", [
    dict(num_advice_per_phase=[1, 0, 1]),                                              # phase 2 after an empty phase 1
    dict(num_advice_per_phase=[0, 1]),                                                 # phase 1 after an empty phase 0
    dict(num_advice_per_phase=[1], num_challenges_per_phase=[0, 1]),                   # a challenge after an empty phase
    dict(num_advice_per_phase=[1, 1], num_challenges_per_phase=[5, 4]),                # nine challenges
    dict(num_advice_per_phase=[600, 600]),                                             # 1200 gate columns
    dict(num_advice_per_phase=[1, 1], num_lookup_advice_per_phase=[200, 100]),         # 300 lookup-advice columns
    dict(num_advice_per_phase=[0, 0]),                                                 # no gate column
])
def test_shape_of_phased_refuses(bad):
    import halo2_lib_amd as H

    lib = H.load_library()
    a = dict(num_lookup_advice_per_phase=[], num_challenges_per_phase=[])
    a.update(bad)
    rc, _ = _shape(lib, 10, a["num_advice_per_phase"], a["num_lookup_advice_per_phase"], 1, 0, 8, a["num_challenges_per_phase"])
    assert rc == -1


def test_shape_of_phased_layout():
    import halo2_lib_amd as H

    lib = H.load_library()
    # [1,1] / [1,1]: table, constant, q_lookup, q_enable x 2; advice: gate 0 (phase 0), gate 1 (phase 1), lookup advice of phase 1
    rc, out = _shape(lib, 10, [1, 1], [1, 1], 1, 0, 8, [1])
    assert rc == 0
    assert (out.num_advice_total, out.num_fixed_total, out.table_col, out.first_constant_col, out.q_lookup_col, out.first_q_enable_col) == (3, 5, 0, 1, 2, 3)
    assert (out.num_lookups, out.num_perm_columns, out.degree) == (2, 4, 5)
    # [2,1,1] / [1,0,1], one instance: no q_lookup, lookup advice of phase 0 (column 4) and phase 2 (column 5)
    rc, out = _shape(lib, 10, [2, 1, 1], [1, 0, 1], 2, 1, 8, [1, 1])
    assert rc == 0
    assert (out.num_advice_total, out.num_fixed_total, out.table_col, out.first_constant_col, out.q_lookup_col, out.first_q_enable_col) == (6, 7, 0, 1, -1, 3)
    assert (out.num_lookups, out.num_perm_columns, out.degree) == (2, 2 + 6 + 1, 4)
    # no lookup_bits: no table, no lookup-advice columns at all
    rc, out = _shape(lib, 10, [2, 3], [1, 1], 0, 0, None, [2])
    assert rc == 0 and (out.num_advice_total, out.table_col, out.num_lookups, out.num_fixed_total) == (5, -1, 0, 5)
    for p in (PL.PhasedCircuitParams.new(10, [1, 1], [1, 1], 1, 0, 8, [1]), PL.PhasedCircuitParams.new(10, [2, 1, 1], [1, 0, 1], 2, 1, 8, [1, 1])):
        sh = SO.Shape.phased(p)
        rc, out = _shape(lib, 10, list(p.num_advice_per_phase), list(p.num_lookup_advice_per_phase), p.num_fixed, p.num_instance,
                         p.lookup_bits, list(p.num_challenges_per_phase))
        assert (out.num_advice_total, out.num_fixed_total, out.num_lookups, out.num_perm_sets, out.degree, out.extended_k) == (
            sh.num_advice_total, sh.num_fixed_total, len(sh.lookups), sh.num_perm_sets, sh.degree, sh.extended_k)
        evals = len(sh.advice_queries) + len(sh.fixed_queries) + 1 + len(sh.perm_columns) + 3 * sh.num_perm_sets - 1 + 5 * len(sh.lookups)
        assert out.num_evals == evals
    assert PL.PhasedCircuitParams.new(10, [2, 1, 1], [1, 0, 1], 2, 1, 8).phase_columns() == [[0, 1, 4], [2], [3, 5]]


def test_sharding_a_phased_key_is_refused(ctx):
    from tests.dyn_lookup_util import srs

    params, _ = shape_params("a", 5, 4)
    circ = PhasedCircuit(params, 3)
    kzg, _ = srs(ctx, 5, 3)
    gpk = PL.keygen(kzg, params, circ.fixed, circ.copies)

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


# ---- 8. the struct agrees across the header, the Rust sys crate and ctypes
def test_phased_params_struct_layout_agrees():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "h2hip.h")).read()
    body = re.search(r"typedef struct h2hip_phased_circuit_params\s*\{(.*?)\}\s*h2hip_phased_circuit_params\s*;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = [(name, ty + ("x" + arr if arr else "")) for ty, name, arr in re.findall(r"(u?int32_t)\s+([a-z_]+)(?:\[(\d+)\])?\s*;", body)]
    c_fields = [(n, t.replace("uint32_t", "u32").replace("int32_t", "i32")) for n, t in c_fields]
    rs = open(os.path.join(root, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    rs_body = re.search(r"pub struct h2hip_phased_circuit_params\s*\{(.*?)\}", rs, flags=re.S).group(1)
    rs_fields = [(n, t + ("x" + a if a else "")) for n, t, a in
                 [(m.group(1), m.group(2) or m.group(3), m.group(4) or "") for m in re.finditer(r"pub ([a-z_]+): (?:(u32|i32)|\[(u32|i32); (\d+)\])", rs_body)]]

    def py(t):
        if isinstance(t, type) and issubclass(t, C.Array):
            return py(t._type_) + "x%d" % t._length_
        return {C.c_uint32: "u32", C.c_int32: "i32"}[t]

    py_fields = [(n, py(t)) for n, t in PL.PhasedCircuitParams._fields_]
    want = [("k", "u32"), ("num_advice_per_phase", "u32x3"), ("num_lookup_advice_per_phase", "u32x3"), ("num_fixed", "u32"), ("num_instance", "u32"),
            ("lookup_bits", "i32"), ("num_challenges_per_phase", "u32x3")]
    assert c_fields == rs_fields == py_fields == want
    assert C.sizeof(PL.PhasedCircuitParams) == 4 * 13
