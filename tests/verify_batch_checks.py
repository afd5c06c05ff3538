"""Backend-agnostic checks of the batch verifier (h2hip_plonk_verify_batch, halo2-lib_amd/csrc/verify_batch.hip) and of the checked point
decompressor under it (h2hip_g1_decompress_checked_dev): run on the CPU-emulated build by tests/test_verify_batch.py and on the GPU by
tests/test_verify_batch_gpu.py.

A `Case` is one verifying key of one of the three configurations with several proofs of DISTINCT witnesses (and distinct instances where the
shape has an instance column), one proof forged from a witness that violates the gate, and the Python oracle verifier of that configuration.
"""
import ctypes as C

import numpy as np
import pytest

import halo2_lib_amd as H
from halo2_lib_amd import halo2_proofs as HP
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import testing as T
from halo2_lib_amd import virtual_region as V
from oracle import bn254 as O
from oracle import c_oracle as CO
from oracle import plonk as P
from tests import dyn_lookup_util as DU
from tests import phases_util as PU
from tests.util import PreDrawnRng, R, rand_fr

Q = O.Q_MOD
ERR_INVALID = -1
_vp = C.c_void_p


class _OracleBackend:
    mul = staticmethod(CO.fr_mul)
    add = staticmethod(CO.fr_add)


class Case:
    def __init__(self, ctx, gpk, kzg, items, forged, oracle):
        self.ctx, self.gpk, self.kzg, self.items, self.forged, self._oracle = ctx, gpk, kzg, items, forged, oracle
        self.has_instance = gpk.params.num_instance > 0
        self.first_eval = 32 * (gpk.shape.num_commitments - 2)   # the commitments up to the h pieces come first; h1 and h2 are the last two words
        self._single = {}

    def oracle_verify(self, inst, proof):
        try:
            return bool(self._oracle([O.limbs_to_ints(v, R) for v in inst], proof))
        except P.VerifyError:
            return False

    def single(self, inst, proof):
        """the verdict of the single verifier (cached: the good proofs are asked about again and again)"""
        key = (tuple(np.asarray(v).tobytes() for v in inst), bytes(proof))
        if key not in self._single:
            self._single[key] = PL.verify_proof(self.gpk, inst, proof)
        return self._single[key]

    def free(self):
        self.gpk.free()
        self.kzg.free()


# ------------------------------------------------------------------------------------------------------------------ the three configurations
def _one(v):
    return O.ints_to_limbs([v], R)


def _base_witness(circ, i):
    """witness i of the key circ belongs to: the free `c` cell of gate 3 and the PUBLIC `c` cell of gate 1 of gate column 0 take new values
    (neither gate's d feeds another cell, and no copy constraint other than the instance's touches those cells), d = a + b*c follows"""
    adv = [np.array(c) for c in circ.advice]
    inst = [np.array(v) for v in circ.instances]
    if i:
        col = adv[0]
        for gate, val in ((1, 1000 + i), (3, 5000 + 7 * i)):
            col[4 * gate + 2] = _one(val)[0]
            col[4 * gate + 3] = CO.fr_add(col[4 * gate:4 * gate + 1], CO.fr_mul(col[4 * gate + 1:4 * gate + 2], col[4 * gate + 2:4 * gate + 3]))[0]
        for v in inst:
            v[1] = col[4 * 1 + 2]
    return adv, inst


def base_case(ctx, shape, nproofs, seed=3):
    k, na, nl, nf, ni, lb = shape
    sh = P.Shape(k, na, nl, nf, ni, lb)
    s_toxic = 0x1D0C0FFEE1234567890ABCDEF + seed
    kzg = HP.ParamsKZG.setup(ctx, k, s_toxic)
    params = P.Params.setup(k, s_toxic, g=ctx.bases_download(kzg.g), g_lagrange=ctx.bases_download(kzg.g_lagrange))
    circ = T.build_circuit(sh, seed, _OracleBackend)
    gpk = PL.keygen(kzg, PL.BaseCircuitParams.new(k, na, nl, nf, ni, lb), circ.fixed, circ.copies)
    budget = DU.rng_budget(sh)
    items = []
    for i in range(nproofs):
        adv, inst = _base_witness(circ, i)
        items.append((inst, PL.create_proof(gpk, adv, inst, PreDrawnRng(budget, 1000 + seed + i))))
    adv, inst = _base_witness(circ, 0)
    adv[0][3] = CO.fr_add(adv[0][3:4], _one(1))[0]   # a + b*c != d in gate 0
    forged = (inst, PL.create_proof(gpk, adv, inst, PreDrawnRng(budget, 7)))
    vk = DU.vk_from_gpu(sh, gpk) if len(gpk.permutation_commitments) else P.VerifyingKey(
        sh, O.limbs_to_points(np.ascontiguousarray(gpk.fixed_commitments).reshape(-1, 8)), [], gpk.transcript_repr)
    return Case(ctx, gpk, kzg, items, forged, lambda inst, proof: P.verify_proof(params, vk, inst, proof))


def dyn_case(ctx, k, nproofs, accesses=50, mem_len=16, key_cols=2, lu_sets=3, seed=2):
    g = np.random.default_rng(seed)
    ptrs = [int(v) for v in g.integers(0, mem_len, size=accesses)]

    def witness(i):   # the same accesses (the key's structure), other memory contents
        memory = [int(v) for v in np.random.default_rng([seed, i]).integers(1, 2**62, size=mem_len)]
        circ = V.RAMCircuit(memory, ptrs, key_cols)
        dp = PL.DynLookupCircuitParams.new(k, circ.num_advice_needed(k), 1, key_cols, lu_sets)
        return (dp,) + tuple(circ.synthesize(dp))

    dp, advice0, fixed, copies = witness(0)
    sh = DU.oracle_shape(dp)
    kzg, params = DU.srs(ctx, k, seed)
    gpk = PL.keygen(kzg, dp, fixed, copies)
    budget = DU.rng_budget(sh)
    items = []
    for i in range(nproofs):
        _, adv, fx, cp = witness(i)
        assert all(np.array_equal(a, b) for a, b in zip(fx, fixed)) and list(cp) == list(copies), "the witnesses must share the key"
        items.append(([], PL.create_proof(gpk, adv, [], PreDrawnRng(budget, 1000 + seed + i))))
    adv = [np.array(c) for c in advice0]
    gate0 = dp.key_cols * (1 + dp.lu_sets)   # the first FlexGate column
    adv[gate0][3] = CO.fr_add(adv[gate0][3:4], _one(1))[0]
    forged = ([], PL.create_proof(gpk, adv, [], PreDrawnRng(budget, 7)))
    vk = DU.vk_from_gpu(sh, gpk)
    return Case(ctx, gpk, kzg, items, forged, lambda inst, proof: DU.oracle_verify(params, vk, proof))


def phased_case(ctx, name, k, nproofs, lookup_bits=4, seed=5):
    pp, inst = PU.shape_params(name, k, lookup_bits)
    circ0 = PU.PhasedCircuit(pp, seed, instance=inst)
    kzg, params = DU.srs(ctx, k, seed)
    gpk = PL.keygen(kzg, pp, circ0.fixed, circ0.copies)
    budget = DU.rng_budget(circ0.sh)
    items = []
    seen, next_seed = set(), seed
    for i in range(nproofs):
        while True:   # the public cells are small values: take the next seed whose instance column is a new one
            circ = PU.PhasedCircuit(pp, next_seed, instance=inst)
            next_seed += 100
            if not inst or tuple(circ.instances[0]) not in seen:
                break
        seen.add(tuple(circ.instances[0]) if inst else None)
        assert all(np.array_equal(a, b) for a, b in zip(circ.fixed, circ0.fixed)) and circ.copies == circ0.copies, "the witnesses must share the key"
        items.append((circ.instance_arrays(), PL.create_proof(gpk, circ.advice0(), circ.instance_arrays(), PreDrawnRng(budget, 1000 + seed + i),
                                                              phase_witness=circ.witness)))
    adv = [np.array(c) for c in circ0.advice0()]
    adv[0][3] = CO.fr_add(adv[0][3:4], _one(1))[0]
    forged = (circ0.instance_arrays(), PL.create_proof(gpk, adv, circ0.instance_arrays(), PreDrawnRng(budget, 7), phase_witness=circ0.witness))
    vk = DU.vk_from_gpu(circ0.sh, gpk)
    return Case(ctx, gpk, kzg, items, forged, lambda inst, proof: PU.oracle_verify(params, vk, inst, proof))


# ------------------------------------------------------------------------------------------------------------------ 1. the decompressor
def expected_point(word: bytes):
    """(status, point) of one 32-byte word by the definition, in Python integers: 0 ok, 1 the identity encoding, 2 malformed"""
    top = word[31]
    x = int.from_bytes(word[:31] + bytes([top & 0x3F]), "little")
    if top & 0x80:
        return (1, None) if x == 0 and not top & 0x40 else (2, None)
    if x >= Q:
        return 2, None
    y2 = (x * x * x + O.CURVE_B) % Q
    y = pow(y2, (Q + 1) // 4, Q)
    if y * y % Q != y2:
        return 2, None
    if y & 1 != (top >> 6) & 1:
        y = Q - y
    assert O.g1_is_on_curve((x, y))
    return 0, (x, y)


def decompress_words(n, seed):
    """n words: random x (about half of them off the curve) with random sign bits, and at fixed places x >= q, the identity flag over a
    non-zero x, the identity flag with the sign bit, the pure identity encoding, and both signs of one known point"""
    g = np.random.default_rng(seed)
    words = []
    for _ in range(n):
        x = int.from_bytes(g.bytes(32), "little") % Q
        words.append(bytearray(x.to_bytes(32, "little")))
        words[-1][31] |= int(g.integers(0, 2)) << 6
    gen = bytearray((1).to_bytes(32, "little"))   # x = 1: (1, 2) and (1, q - 2)
    special = [bytearray(Q.to_bytes(32, "little")), bytearray((Q + 5).to_bytes(32, "little")), bytearray(((1 << 254) - 1).to_bytes(32, "little")),
               bytearray((7).to_bytes(31, "little") + b"\x80"), bytearray(bytes(31) + b"\xc0"), bytearray(bytes(31) + b"\x80"), bytearray(gen),
               bytearray(gen[:31] + b"\x40")]
    for j, w in enumerate(special):
        if n:
            words[(j * 37 + (n - 1 if j == 0 else 0)) % n] = w   # the first special word is the LAST lane
    return [bytes(w) for w in words]


def check_decompressor(ctx, n, seed=11):
    lib = ctx.lib
    words = decompress_words(n, seed)
    want = [expected_point(w) for w in words]
    if n >= 255:   # the oracle run confirms the mix before the kernel is asked
        assert sum(1 for s, _ in want if s == 2) * 3 >= n and sum(1 for s, _ in want if s == 0) * 3 >= n
        assert {s for s, _ in want} == {0, 1, 2}
    table = np.frombuffer(b"".join(words) or bytes(32), dtype=np.uint8).copy()
    d_words = ctx.to_device(table)
    slot_sets = [None, np.arange(n, dtype=np.uint32)[::-1].copy(), np.repeat(np.arange((n + 2) // 3, dtype=np.uint32), 3)[:n].copy()]
    d_out, d_status = ctx.malloc(64 * max(n, 1)), ctx.malloc(4 * max(n, 1))
    try:
        for slots in slot_sets:
            order = list(range(n)) if slots is None else [int(s) for s in slots]
            d_slots = ctx.to_device(slots) if slots is not None and n else None
            ctx._chk(lib.h2hip_g1_decompress_checked_dev(ctx.handle, _vp(d_words), _vp(d_slots) if d_slots else None, n, _vp(d_out), _vp(d_status)))
            ctx.sync()
            if d_slots:
                ctx.free(d_slots)
            if not n:
                continue
            status = ctx.download(d_status, (n,), np.uint32)
            pts = O.limbs_to_points(ctx.download(d_out, (n, 8)))
            assert [int(s) for s in status] == [want[j][0] for j in order]
            assert pts == [want[j][1] for j in order]
        # the valid points: what the SRS decompressor gives for the same words (it fails the whole call on a malformed one)
        good = [j for j in range(n) if want[j][0] == 0]
        if good:
            d_good = ctx.to_device(np.frombuffer(b"".join(words[j] for j in good), dtype=np.uint8).copy())
            d_ref, d_got, d_st = ctx.malloc(64 * len(good)), ctx.malloc(64 * len(good)), ctx.malloc(4 * len(good))
            ctx._chk(lib.h2hip_g1_decompress_batch_dev(ctx.handle, _vp(d_good), len(good), _vp(d_ref), 6, 7))
            ctx._chk(lib.h2hip_g1_decompress_checked_dev(ctx.handle, _vp(d_good), None, len(good), _vp(d_got), _vp(d_st)))
            ctx.sync()
            assert np.array_equal(ctx.download(d_got, (len(good), 8)), ctx.download(d_ref, (len(good), 8)))
            assert not ctx.download(d_st, (len(good),), np.uint32).any()
            for p in (d_good, d_ref, d_got, d_st):
                ctx.free(p)
    finally:
        for p in (d_words, d_out, d_status):
            ctx.free(p)


# ------------------------------------------------------------------------------------------------------------------ helpers
class CountingRng:
    """serves pre-drawn combiners and records every call"""

    def __init__(self, values):
        self.values, self.calls = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4), []

    def fill_into(self, dst, n):
        self.calls.append(n)
        C.memmove(dst, self.values.ctypes.data, 32 * n)


def rho_rng(count, seed=77):
    return CountingRng(rand_fr(max(count, 1), seed))


def batch(case, items, rng=None, want_rejected=False, want_acc=False, kind=None):
    return PL.verify_batch(case.gpk, [i for i, _ in items], [p for _, p in items], rng or rho_rng(len(items)), want_rejected, want_acc, kind)


def acc_points(acc):
    return O.limbs_to_points(np.ascontiguousarray(acc).reshape(2, 8))


# ------------------------------------------------------------------------------------------------------------------ 2. accept
def check_accept(case, count):
    items = case.items[:count]
    assert len(items) == count and len({p for _, p in items}) == count
    if case.has_instance and count > 1:
        assert len({np.asarray(i[0]).tobytes() for i, _ in items}) == count, "the instances must differ"
    ok, rejected, _ = batch(case, items, want_rejected=True)
    assert ok and rejected == [False] * count
    assert batch(case, items)[0]
    assert all(case.single(i, p) for i, p in items)


# ------------------------------------------------------------------------------------------------------------------ 3. the accumulator
def check_accumulator(case):
    lib, kzg = case.ctx.lib, case.kzg
    A, B = case.items[0], case.items[1]
    a, b = 0x1234567890ABCDEF1234567, R - 5
    ok, _, acc = batch(case, [A, B], CountingRng(O.ints_to_limbs([a, b], R)), want_acc=True)
    assert ok
    L, Rp = acc_points(acc)
    # e(L, s_g2) * e(-R, g2) == 1
    g2 = np.frombuffer(kzg.g2_raw, dtype=np.uint8)
    g1 = O.points_to_limbs([L, O.g1_neg(Rp)])
    one = C.c_int(0)
    assert lib.h2hip_pairing_check(_vp(g1.ctypes.data), _vp(np.concatenate([g2[128:256], g2[:128]]).ctypes.data), 2, C.byref(one)) == 0 and one.value == 1
    # L = sum rho_i * (the last word of proof i)
    from oracle.transcript import g1_decompress

    w = [g1_decompress(p[-32:]) for _, p in (A, B)]
    assert L == O.g1_add(O.g1_mul(w[0], a), O.g1_mul(w[1], b))
    # linearity in the combiners, both components
    unit = lambda item: acc_points(batch(case, [item], CountingRng(O.ints_to_limbs([1], R)), want_acc=True)[2])
    ua, ub = unit(A), unit(B)
    assert ua[0] == w[0] and ub[0] == w[1]
    for c in (0, 1):
        assert (L, Rp)[c] == O.g1_add(O.g1_mul(ua[c], a), O.g1_mul(ub[c], b))
    # other combiners, another accumulator
    _, _, acc2 = batch(case, [A, B], CountingRng(O.ints_to_limbs([a + 1, b], R)), want_acc=True)
    L2, R2 = acc_points(acc2)
    assert L2 != L and R2 != Rp


# ------------------------------------------------------------------------------------------------------------------ 4. reject
MUTATIONS = ["eval_byte", "first_commitment_byte", "h2_byte", "truncated", "appended", "eval_is_r", "commitment_identity_bit", "first_instance",
             "forged"]


def mutate(case, name, item):
    inst, proof = item
    p = bytearray(proof)
    fe = case.first_eval
    if name == "eval_byte":
        p[fe + 5] ^= 1
    elif name == "first_commitment_byte":
        p[0] ^= 1
    elif name == "h2_byte":
        p[len(p) - 32] ^= 1
    elif name == "truncated":
        p = p[:-32]
    elif name == "appended":
        p += bytes(32)
    elif name == "eval_is_r":
        p[fe:fe + 32] = R.to_bytes(32, "little")
    elif name == "commitment_identity_bit":
        p[31] |= 0x80
    elif name == "first_instance":
        if not case.has_instance:
            return None
        inst = [np.array(v) for v in inst]
        inst[0][0] = CO.fr_add(inst[0][0:1], _one(1))[0]
    elif name == "forged":
        return case.forged
    else:
        raise KeyError(name)
    return inst, bytes(p)


def check_reject(case, name, positions=(0, 2, 4)):
    good = case.items[:5]
    assert len(good) == 5
    for pos in positions:
        bad = mutate(case, name, good[pos])
        if bad is None:
            return
        items = list(good)
        items[pos] = bad
        want = [not case.single(i, p) for i, p in items]
        assert want[pos] and sum(want) == 1, (name, pos, want)
        ok, rejected, _ = batch(case, items, want_rejected=True)
        assert not ok and rejected == want, (name, pos, rejected)
        assert not batch(case, items)[0]


def check_reject_two(case):
    good = case.items[:5]
    items = list(good)
    items[1] = mutate(case, "eval_byte", good[1])
    items[3] = case.forged
    want = [not case.single(i, p) for i, p in items]
    assert want == [False, True, False, True, False]
    ok, rejected, _ = batch(case, items, want_rejected=True)
    assert not ok and rejected == want
    assert not batch(case, items)[0]
    items[1] = mutate(case, "truncated", good[1])   # one malformed, one that only the pairing catches
    ok, rejected, _ = batch(case, items, want_rejected=True)
    assert not ok and rejected == want
    assert not batch(case, items)[0]


# ------------------------------------------------------------------------------------------------------------------ 5. protocol
def _raw_args(case, items, rng_cb, ok, drop=None):
    gpk, kzg, ctx = case.gpk, case.kzg, case.ctx
    keep = []
    inst = [PL._fe(c) for i, _ in items for c in i]
    ip = (_vp * max(len(inst), 1))(*[_vp(c.ctypes.data) for c in inst])
    il = (C.c_size_t * max(len(inst), 1))(*[len(c) for c in inst])
    bufs = [np.frombuffer(p, dtype=np.uint8).copy() for _, p in items]
    pp = (_vp * max(len(bufs), 1))(*[_vp(b.ctypes.data) for b in bufs])
    pl = (C.c_size_t * max(len(bufs), 1))(*[len(b) for b in bufs])
    g0 = ctx.bases_download(kzg.g)[:1].copy()
    g2 = np.frombuffer(kzg.g2_raw, dtype=np.uint8).copy()
    fc, pc = np.ascontiguousarray(gpk.fixed_commitments), np.ascontiguousarray(gpk.permutation_commitments)
    tr = HP.fr_limbs(gpk.transcript_repr)
    keep += [inst, ip, il, bufs, pp, pl, g0, g2, fc, pc, tr]
    args = dict(ctx=ctx.handle, kind=PL._CIRCUIT_KINDS[type(gpk.params)], params=C.cast(C.byref(gpk.params), _vp), fixed=_vp(fc.ctypes.data),
                perm=_vp(pc.ctypes.data), repr=_vp(tr.ctypes.data), g1=_vp(g0.ctypes.data), g2=_vp(g2.ctypes.data), s_g2=_vp(g2.ctypes.data + 128),
                n=len(items), inst=ip if case.has_instance else None, lens=il if case.has_instance else None, proofs=pp, plens=pl,
                rng=C.cast(rng_cb, _vp), user=None, accepted=C.byref(ok), rejected=None, acc=None)
    if drop:
        args[drop] = None
    return list(args.values()), keep


def check_protocol(case):
    lib = case.ctx.lib
    items = case.items[:3]
    good = lambda: batch(case, items)[0]
    # the rng: one call, num_proofs elements
    rng = rho_rng(3)
    assert batch(case, items, rng, want_rejected=True)[0] and rng.calls == [3]
    # a zero combiner
    zero = CountingRng(np.concatenate([rand_fr(1, 5), np.zeros((1, 4), dtype=np.uint64), rand_fr(1, 6)]))
    with pytest.raises(H.H2HipError) as ei:
        batch(case, items, zero)
    assert ei.value.code == ERR_INVALID
    assert zero.calls == [3] and good()
    # no proofs: accepted, the rng is not needed
    none = rho_rng(1)
    ok, rejected, acc = batch(case, [], none, want_rejected=True, want_acc=True)
    assert ok and rejected == [] and not acc.any() and none.calls == []
    # an unknown kind
    with pytest.raises(H.H2HipError) as ei:
        batch(case, items, kind=3)
    assert ei.value.code == ERR_INVALID
    assert good()
    # NULL arguments
    calls = []
    cb = PL._RNG_FN(lambda _u, out, n: (calls.append(n), C.memmove(out, rand_fr(n, 9).ctypes.data, 32 * n))[0])
    nullable = ["ctx", "params", "fixed", "repr", "g1", "g2", "s_g2", "proofs", "plens", "rng", "accepted"] + (["inst", "lens"] if case.has_instance else [])
    if case.gpk.shape.num_perm_columns:
        nullable.append("perm")
    for drop in nullable:
        ok = C.c_int(7)
        args, keep = _raw_args(case, items, cb, ok, drop)
        assert lib.h2hip_plonk_verify_batch(*args) == ERR_INVALID, drop
        assert b"NULL" in lib.h2hip_last_error() or drop == "ctx", (drop, lib.h2hip_last_error())
        del keep
    assert calls == [] and good()
    ok = C.c_int(7)
    args, keep = _raw_args(case, items, cb, ok)
    assert lib.h2hip_plonk_verify_batch(*args) == 0 and ok.value == 1 and calls == [3]


# ------------------------------------------------------------------------------------------------------------------ 6. the single verifier
def check_single_against_oracle(case, names=MUTATIONS):
    """the refactored single verifier (derive, then finish) says what the Python oracle verifier says, on the good proof and on every mutation"""
    item = case.items[0]
    assert case.single(*item) and case.oracle_verify(*item)
    for name in names:
        bad = mutate(case, name, item)
        if bad is None:
            continue
        assert case.single(*bad) == case.oracle_verify(*bad) == False, name


# ------------------------------------------------------------------------------------------------------------------ 7. the mirrors
def check_python_mirror(case):
    items = case.items[:3]
    insts, proofs = [i for i, _ in items], [p for _, p in items]
    assert PL.verify_proofs(case.gpk, insts, proofs) is True                       # the default rng: os.urandom-seeded ChaCha
    assert PL.verify_proofs(case.gpk, insts, proofs, want_rejected=True) == (True, [False] * 3)
    bad = list(items)
    bad[1] = mutate(case, "eval_byte", items[1])
    want = (False, [False, True, False])
    assert PL.verify_proofs(case.gpk, [i for i, _ in bad], [p for _, p in bad], rho_rng(3), want_rejected=True) == want
    assert batch(case, bad, want_rejected=True)[:2] == want
    assert PL.verify_proofs(case.gpk, [i for i, _ in bad], [p for _, p in bad]) is False
    bv = PL.BatchVerifier()
    for i, p in items:
        bv.add_proof(i, p)
    assert bv.finalize(case.gpk) is True
    bv.add_proof(*bad[1])
    assert bv.finalize(case.gpk, rho_rng(4)) is False
    assert PL.BatchVerifier().finalize(case.gpk) is True
