"""Proving and verifying over a caller-supplied transcript (h2hip_plonk_create_proof_transcript / h2hip_plonk_verify_proof_transcript), shared by
tests/test_transcript.py (the CPU-emulated build) and tests/test_transcript_gpu.py: every check takes a Case, built once per shape.

Two transcripts, both plain Python:
  T1  oracle.transcript.Blake2bWrite / Blake2bRead themselves: through the callbacks they must give the built-in entries' bytes;
  T2  a transcript the library has never seen: a sponge over oracle/poseidon.py's Spec(3, 8, 57) that absorbs a point as the four 128-bit
      halves of x and y and a scalar as itself, squeezes a full-width Fr, and serialises points uncompressed (64 B, big-endian) and scalars
      big-endian.  It claims no upstream format.  The two Python provers (oracle.plonk and tests/shape_oracle.py) build their transcript through the module-level names Blake2bWrite /
      Blake2bRead, so pytest's monkeypatch makes them prove and verify over T2: exact equalities, no recalled statement.
"""
import ctypes as C
import os
import re

import numpy as np

import halo2_lib_amd as H
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import testing as T
from oracle import bn254 as O
from oracle import c_oracle as CO
from oracle import plonk as P
from oracle import poseidon as PS
from oracle.transcript import Blake2bRead, Blake2bWrite
from tests import rlc_checks as RC
from tests import shape_oracle as SO
from tests.dyn_lookup_util import oracle_pk, oracle_shape, ram_circuit, rng_budget, srs
from tests.phases_util import PhasedCircuit, shape_params
from tests.util import PreDrawnRng, R, fr

_vp = C.c_void_p
Q = O.Q_MOD
ERR_INVALID = -1
THREADS = 4


# ------------------------------------------------------------------------------------------------ T2
_SPEC = []


def _spec():
    if not _SPEC:
        _SPEC.append(PS.Spec(3, 8, 57))
    return _SPEC[0]


class _T2:
    """The sponge: values wait in a buffer; a squeeze appends the marker 1, pads with zeros to the rate (2), adds every pair to state[1..]
    with a permutation each, and returns state[1]."""
    MASK = (1 << 128) - 1

    def __init__(self):
        self.state, self.buf = [0, 0, 0], []

    def common_point(self, pt):
        if pt is None:
            raise ValueError("cannot write points at infinity to the transcript")
        x, y = pt
        self.buf += [x & self.MASK, x >> 128, y & self.MASK, y >> 128]

    def common_scalar(self, s):
        self.buf.append(s % R)

    def squeeze_challenge(self):
        buf = self.buf + [1]
        buf += [0] * (len(buf) % 2)
        spec, s = _spec(), self.state
        for i in range(0, len(buf), 2):
            s = spec.permute([s[0], (s[1] + buf[i]) % R, (s[2] + buf[i + 1]) % R])
        self.state, self.buf = s, []
        return s[1]


class T2Write(_T2):
    def __init__(self):
        super().__init__()
        self.proof = bytearray()

    def write_point(self, pt):
        self.common_point(pt)
        self.proof += pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")

    def write_scalar(self, s):
        self.common_scalar(s)
        self.proof += (s % R).to_bytes(32, "big")

    def finalize(self):
        return bytes(self.proof)


class T2Read(_T2):
    def __init__(self, proof):
        super().__init__()
        self.proof, self.pos = bytes(proof), 0

    def _take(self, n):
        if self.pos + n > len(self.proof):
            raise ValueError("proof too short")
        b = self.proof[self.pos:self.pos + n]
        self.pos += n
        return b

    def read_point(self):
        b = self._take(64)
        x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
        if x >= Q or y >= Q or (y * y - x * x * x - 3) % Q != 0:
            raise ValueError("not a point of the curve")
        self.common_point((x, y))
        return (x, y)

    def read_scalar(self):
        s = int.from_bytes(self._take(32), "big")
        if s >= R:
            raise ValueError("invalid field element encoding in proof")
        self.common_scalar(s)
        return s

    def exhausted(self):
        return self.pos == len(self.proof)


# ------------------------------------------------------------------------------------------------ the shapes
class _Backend:
    mul = staticmethod(CO.fr_mul)
    add = staticmethod(CO.fr_add)


class Case:
    """One key with its witness, on libh2hip and on the matching Python prover (same SRS, same RNG stream)."""

    def __init__(self, ctx, name, oracle, params, sh, fixed, copies, advice, inst_ints, seed, witness=None, num_challenges=0):
        self.ctx, self.name, self.oracle, self.params, self.sh = ctx, name, oracle, params, sh
        self.fixed, self.copies, self.advice, self.inst_ints, self.seed, self.witness = fixed, copies, advice, inst_ints, seed, witness
        self.num_challenges = num_challenges
        self.inst = [O.ints_to_limbs(v, R) for v in inst_ints]
        self.kzg, self.srs = srs(ctx, params.k, seed)
        self.gpk = PL.keygen(self.kzg, params, fixed, copies)
        self.budget = rng_budget(sh)
        self._opk = None
        self.cache = {}

    def free(self):
        self.gpk.free()
        self.kzg.free()

    def rng(self):
        return PreDrawnRng(self.budget, 1000 + self.seed)

    def prove(self, rng=None, transcript=None, advice=None, advice_on_device=False):
        return PL.create_proof(self.gpk, self.advice if advice is None else advice, self.inst, rng or self.rng(), advice_on_device=advice_on_device,
                               phase_witness=self.witness, transcript=transcript)

    def verify(self, proof=None, transcript=None, want_accumulator=False):
        return PL.verify_proof(self.gpk, self.inst, proof, transcript=transcript, want_accumulator=want_accumulator)

    def opk(self):
        if self._opk is None:
            self._opk = oracle_pk(self.sh, self.srs, self.fixed, self.copies, THREADS)
            assert self._opk.vk.transcript_repr == self.gpk.transcript_repr, "verifying keys differ (fixed / permutation commitments)"
        return self._opk

    def oracle_prove(self):
        kw = {"phase_witness": self.witness} if self.witness else {}
        return self.oracle.create_proof(self.srs, self.opk(), self.advice, self.inst_ints, self.rng(), THREADS, **kw)

    def oracle_verify(self, proof):
        try:
            return bool(self.oracle.verify_proof(self.srs, self.opk().vk, self.inst_ints, proof))
        except (P.VerifyError, ValueError, AssertionError):
            return False

    def builtin(self):
        """the built-in entry's bytes for this case's RNG stream (computed once)"""
        if "builtin" not in self.cache:
            self.cache["builtin"] = self.prove()
        return self.cache["builtin"]

    def t2_proof(self):
        if "t2" not in self.cache:
            self.cache["t2"] = self.prove(transcript=T2Write())
        return self.cache["t2"]


def _base_case(ctx, name, k, na, nl, nf, ni, lb, seed):
    sh = P.Shape(k, na, nl, nf, ni, lb)
    circ = T.build_circuit(sh, seed, _Backend)
    return Case(ctx, name, P, PL.BaseCircuitParams.new(k, na, nl, nf, ni, lb), sh, circ.fixed, circ.copies, circ.advice,
                [O.limbs_to_ints(v, R) for v in circ.instances], seed)


def make_case(ctx, name, k):
    """the issue's five shapes; lookup_bits = max(4, k - 2): the phased circuit's cells go up to 12"""
    lb = max(4, k - 2)
    if name == "base1":    # one gate column with q_lookup: the lone-commitment path
        return _base_case(ctx, name, k, 1, 1, 1, 0, lb, 11)
    if name == "base2":    # 2 gate + 1 lookup-advice + 1 fixed + 1 instance column: the batched commitment path, instances absorbed
        return _base_case(ctx, name, k, 2, 1, 1, 1, lb, 12)
    if name == "dyn":      # dynamic lookup: key_cols 2, 2 sets
        _, dp, advice, fixed, copies = ram_circuit(k, 40, 16, 2, 2, seed=13)
        return Case(ctx, name, SO, dp, oracle_shape(dp), fixed, copies, advice, [], 13)
    if name == "phased":   # two phases [1, 1] / [1, 1] with one challenge
        params, inst = shape_params("a", k, lb)
        circ = PhasedCircuit(params, 14, instance=inst)
        return Case(ctx, name, SO, params, circ.sh, circ.fixed, circ.copies, circ.advice0(), circ.instances, 14, witness=circ.witness, num_challenges=1)
    if name == "rlc":      # RLC shape B
        params, inst = RC.shape_b(k, lb)
        circ = RC.RlcCircuit(params, 15, instance=inst)
        return Case(ctx, name, SO, params, circ.sh, circ.fixed, circ.copies, circ.advice0(), circ.instances, 15, witness=circ.witness, num_challenges=1)
    raise ValueError(name)


SHAPES = ["base1", "base2", "dyn", "phased", "rlc"]


class Cases:
    """the cases of one test module, each built on first use"""

    def __init__(self, ctx, k_of):
        self.ctx, self.k_of, self.made = ctx, k_of, {}

    def __call__(self, name):
        if name not in self.made:
            self.made[name] = make_case(self.ctx, name, self.k_of(name))
        return self.made[name]

    def free(self):
        for c in self.made.values():
            c.free()


# ------------------------------------------------------------------------------------------------ check 1
def check_t1_equals_builtin(case):
    """T1 through the callbacks gives the built-in entry's bytes from the same seeded RNG, and leaves the RNG at the same position"""
    lib = case.ctx.lib
    a, b = PL.ChaChaRng(lib, 5 + case.seed), PL.ChaChaRng(lib, 5 + case.seed)
    want = case.prove(rng=a)
    got = case.prove(rng=b, transcript=Blake2bWrite())
    assert got == want, "%s: T1 through the callbacks differs from the built-in entry" % case.name
    assert a.pos == b.pos and a.pos > 0
    # ... and from a host RNG behind a callback
    assert case.prove(transcript=Blake2bWrite()) == case.builtin()
    assert case.verify(transcript=Blake2bRead(want)) and case.verify(want)


# ------------------------------------------------------------------------------------------------ check 2
def check_t2_equals_python_prover(case, monkeypatch):
    """over T2 the library's bytes are the matching Python prover's; the patched Python verifier, and the library over T2's reader, accept them;
    the built-in verifier rejects them without an error"""
    got = case.t2_proof()
    assert got != case.builtin()
    monkeypatch.setattr(case.oracle, "Blake2bWrite", T2Write)
    monkeypatch.setattr(case.oracle, "Blake2bRead", T2Read)
    want = case.oracle_prove()
    assert got == want, "%s: proof bytes over T2 differ from the Python prover's" % case.name
    assert case.oracle_verify(got), "the patched Python verifier rejects the library's proof"
    assert case.verify(transcript=T2Read(got)), "h2hip_plonk_verify_proof_transcript rejects the proof"
    assert case.verify(got) is False, "the built-in verifier accepts T2 bytes"
    assert not case.verify(transcript=T2Read(got + bytes(32))), "trailing input went unnoticed"


# ------------------------------------------------------------------------------------------------ check 3
def _neg(pt):
    """-P for a (8,) uint64 Montgomery affine point"""
    y = sum(int(v) << (64 * i) for i, v in enumerate(pt[4:]))
    out = pt.copy()
    ny = (Q - y) % Q
    out[4:] = [(ny >> (64 * i)) & (2**64 - 1) for i in range(4)]
    return out


def check_accumulator(case):
    """acc_out = (W', outer) satisfies the pairing equation; for a T1 proof it is verify_batch's accumulator of that one proof with rho = 1"""
    ctx = case.ctx
    g2 = np.frombuffer(case.kzg.g2_raw, dtype=np.uint8).copy()
    for proof, reader in ((case.t2_proof(), T2Read), (case.builtin(), Blake2bRead)):
        ok, acc = case.verify(transcript=reader(proof), want_accumulator=True)
        assert ok and acc.any()
        g1s = np.ascontiguousarray(np.stack([acc[0], _neg(acc[1])]))
        g2s = np.concatenate([g2[128:256], g2[:128]])   # (W', s_g2), (-outer, g2)
        one = C.c_int(0)
        ctx._chk(ctx.lib.h2hip_pairing_check(g1s.ctypes.data_as(_vp), g2s.ctypes.data_as(_vp), 2, C.byref(one)))
        assert one.value == 1
    if case.name != "rlc":   # (h2hip_plonk_verify_batch refuses RLC keys)
        ok, _, bacc = PL.verify_batch(case.gpk, [case.inst], [case.builtin()], rng=PL.ArrayRng(fr([1])), want_acc=True)
        assert ok and np.array_equal(bacc, acc), "the accumulator differs from verify_batch's with rho = 1"
    # a malformed proof leaves the accumulator zeroed
    ok, acc = case.verify(transcript=T2Read(case.t2_proof()[:-1]), want_accumulator=True)
    assert not ok and not acc.any()


# ------------------------------------------------------------------------------------------------ check 4
class _BadRead(T2Read):
    """T2's reader that misbehaves at its n-th read (points and scalars counted together, from 1)"""

    def __init__(self, proof, n, what):
        super().__init__(proof)
        self.n, self.what, self.reads = n, what, 0

    def _bad(self):
        self.reads += 1
        return self.reads == self.n

    def read_point(self):
        if self._bad():
            if self.what == "fail":
                raise ValueError("the third read fails")
            x, y = super().read_point()
            return {"off_curve": (x, (y + 1) % Q), "identity": None, "x_not_canonical": (x + Q, y)}[self.what]
        return super().read_point()

    def read_scalar(self):
        if self._bad():
            super().read_scalar()
            return R + 1   # limbs >= r
        return super().read_scalar()


class _BadSqueeze:
    """wraps a transcript; its n-th squeeze returns limbs >= r"""

    def __init__(self, inner, n):
        self.inner, self.n, self.count = inner, n, 0
        for name in ("common_point", "common_scalar", "write_point", "write_scalar", "read_point", "read_scalar"):
            if hasattr(inner, name):
                setattr(self, name, getattr(inner, name))

    def squeeze_challenge(self):
        self.count += 1
        v = self.inner.squeeze_challenge()
        return R + 7 if self.count == self.n else v


def _invalid(fn, what):
    try:
        fn()
    except H.H2HipError as e:
        assert e.code == ERR_INVALID, (what, e.code, str(e))
        return str(e)
    raise AssertionError("%s was accepted" % what)


def check_rejections(case):
    proof = case.t2_proof()
    npts_tail = 2 * 64
    nevals = case.gpk.shape.num_evals
    head_points = (len(proof) - npts_tail - 32 * nevals) // 64
    assert 64 * head_points + 32 * nevals + npts_tail == len(proof)
    bad = bytearray(proof)
    bad[64 * head_points + 32 * (nevals // 2) + 31] ^= 1   # one evaluation
    assert case.verify(transcript=T2Read(bytes(bad))) is False
    for what in ("off_curve", "identity", "x_not_canonical"):
        assert case.verify(transcript=_BadRead(proof, 2, what)) is False, what
    assert case.verify(transcript=_BadRead(proof, head_points + 3, "scalar")) is False, "limbs >= r"
    r = _BadRead(proof, 3, "fail")
    assert case.verify(transcript=r) is False
    assert r.reads == 3, "a callback ran after the failed read"
    assert case.verify(transcript=T2Read(proof)) is True
    # a broken squeeze_challenge is the caller's error, for the verifier and the prover
    msg = _invalid(lambda: case.verify(transcript=_BadSqueeze(T2Read(proof), 2)), "verifier: squeeze_challenge >= r")
    assert "squeeze_challenge" in msg
    msg = _invalid(lambda: case.prove(transcript=_BadSqueeze(T2Write(), 2)), "prover: squeeze_challenge >= r")
    assert "squeeze_challenge #2" in msg
    assert case.prove() == case.builtin()


# ------------------------------------------------------------------------------------------------ check 5
class _Recording(Blake2bWrite):
    def __init__(self):
        super().__init__()
        self.ops = []

    def common_scalar(self, s):
        self.ops.append("common_scalar")
        super().common_scalar(s)

    def write_point(self, pt):
        self.ops.append("write_point")
        super().common_point(pt)
        self.proof += b"\0" * 32

    def write_scalar(self, s):
        self.ops.append("write_scalar")
        super().common_scalar(s)
        self.proof += b"\0" * 32

    def squeeze_challenge(self):
        self.ops.append("squeeze_challenge")
        return super().squeeze_challenge()


class _Boom(Exception):
    pass


class _FailAt(_Recording):
    """T1 that fails at its n-th call (all operations counted together, from 0)"""

    def __init__(self, n, exc=_Boom):
        super().__init__()
        self.n, self.exc = n, exc

    def _tick(self):
        if len(self.ops) == self.n:
            self.ops.append("failed")
            raise self.exc("call %d" % self.n)

    def common_scalar(self, s):
        self._tick()
        super().common_scalar(s)

    def write_point(self, pt):
        self._tick()
        super().write_point(pt)

    def write_scalar(self, s):
        self._tick()
        super().write_scalar(s)

    def squeeze_challenge(self):
        self._tick()
        return super().squeeze_challenge()


def raw_create_proof(case, transcript, rng):
    """h2hip_plonk_create_proof_transcript as a C caller sees it -> (return code, last error, the exceptions the callbacks raised)"""
    ctx, gpk = case.ctx, case.gpk
    n = 1 << case.params.k
    err = []
    keep = [np.ascontiguousarray(c, dtype=np.uint64) for c in case.advice]
    adv = (_vp * len(keep))(*[_vp(c.ctypes.data) for c in keep])
    ip = (_vp * max(len(case.inst), 1))(*[_vp(c.ctypes.data) for c in case.inst])
    il = (C.c_size_t * max(len(case.inst), 1))(*[len(c) for c in case.inst])
    wit = PL._phase_witness_trampoline(ctx, n, case.witness, err) if case.witness else None
    tr = PL._transcript_trampolines(transcript, err)

    def fill(_user, out, count):
        rng.fill_into(out, count)

    cb = PL._RNG_FN(fill)
    rc = ctx.lib.h2hip_plonk_create_proof_transcript(ctx.handle, gpk.handle, adv, 0, ip, il, C.cast(cb, _vp), None, C.byref(wit[0]) if wit else None,
                                                     C.byref(tr[0]), None)
    return rc, ctx.lib.h2hip_last_error().decode(), err


def abort_points(case):
    """{stretch: index of the call that fails}, one per stretch of the proof, from the operations of a complete proof"""
    rec = _Recording()
    case.prove(transcript=rec)
    ops = rec.ops
    nth = lambda op, j: [i for i, o in enumerate(ops) if o == op][j]
    nch = case.num_challenges
    pts = {"vk common_scalar": 0, "first-round write_point": nth("write_point", 0), "theta squeeze": nth("squeeze_challenge", nch),
           "h-piece write_point": nth("squeeze_challenge", nch + 3) + 1, "evaluation write_scalar": nth("write_scalar", 1),
           "last write_point": len(ops) - 1}
    if case.inst_ints and case.inst_ints[0]:
        pts["instance value"] = 1
    if nch:
        pts["between the phases"] = nth("squeeze_challenge", 0)
        pts["phase 1's first write_point"] = nth("squeeze_challenge", nch - 1) + 1
    assert ops[0] == "common_scalar" and ops[pts["h-piece write_point"]] == "write_point" and ops[-1] == "write_point"
    assert ops[pts["theta squeeze"] + 1] == "write_point" and ops[nth("squeeze_challenge", nch + 3) - 1] == "write_point"
    return ops, pts


def check_aborts(case):
    """a transcript that fails at its n-th call, one n in every stretch: H2HIP_ERR_INVALID naming the operation and its ordinal, and the built-in
    entry on the same key and context reproduces its bytes afterwards"""
    before = case.builtin()
    ops, pts = abort_points(case)
    for stretch, n in pts.items():
        t = _FailAt(n)
        rc, msg, err = raw_create_proof(case, t, case.rng())
        op = ops[n]
        ordinal = ops[: n + 1].count(op)
        assert rc == ERR_INVALID, (stretch, rc, msg)
        assert "%s #%d " % (op, ordinal) in msg, (stretch, msg)
        assert len(err) == 1 and isinstance(err[0], _Boom) and t.ops[-1] == "failed" and len(t.ops) == n + 1, (stretch, "a callback ran after the failure")
        assert case.prove() == before, "%s: the key or the context did not survive an abort at the %s" % (case.name, stretch)
    # through the Python mirror the callback's own exception comes back
    try:
        case.prove(transcript=_FailAt(pts["first-round write_point"], exc=KeyError))
    except KeyError:
        pass
    else:
        raise AssertionError("the callback's exception was not re-raised")
    assert case.prove() == before
    assert case.prove(transcript=Blake2bWrite()) == before


def check_refusals(case):
    """missing callbacks and a sharded key are refused before anything is drawn or launched"""
    ctx, lib = case.ctx, case.ctx.lib
    before = case.builtin()
    full = Blake2bWrite()
    for missing in ("common_scalar", "write_point", "write_scalar", "squeeze_challenge"):
        class Partial:
            pass

        t = Partial()
        for name in ("common_scalar", "write_point", "write_scalar", "squeeze_challenge"):
            if name != missing:
                setattr(t, name, getattr(full, name))
        rng = PL.ChaChaRng(lib, 3)
        _invalid(lambda: case.prove(rng=rng, transcript=t), "a transcript without " + missing)
        assert rng.pos == 0 and not full.proof, missing
    proof = case.builtin()
    for missing in ("common_scalar", "read_point", "read_scalar", "squeeze_challenge"):
        class PartialR:
            pass

        t, r = PartialR(), Blake2bRead(proof)
        for name in ("common_scalar", "read_point", "read_scalar", "squeeze_challenge"):
            if name != missing:
                setattr(t, name, getattr(r, name))
        _invalid(lambda: case.verify(transcript=t), "a reader without " + missing)
        assert r.pos == 0
    if case.oracle is not P:   # (only BaseConfig keys can be sharded)
        return
    # a sharded key: the callback transport with a world of one, forced onto the sharded path
    def _allgather(_user, local, nbytes, out):
        C.memmove(out, local, nbytes)
        return 0

    cb = C.CFUNCTYPE(C.c_int, _vp, _vp, C.c_size_t, _vp)(_allgather)
    comm = _vp()
    ctx._chk(lib.h2hip_comm_init_callback(1, 0, C.cast(cb, _vp), None, C.byref(comm)))
    try:
        n = 1 << case.params.k
        ctx._chk(lib.h2hip_plonk_pk_set_sharding(case.gpk.handle, comm, case.kzg.g.handle, case.kzg.g_lagrange.handle, 0, n, 2))   # H2HIP_SHARD_FORCE
        rng = PL.ChaChaRng(lib, 3)
        msg = _invalid(lambda: case.prove(rng=rng, transcript=Blake2bWrite()), "a sharded key")
        assert "sharded" in msg and rng.pos == 0
    finally:
        ctx._chk(lib.h2hip_plonk_pk_set_sharding(case.gpk.handle, None, None, None, 0, 0, 0))
        lib.h2hip_comm_destroy(comm)
    assert case.prove() == before
    assert case.prove(transcript=Blake2bWrite()) == before


# ------------------------------------------------------------------------------------------------ check 6 (GPU)
def check_schedule_switches(ctx):
    """BaseConfig k = 12, 3 gate + 1 lookup-advice columns, device ChaCha RNG: T1 through the callbacks gives the built-in bytes with each of the
    schedule switches off and on, from host and from device advice"""
    k = 12
    case = _base_case(ctx, "switches", k, 3, 1, 1, 0, k - 2, 21)
    names = ("plonk_tail_overlap", "plonk_permute_in_commit", "plonk_lazy_upload")
    old = {n: ctx.get_param(n) for n in names}
    d_adv = [ctx.to_device(np.ascontiguousarray(c)) for c in case.advice]
    try:
        ref = None
        for name in names:
            for v in (0, 1):
                for n_, o in old.items():
                    ctx.set_param(n_, o)
                ctx.set_param(name, v)
                for on_device in (False, True):
                    adv = d_adv if on_device else None
                    a, b = PL.ChaChaRng(ctx.lib, 9), PL.ChaChaRng(ctx.lib, 9)
                    want = case.prove(rng=a, advice=adv, advice_on_device=on_device)
                    got = case.prove(rng=b, transcript=Blake2bWrite(), advice=adv, advice_on_device=on_device)
                    assert got == want and a.pos == b.pos, (name, v, on_device)
                    ref = ref or want
                    assert want == ref, (name, v, on_device)
        assert case.verify(ref)
    finally:
        for n_, o in old.items():
            ctx.set_param(n_, o)
        for p in d_adv:
            ctx.free(p)
        case.free()


# ------------------------------------------------------------------------------------------------ check 8
def check_struct_layout():
    """h2hip_transcript and its callback types: the same fields, order and classes in the header, the Rust sys crate and ctypes"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "h2hip.h")).read()
    rs = open(os.path.join(root, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    body = re.search(r"typedef struct h2hip_transcript\s*\{(.*?)\}\s*h2hip_transcript\s*;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            if ty == "void":   # void *user
                c_fields.append((names.replace("*", "").strip(), "void*"))
            else:
                c_fields += [(nm.strip(), ty) for nm in names.split(",")]
    want = [("user", "void*"), ("common_point", "h2hip_transcript_point_fn"), ("write_point", "h2hip_transcript_point_fn"),
            ("common_scalar", "h2hip_transcript_scalar_fn"), ("write_scalar", "h2hip_transcript_scalar_fn"),
            ("read_point", "h2hip_transcript_read_fn"), ("read_scalar", "h2hip_transcript_read_fn"), ("squeeze_challenge", "h2hip_transcript_read_fn")]
    assert c_fields == want, c_fields
    rs_body = re.search(r"#\[repr\(C\)\](?:\s*#\[[^\]]*\])*\s*pub struct h2hip_transcript\s*\{(.*?)\}", rs, flags=re.S).group(1)
    rs_fields = [(m.group(1), m.group(2).strip()) for m in re.finditer(r"pub ([a-z_]+): ([^,\n]+),", rs_body)]
    assert rs_fields == [(n, "*mut c_void" if t == "void*" else t) for n, t in want], rs_fields
    assert [n for n, _ in PL._Transcript._fields_] == [n for n, _ in want] and all(t is _vp for _, t in PL._Transcript._fields_)
    # the callback types: (user, in) -> int for points and scalars, (user, out) -> int for reads, in all three places
    for name, arg in (("point", r"const void \*g1_affine"), ("scalar", r"const void \*fr"), ("read", r"void \*out")):
        assert re.search(r"typedef int \(\*h2hip_transcript_%s_fn\)\(void \*user, %s\);" % (name, arg), hdr), name
    for name, arg in (("point", "g1_affine: *const c_void"), ("scalar", "fr: *const c_void"), ("read", "out: *mut c_void")):
        assert 'pub type h2hip_transcript_%s_fn = Option<unsafe extern "C" fn(user: *mut c_void, %s) -> c_int>;' % (name, arg) in rs, name
    for proto in (PL._TR_IN_FN, PL._TR_OUT_FN):
        assert proto._restype_ is C.c_int and tuple(proto._argtypes_) == (_vp, _vp)
    assert re.search(r"#define H2HIP_CIRCUIT_RLC 3\b", hdr) and "pub const H2HIP_CIRCUIT_RLC: c_int = 3;" in rs and PL._CIRCUIT_RLC == 3
