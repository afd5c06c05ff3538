"""
Host-side mirror of `halo2_proofs::plonk::{keygen_vk, keygen_pk, create_proof}` for halo2-base circuits, over libh2hip's
prover entry points (include/h2hip.h, "a1").  The reference reaches these names at

    halo2-base/src/utils/testing.rs:224-227   keygen_vk / keygen_pk
    halo2-base/src/utils/testing.rs:32-50     create_proof::<KZGCommitmentScheme<Bn256>, ProverSHPLONK<_>, Challenge255<_>, _,
                                              Blake2bWrite<_, _, _>, _>(params, pk, &[circuit], &[instances], rng, &mut transcript)

The circuit here is what the reference's `BaseCircuitBuilder` hands to the prover after synthesis: its BaseCircuitParams
(halo2-base/src/gates/circuit/mod.rs:25-45), the fixed columns, the copy constraints and the advice columns produced by
`assign_witnesses` (halo2-base/src/gates/flex_gate/threads/single_phase.rs:273-312).  The whole proof is computed on the GPU by
libh2hip; this module only marshals pointers.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import hashlib
from typing import Callable, NamedTuple, Optional, Sequence

import numpy as np

from .h2hip import WITNESS_COPY, WITNESS_GATE, WITNESS_LOOKUP, Context, H2HipError, WitnessFailureStruct, _fe, _ptr, load_library
from .halo2_proofs import ParamsKZG, R_MOD, fr_int, fr_limbs

_vp = C.c_void_p
PLONK_STAGES = 12


class BaseCircuitParams(C.Structure):
    """BaseCircuitParams, first phase (gates/circuit/mod.rs:25-45); lookup_bits < 0 means None"""
    _fields_ = [("k", C.c_uint32), ("num_advice", C.c_uint32), ("num_lookup_advice", C.c_uint32), ("num_fixed", C.c_uint32),
                ("num_instance", C.c_uint32), ("lookup_bits", C.c_int32)]

    @classmethod
    def new(cls, k, num_advice, num_lookup_advice, num_fixed, num_instance=0, lookup_bits: Optional[int] = None):
        return cls(k, num_advice, num_lookup_advice, num_fixed, num_instance, -1 if lookup_bits is None else lookup_bits)


class DynLookupCircuitParams(C.Structure):
    """h2hip_dyn_circuit_params: BasicDynLookupConfig::<key_cols>::new(meta, || FirstPhase, lu_sets) followed by FlexGateConfig::configure
    (halo2-base/src/virtual_region/lookups/basic.rs:52-78, the RAMCircuit of virtual_region/tests/lookups/memory.rs:92-98)"""
    _fields_ = [("k", C.c_uint32), ("num_advice", C.c_uint32), ("num_fixed", C.c_uint32), ("key_cols", C.c_uint32), ("lu_sets", C.c_uint32)]
    num_instance = 0   # the configuration has no instance columns

    @classmethod
    def new(cls, k, num_advice, num_fixed, key_cols, lu_sets):
        return cls(k, num_advice, num_fixed, key_cols, lu_sets)


class PhasedCircuitParams(C.Structure):
    """h2hip_phased_circuit_params: BaseCircuitParams with num_advice_per_phase / num_lookup_advice_per_phase of up to MAX_PHASE = 3 entries
    (gates/flex_gate/mod.rs:28,121-137, gates/range/mod.rs:87-108) and the challenges the circuit declares after each phase
    (meta.challenge_usable_after(phase)); lookup_bits < 0 means None.  One used phase and no challenge is the BaseConfig of that phase."""
    _fields_ = [("k", C.c_uint32), ("num_advice_per_phase", C.c_uint32 * 3), ("num_lookup_advice_per_phase", C.c_uint32 * 3), ("num_fixed", C.c_uint32),
                ("num_instance", C.c_uint32), ("lookup_bits", C.c_int32), ("num_challenges_per_phase", C.c_uint32 * 3)]

    @classmethod
    def new(cls, k, num_advice_per_phase, num_lookup_advice_per_phase, num_fixed, num_instance=0, lookup_bits: Optional[int] = None,
            num_challenges_per_phase=()):
        pad = lambda v: (C.c_uint32 * 3)(*(list(v) + [0] * (3 - len(v))))
        return cls(k, pad(num_advice_per_phase), pad(num_lookup_advice_per_phase), num_fixed, num_instance, -1 if lookup_bits is None else lookup_bits,
                   pad(num_challenges_per_phase))

    def phase_columns(self) -> list:
        """the advice columns of each phase, index order (gate columns of every phase, then the dedicated lookup-advice columns of every phase);
        trailing phases without columns are dropped"""
        g, la = list(self.num_advice_per_phase), list(self.num_lookup_advice_per_phase)
        rng = self.lookup_bits >= 0 and sum(la) != 0
        q = rng and g[0] == 1 and la[0] != 0
        ded = [0 if (not rng or (p == 0 and q)) else la[p] for p in range(3)]
        out, go, lo = [], 0, sum(g)
        for p in range(3):
            out.append(list(range(go, go + g[p])) + list(range(lo, lo + ded[p])))
            go, lo = go + g[p], lo + ded[p]
        while len(out) > 1 and not out[-1]:
            out.pop()
        return out

    def base_params(self) -> Optional[BaseCircuitParams]:
        """the BaseCircuitParams this is, if it has one used phase and no challenge"""
        if len(self.phase_columns()) != 1 or any(self.num_challenges_per_phase):
            return None
        return BaseCircuitParams(self.k, self.num_advice_per_phase[0], self.num_lookup_advice_per_phase[0], self.num_fixed, self.num_instance,
                                 self.lookup_bits)


class RlcCircuitParams(C.Structure):
    """h2hip_rlc_circuit_params: BaseConfig::configure(base) followed by num_rlc_advice RLC columns (downstream's RlcConfig): phase-1 advice
    columns behind every column of `base`, one selector q_rlc each, the gate q_rlc * (a[r] * gamma + a[r+1] - a[r+2]) with gamma = challenge 0.
    include/h2hip.h states the layout."""
    _fields_ = [("base", PhasedCircuitParams), ("num_rlc_advice", C.c_uint32)]

    @classmethod
    def new(cls, k, num_advice_per_phase, num_lookup_advice_per_phase, num_fixed, num_instance=0, lookup_bits: Optional[int] = None,
            num_challenges_per_phase=(1,), num_rlc_advice=1):
        return cls(PhasedCircuitParams.new(k, num_advice_per_phase, num_lookup_advice_per_phase, num_fixed, num_instance, lookup_bits,
                                           num_challenges_per_phase), num_rlc_advice)

    k = property(lambda self: self.base.k)
    num_fixed = property(lambda self: self.base.num_fixed)
    num_instance = property(lambda self: self.base.num_instance)
    lookup_bits = property(lambda self: self.base.lookup_bits)

    def rlc_columns(self) -> list:
        """the advice indices of the RLC columns (the last ones)"""
        first = sum(len(c) for c in self.base.phase_columns())
        return list(range(first, first + self.num_rlc_advice))

    def phase_columns(self) -> list:
        """base's phases with the RLC columns at the end of phase 1"""
        out = self.base.phase_columns()
        while len(out) < 2:
            out.append([])
        out[1] = out[1] + self.rlc_columns()
        return out


class ConstraintSystemShape(C.Structure):
    """what BaseConfig::configure derives from the params (h2hip_plonk_shape)"""
    _fields_ = [("num_advice_total", C.c_uint32), ("num_fixed_total", C.c_uint32), ("table_col", C.c_int32), ("first_constant_col", C.c_int32),
                ("q_lookup_col", C.c_int32), ("first_q_enable_col", C.c_int32), ("num_lookups", C.c_uint32), ("num_perm_columns", C.c_uint32),
                ("num_perm_sets", C.c_uint32), ("degree", C.c_uint32), ("extended_k", C.c_uint32), ("blinding_factors", C.c_uint32),
                ("usable_rows", C.c_uint32), ("quotient_pieces", C.c_uint32), ("num_commitments", C.c_uint32), ("num_evals", C.c_uint32)]


class _Kind(NamedTuple):
    """what differs between the circuit kinds on the way into libh2hip"""
    id: int                   # H2HIP_CIRCUIT_*
    shape_of: str             # the per-kind entries' names
    keygen: str
    verify_proof: str
    phased: bool              # the advice is committed phase by phase: create_proof takes phase 0's columns and a phase_witness
    verify_instances: bool    # the verify entry takes instance columns
    batched: bool             # h2hip_plonk_verify_batch serves the kind


_KIND_OF = {
    BaseCircuitParams: _Kind(0, "h2hip_plonk_shape_of", "h2hip_plonk_keygen", "h2hip_plonk_verify_proof", False, True, True),
    DynLookupCircuitParams: _Kind(1, "h2hip_plonk_shape_of_dyn", "h2hip_plonk_keygen_dyn", "h2hip_plonk_verify_proof_dyn", False, False, True),
    PhasedCircuitParams: _Kind(2, "h2hip_plonk_shape_of_phased", "h2hip_plonk_keygen_phased", "h2hip_plonk_verify_proof_phased", True, True, True),
    RlcCircuitParams: _Kind(3, "h2hip_plonk_shape_of_rlc", "h2hip_plonk_keygen_rlc", "h2hip_plonk_verify_proof_rlc", True, True, False),
}
_CIRCUIT_KINDS = {t: k.id for t, k in _KIND_OF.items() if k.batched}   # the kinds h2hip_plonk_verify_batch takes (RLC keys: not batched)
_CIRCUIT_RLC = _KIND_OF[RlcCircuitParams].id   # H2HIP_CIRCUIT_RLC: h2hip_plonk_verify_proof_transcript only


def shape_of(ctx: Context, params) -> ConstraintSystemShape:
    out = ConstraintSystemShape()
    ctx._chk(getattr(ctx.lib, _KIND_OF[type(params)].shape_of)(C.byref(params), C.byref(out)))
    return out


def describe(params) -> str:
    """the key description transcript_repr hashes (one per configuration)"""
    if isinstance(params, RlcCircuitParams):
        b = params.base
        return "halo2-lib_amd BaseConfig+RlcConfig k=%d advice=%s lookup_advice=%s fixed=%d instance=%d lookup_bits=%s challenges=%s rlc_advice=%d" % (
            b.k, list(b.num_advice_per_phase), list(b.num_lookup_advice_per_phase), b.num_fixed, b.num_instance,
            None if b.lookup_bits < 0 else b.lookup_bits, list(b.num_challenges_per_phase), params.num_rlc_advice)
    if isinstance(params, PhasedCircuitParams):
        if params.base_params() is not None:   # one phase, no challenge: the BaseConfig key, the same transcript_repr
            return describe(params.base_params())
        return "halo2-lib_amd BaseConfig k=%d advice=%s lookup_advice=%s fixed=%d instance=%d lookup_bits=%s challenges=%s" % (
            params.k, list(params.num_advice_per_phase), list(params.num_lookup_advice_per_phase), params.num_fixed, params.num_instance,
            None if params.lookup_bits < 0 else params.lookup_bits, list(params.num_challenges_per_phase))
    if isinstance(params, DynLookupCircuitParams):
        return "halo2-lib_amd BasicDynLookupConfig k=%d advice=%d fixed=%d key_cols=%d lu_sets=%d" % (
            params.k, params.num_advice, params.num_fixed, params.key_cols, params.lu_sets)
    return "halo2-lib_amd BaseConfig k=%d advice=%d lookup_advice=%d fixed=%d instance=%d lookup_bits=%s" % (
        params.k, params.num_advice, params.num_lookup_advice, params.num_fixed, params.num_instance,
        None if params.lookup_bits < 0 else params.lookup_bits)


def transcript_repr(params: BaseCircuitParams | DynLookupCircuitParams, fixed_commitments: np.ndarray, permutation_commitments: np.ndarray) -> int:
    """Stand-in for VerifyingKey::transcript_repr.  Upstream hashes the Rust Debug rendering of the pinned verifying key with
    Blake2b-512("Halo2-Verify-Key"); that rendering belongs to the Rust side of the FFI (the shim passes the value in).  Without Rust
    the same construction is applied to an equivalent description of the key."""
    h = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
    s = describe(params).encode()
    h.update(len(s).to_bytes(8, "little") + s)
    q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
    rinv = pow(1 << 256, -1, q)
    for pts in (fixed_commitments, permutation_commitments):
        for row in np.asarray(pts, dtype=np.uint64).reshape(-1, 8).tolist():
            x = sum(v << (64 * i) for i, v in enumerate(row[:4])) * rinv % q
            y = sum(v << (64 * i) for i, v in enumerate(row[4:])) * rinv % q
            h.update(x.to_bytes(32, "little") + y.to_bytes(32, "little"))     # the identity (0, 0) hashes as 64 zero bytes
    return int.from_bytes(h.digest(), "little") % R_MOD


_RNG_FN = C.CFUNCTYPE(None, _vp, _vp, C.c_size_t)
_PHASE_FN = C.CFUNCTYPE(C.c_int, _vp, C.c_uint32, _vp, C.c_size_t, C.POINTER(_vp), C.c_size_t)   # h2hip_phase_witness_fn


class _PhaseWitness(C.Structure):   # h2hip_phase_witness
    _fields_ = [("fill", _vp), ("user", _vp)]


_TR_IN_FN = C.CFUNCTYPE(C.c_int, _vp, _vp)    # h2hip_transcript_point_fn / h2hip_transcript_scalar_fn
_TR_OUT_FN = C.CFUNCTYPE(C.c_int, _vp, _vp)   # h2hip_transcript_read_fn


class _Transcript(C.Structure):   # h2hip_transcript
    _fields_ = [("user", _vp), ("common_point", _vp), ("write_point", _vp), ("common_scalar", _vp), ("write_scalar", _vp), ("read_point", _vp),
                ("read_scalar", _vp), ("squeeze_challenge", _vp)]


Q_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
_MONT = 1 << 256


def _mont_in(ptr, mod) -> int:
    """the integer behind 4 Montgomery limbs at ptr"""
    v = int.from_bytes(C.string_at(ptr, 32), "little")
    return v * pow(_MONT, -1, mod) % mod


def _mont_out(ptr, v: int, mod):
    """v (an int in [0, mod)) as 4 Montgomery limbs at ptr; anything else is written as it stands, for the library to refuse"""
    raw = int(v) * _MONT % mod if 0 <= int(v) < mod else int(v) & (_MONT - 1)
    C.memmove(ptr, raw.to_bytes(32, "little"), 32)


def _transcript_trampolines(obj, err: list):
    """(h2hip_transcript, the callback objects to keep alive) over a Python transcript: an object with some of common_point / write_point((x, y)),
    common_scalar / write_scalar(int), read_point() -> (x, y), read_scalar() -> int, squeeze_challenge() -> int, as oracle/transcript.py's
    classes have them.  A method the object lacks stays NULL.  An exception inside a method makes the callback return 1; it is kept in err."""
    q_inv, r_inv = pow(_MONT, -1, Q_MOD), pow(_MONT, -1, R_MOD)

    def guard(fn):
        def run(_user, ptr):
            try:
                fn(ptr)
                return 0
            except BaseException as e:   # never unwind through the C frames
                err.append(e)
                return 1
        return run

    def point_in(method):
        def fn(ptr):
            b = C.string_at(ptr, 64)
            method((int.from_bytes(b[:32], "little") * q_inv % Q_MOD, int.from_bytes(b[32:], "little") * q_inv % Q_MOD))
        return fn

    def scalar_in(method):
        return lambda ptr: method(int.from_bytes(C.string_at(ptr, 32), "little") * r_inv % R_MOD)

    def point_out(method):
        def fn(ptr):
            P = method()
            if P is None:   # the identity: all-zero, which the library rejects
                C.memset(ptr, 0, 64)
                return
            _mont_out(ptr, P[0], Q_MOD)
            _mont_out(ptr + 32, P[1], Q_MOD)
        return fn

    def scalar_out(method):
        return lambda ptr: _mont_out(ptr, method(), R_MOD)

    wrap = {"common_point": (_TR_IN_FN, point_in), "write_point": (_TR_IN_FN, point_in), "common_scalar": (_TR_IN_FN, scalar_in),
            "write_scalar": (_TR_IN_FN, scalar_in), "read_point": (_TR_OUT_FN, point_out), "read_scalar": (_TR_OUT_FN, scalar_out),
            "squeeze_challenge": (_TR_OUT_FN, scalar_out)}
    t, keep = _Transcript(), []
    for name, (proto, make) in wrap.items():
        method = getattr(obj, name, None)
        if method is not None:
            cb = proto(guard(make(method)))
            keep.append(cb)
            setattr(t, name, C.cast(cb, _vp))
    return t, keep


class _ArrayRngState(C.Structure):   # h2hip_array_rng
    _fields_ = [("values", _vp), ("count", C.c_size_t), ("pos", C.c_size_t), ("exhausted", C.c_int)]


class ArrayRng:
    """`Fr::random(rng)` stream served from a pre-drawn (m, 4) Montgomery array (the RNG itself stays with the caller: upstream draws
    from the `StdRng` the reference seeds at halo2-base/src/utils/testing.rs:38)."""

    def __init__(self, values: np.ndarray):
        self.values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        self.pos = 0

    def fill_into(self, dst: int, n: int):
        if self.pos + n > len(self.values):
            raise RuntimeError("ArrayRng exhausted")
        C.memmove(dst, self.values.ctypes.data + 32 * self.pos, 32 * n)
        self.pos += n


class _ChaChaRngState(C.Structure):   # h2hip_chacha_rng
    _fields_ = [("seed", C.c_uint8 * 32), ("rounds", C.c_int32), ("pos", C.c_uint64)]


class ChaChaRng:
    """The `Fr::random(&mut rng)` stream of a seeded rand_chacha generator — what the reference hands to create_proof
    (halo2-base/src/utils/testing.rs:38: `StdRng::seed_from_u64(0)`, rand 0.8's StdRng = ChaCha12).  libh2hip's own generator
    (csrc/rng.hip): create_proof produces its large draws ON THE DEVICE from (seed, position); `device=False` forces every draw through the
    one-thread host generator behind a Python callback (same values, same bytes: the A/B the bench line and the tests use).
    seed: 32 bytes, or an int for `seed_from_u64`."""

    def __init__(self, lib, seed=0, rounds: int = 12, device: bool = True):
        self.lib, self.device = lib, device
        if isinstance(seed, int):
            buf = (C.c_uint8 * 32)()
            lib.h2hip_rng_seed_from_u64(C.c_uint64(seed), buf)
            seed = bytes(buf)
        if len(seed) != 32:
            raise ValueError("ChaChaRng: the seed has 32 bytes")
        self.state = _ChaChaRngState()
        lib.h2hip_chacha_rng_init(C.byref(self.state), (C.c_uint8 * 32)(*seed), rounds)

    @property
    def pos(self) -> int:
        return int(self.state.pos)

    def fill_into(self, dst: int, n: int):
        self.lib.h2hip_chacha_rng_fill(C.byref(self.state), _vp(dst), n)

    def fill(self, n: int) -> np.ndarray:
        out = np.empty((n, 4), dtype=np.uint64)
        self.fill_into(out.ctypes.data, n)
        return out


class CallbackRng:
    """adapts any object with fill(n) -> (n, 4) uint64 Montgomery array"""

    def __init__(self, src):
        self.src = src

    def fill_into(self, dst: int, n: int):
        a = np.ascontiguousarray(self.src.fill(n), dtype=np.uint64).reshape(n, 4)
        C.memmove(dst, a.ctypes.data, 32 * n)


class ProvingKey:
    """ProvingKey<G1Affine> resident on the GPU: fixed / permutation polynomials in Lagrange, coefficient and extended form, l_0 /
    l_last / l_blind, and the verifying key's commitments."""

    def __init__(self, ctx: Context, handle, params: BaseCircuitParams, shape: ConstraintSystemShape, kzg: ParamsKZG):
        self.ctx, self.handle, self.params, self.shape, self.kzg = ctx, handle, params, shape, kzg
        fc = np.zeros((shape.num_fixed_total, 8), dtype=np.uint64)
        pc = np.zeros((max(shape.num_perm_columns, 1), 8), dtype=np.uint64)
        ctx._chk(ctx.lib.h2hip_plonk_pk_commitments(handle, _ptr(fc), _ptr(pc)))
        self.fixed_commitments, self.permutation_commitments = fc, pc[: shape.num_perm_columns]
        self.set_transcript_repr(transcript_repr(params, self.fixed_commitments, self.permutation_commitments))

    def set_transcript_repr(self, value: int):
        self.transcript_repr = value % R_MOD
        self.ctx._chk(self.ctx.lib.h2hip_plonk_pk_set_transcript_repr(self.handle, _ptr(fr_limbs(self.transcript_repr))))

    def proof_size(self) -> int:
        return 32 * (self.shape.num_commitments + self.shape.num_evals)

    def free(self):
        if self.handle:
            self.ctx.lib.h2hip_plonk_pk_free(self.ctx.handle, self.handle)
            self.handle = None


def perm_column_index(params, shape: ConstraintSystemShape, kind: str, index: int) -> int:
    """position of a column among the equality-enabled columns: constants, gate advice, lookup advice, instance (BaseConfig); the table and
    key columns, constants, gate advice (DynLookupCircuitParams)"""
    if isinstance(params, DynLookupCircuitParams):
        ndyn = params.key_cols * (1 + params.lu_sets)
        if kind == "fixed":
            return ndyn + index - shape.first_constant_col
        if kind == "advice":
            return index if index < ndyn else ndyn + params.num_fixed + index - ndyn
        raise ValueError(kind)
    if isinstance(params, RlcCircuitParams):   # constants, gate advice, lookup advice, instance, then the RLC columns
        first_rlc = shape.num_advice_total - params.num_rlc_advice
        if kind == "advice" and index >= first_rlc:
            return params.num_fixed + index + params.num_instance
        if kind == "instance":
            return params.num_fixed + first_rlc + index
    if kind == "fixed":
        return index - shape.first_constant_col
    if kind == "advice":   # (PhasedCircuitParams: advice indices run over every phase's gate columns, then the lookup-advice columns)
        return params.num_fixed + index
    if kind == "instance":
        return params.num_fixed + shape.num_advice_total + index
    raise ValueError(kind)


def keygen(kzg: ParamsKZG, params, fixed: Sequence[np.ndarray], copies) -> ProvingKey:
    """keygen_vk + keygen_pk.  fixed: num_fixed_total (n,4) Lagrange columns; copies: (m,4) uint32 (column, row, column, row) over the
    permutation columns, or a list of (((kind, column), row), ((kind, column), row)) in the order the circuit emitted them."""
    ctx = kzg.ctx
    shape = shape_of(ctx, params)
    n = 1 << params.k
    cols = [_fe(c) for c in fixed]
    if len(cols) != shape.num_fixed_total or any(len(c) != n for c in cols):
        raise ValueError("keygen: need %d fixed columns of 2^k elements" % shape.num_fixed_total)
    if not isinstance(copies, np.ndarray):
        copies = np.array([[perm_column_index(params, shape, l[0][0], l[0][1]), l[1], perm_column_index(params, shape, r[0][0], r[0][1]), r[1]]
                           for l, r in copies], dtype=np.uint32).reshape(-1, 4)
    copies = np.ascontiguousarray(copies, dtype=np.uint32).reshape(-1, 4)
    arr = (_vp * len(cols))(*[_vp(c.ctypes.data) for c in cols])
    out = _vp()
    fn = getattr(ctx.lib, _KIND_OF[type(params)].keygen)
    ctx._chk(fn(ctx.handle, C.byref(params), kzg.g.handle, kzg.g_lagrange.handle, arr, _vp(copies.ctypes.data), len(copies), C.byref(out)))
    return ProvingKey(ctx, out, params, shape, kzg)


# ---- argument groups several entries share: (the arguments, the arrays they point into)
def _advice_args(who: str, advice: Sequence, n: int, on_device: bool):
    """the advice column pointer array over host (n,4) arrays or device pointers"""
    if on_device:
        return (_vp * len(advice))(*[_vp(int(p)) for p in advice]), None
    keep = [_fe(c) for c in advice]
    if any(len(c) != n for c in keep):
        raise ValueError("%s: advice columns must have 2^k elements" % who)
    return (_vp * len(keep))(*[_vp(c.ctypes.data) for c in keep]), keep


def _column_arrays(cols: Sequence[np.ndarray]):
    """the pointer and length arrays over host columns"""
    return (_vp * max(len(cols), 1))(*[_vp(c.ctypes.data) for c in cols]), (C.c_size_t * max(len(cols), 1))(*[len(c) for c in cols])


def _instance_args(who: str, params, instances: Sequence[np.ndarray]):
    inst = [_fe(c) for c in instances]
    if len(inst) != params.num_instance:
        raise ValueError("%s: need %d instance columns" % (who, params.num_instance))
    return _column_arrays(inst), inst


def _vk_args(who: str, pk: ProvingKey):
    """the verifying key as the verify entries take it: fixed and permutation commitments, transcript_repr, g[0], g2, s_g2"""
    ctx, kzg = pk.ctx, pk.kzg
    if len(kzg.g2_raw) != 256:
        raise ValueError("%s: the ParamsKZG carries no G2 elements (g2_raw)" % who)
    if not hasattr(kzg, "_g0"):
        kzg._g0 = ctx.bases_download(kzg.g)[:1].copy()
    g2 = np.frombuffer(kzg.g2_raw, dtype=np.uint8).copy()
    pc = pk.permutation_commitments if len(pk.permutation_commitments) else np.zeros((1, 8), dtype=np.uint64)
    keep = [np.ascontiguousarray(pk.fixed_commitments), np.ascontiguousarray(pc), fr_limbs(pk.transcript_repr), kzg._g0, g2]
    return tuple(_ptr(a) for a in keep[:4]) + (_vp(g2.ctypes.data), _vp(g2.ctypes.data + 128)), keep


def create_proof(pk: ProvingKey, advice: Sequence, instances: Sequence[np.ndarray], rng, timings: Optional[dict] = None,
                 advice_on_device: bool = False, phase_witness=None, phase_witness_dev=None, transcript=None) -> bytes:
    """create_proof for one circuit: advice columns (host (n,4) arrays, or device pointers with advice_on_device), instance columns
    ((m,4) arrays), rng = ArrayRng / ChaChaRng / CallbackRng.  Returns the proof bytes (Blake2bWrite::finalize).
    A PhasedCircuitParams key takes phase 0's columns in `advice`; phase_witness(phase, challenges: list[int]) -> list returns each later
    phase's columns (host (n,4) arrays or device pointers to n Fr) given every challenge squeezed so far.  An RlcCircuitParams key likewise;
    its phase-1 column list ends with the RLC columns.  phase_witness_dev(phase, challenges: list[int], column_ptrs: list[int]) instead writes
    the phase's zeroed device columns in place (rlc_fill_chains, `_dev` functions on the key's context, completed device copies).
    transcript: the caller's transcript object (h2hip_plonk_create_proof_transcript) with common_scalar(int), write_point((x, y)),
    write_scalar(int) and squeeze_challenge() -> int, as oracle/transcript.py's Blake2bWrite has them; its methods run while the proof is in
    flight and must not use pk's context.  The proof's bytes are then the transcript's: the call returns transcript.finalize() if the object
    has it, else None.  An exception raised inside a method aborts the proof and is re-raised here."""
    ctx, sh = pk.ctx, pk.shape
    n = 1 << pk.params.k
    phased = _KIND_OF[type(pk.params)].phased
    if phase_witness is not None and phase_witness_dev is not None:
        raise ValueError("create_proof: give phase_witness or phase_witness_dev, not both")
    want = len(pk.params.phase_columns()[0]) if phased else sh.num_advice_total
    if len(advice) != want:
        raise ValueError("create_proof: need %d advice columns" % want)
    adv, keep = _advice_args("create_proof", advice, n, advice_on_device)
    (ip, il), inst = _instance_args("create_proof", pk.params, instances)
    err = []

    def _fill(_user, out, count):
        try:
            rng.fill_into(out, count)
        except BaseException as e:   # never unwind through the C frames
            err.append(e)
            C.memset(out, 0, 32 * count)

    proof = np.zeros(pk.proof_size(), dtype=np.uint8)
    plen = C.c_size_t(0)
    stage = (C.c_double * PLONK_STAGES)() if timings is not None else None
    if phased:
        wit = _phase_witness_trampoline(ctx, n, phase_witness, err, phase_witness_dev)
    if transcript is not None:   # one entry for every kind of key; it returns no bytes
        tr = _transcript_trampolines(transcript, err)
        entry = lambda *a: ctx.lib.h2hip_plonk_create_proof_transcript(*a[:8], C.byref(wit[0]) if phased else None, C.byref(tr[0]), a[11])
    elif phased:
        entry = lambda *a: ctx.lib.h2hip_plonk_create_proof_phased(*a[:8], C.byref(wit[0]), *a[8:])
    else:
        entry = ctx.lib.h2hip_plonk_create_proof
    if isinstance(rng, ArrayRng):   # libh2hip's own array RNG: no Python frame per draw (a wide shape draws several hundred blinding tails)
        st = _ArrayRngState(rng.values.ctypes.data + 32 * rng.pos, len(rng.values) - rng.pos, 0, 0)
        rc = entry(ctx.handle, pk.handle, adv, 1 if advice_on_device else 0, ip, il,
                                              C.cast(ctx.lib.h2hip_array_rng_fill, _vp), C.cast(C.pointer(st), _vp), _ptr(proof), proof.nbytes,
                                              C.byref(plen), stage)
        rng.pos += st.pos
        if st.exhausted:
            raise RuntimeError("ArrayRng exhausted")
    elif isinstance(rng, ChaChaRng) and rng.device:   # libh2hip's seeded generator: the prover's device path for the large draws
        rc = entry(ctx.handle, pk.handle, adv, 1 if advice_on_device else 0, ip, il,
                                              C.cast(ctx.lib.h2hip_chacha_rng_fill, _vp), C.cast(C.pointer(rng.state), _vp), _ptr(proof), proof.nbytes,
                                              C.byref(plen), stage)
    else:
        cb = _RNG_FN(_fill)
        rc = entry(ctx.handle, pk.handle, adv, 1 if advice_on_device else 0, ip, il, C.cast(cb, _vp), None, _ptr(proof),
                                              proof.nbytes, C.byref(plen), stage)
    if err:
        raise err[0]
    ctx._chk(rc)
    if timings is not None:
        for i in range(PLONK_STAGES):
            name = ctx.lib.h2hip_plonk_stage_name(i).decode()
            timings[name] = timings.get(name, 0.0) + stage[i]
    del keep
    if transcript is not None:
        return transcript.finalize() if hasattr(transcript, "finalize") else None
    return proof[: plen.value].tobytes()


def _phase_witness_trampoline(ctx: Context, n: int, phase_witness, err: list, phase_witness_dev=None):
    """(h2hip_phase_witness, the callback object to keep alive) over phase_witness(phase, challenges) -> list of columns, or over
    phase_witness_dev(phase, challenges, column_ptrs), which writes the device columns itself"""
    one = fr_limbs(1)

    def _fill(_user, phase, chal, nchal, cols, ncols):
        try:
            if phase_witness is None and phase_witness_dev is None:
                raise ValueError("create_proof: the key has a later phase and no phase_witness was given")
            ch = np.ctypeslib.as_array(C.cast(chal, C.POINTER(C.c_uint64)), shape=(nchal, 4)).copy() if nchal else np.zeros((0, 4), dtype=np.uint64)
            if phase_witness_dev is not None:
                phase_witness_dev(int(phase), [fr_int(r) for r in ch], [int(cols[j]) for j in range(ncols)])
                ctx.sync()
                return 0
            got = list(phase_witness(int(phase), [fr_int(r) for r in ch]))
            if len(got) != ncols:
                raise ValueError("phase_witness: phase %d has %d columns, got %d" % (phase, ncols, len(got)))
            for j, col in enumerate(got):
                if isinstance(col, (int, np.integer)):   # a device pointer to n Fr: y += 1 * x into the zeroed column
                    ctx._chk(ctx.lib.h2hip_fr_axpy_dev(ctx.handle, _vp(cols[j]), _ptr(one), _vp(int(col)), n))
                else:
                    a = _fe(col)
                    if len(a) > n:
                        raise ValueError("phase_witness: a column has more than 2^k rows")
                    ctx._chk(ctx.lib.h2hip_upload(ctx.handle, _vp(cols[j]), _ptr(a), a.nbytes))
            ctx.sync()
            return 0
        except BaseException as e:   # never unwind through the C frames
            err.append(e)
            return 1

    cb = _PHASE_FN(_fill)
    return _PhaseWitness(C.cast(cb, _vp), None), cb


def verify_proof(pk: ProvingKey, instances: Sequence[np.ndarray], proof: Optional[bytes] = None, transcript=None, want_accumulator: bool = False):
    """verify_proof with the key's verifying half (VerifierSHPLONK, SingleStrategy) — check_proof of halo2-base/src/utils/testing.rs:64-88.
    Host code inside libh2hip; needs the G2 half of the SRS (ParamsKZG.g2_raw).
    transcript: instead of `proof`, the caller's reading transcript (h2hip_plonk_verify_proof_transcript) with common_scalar(int), read_point()
    -> (x, y), read_scalar() -> int and squeeze_challenge() -> int, as oracle/transcript.py's Blake2bRead has them.  A read that raises, or
    returns a bad value, rejects the proof (the exception is dropped: a malformed proof is not an error); an exception in common_scalar or
    squeeze_challenge is re-raised.  If the object has exhausted(), input left over rejects the proof.  want_accumulator: return (accepted,
    acc) with acc the (2, 8) uint64 pair (W', outer) the pairing decides (zeros when the proof is malformed)."""
    if transcript is not None:
        if proof is not None:
            raise ValueError("verify_proof: give proof or transcript, not both")
        return _verify_proof_transcript(pk, instances, transcript, want_accumulator)
    if want_accumulator:
        raise ValueError("verify_proof: want_accumulator needs transcript=")
    ctx, kind = pk.ctx, _KIND_OF[type(pk.params)]
    vk, keep = _vk_args("verify_proof", pk)
    (ip, il), inst = _instance_args("verify_proof", pk.params, instances)
    buf = np.frombuffer(bytes(proof), dtype=np.uint8).copy()
    ok = C.c_int(0)
    ctx._chk(getattr(ctx.lib, kind.verify_proof)(C.byref(pk.params), *vk, *((ip, il) if kind.verify_instances else ()), _vp(buf.ctypes.data), len(buf),
                                                 C.byref(ok)))
    del keep
    return bool(ok.value)


def _verify_proof_transcript(pk: ProvingKey, instances, transcript, want_accumulator: bool):
    ctx = pk.ctx
    vk, keep_vk = _vk_args("verify_proof", pk)
    (ip, il), inst = _instance_args("verify_proof", pk.params, instances)
    err = []
    tr, keep = _transcript_trampolines(transcript, err)
    ok = C.c_int(0)
    acc = np.zeros((2, 8), dtype=np.uint64)
    rc = ctx.lib.h2hip_plonk_verify_proof_transcript(_KIND_OF[type(pk.params)].id, C.cast(C.byref(pk.params), _vp), *vk, ip if inst else None,
                                                     il if inst else None, C.byref(tr), C.byref(ok), _ptr(acc))
    del keep, keep_vk
    if rc != 0 and err:   # the transcript failed where no proof byte is involved
        raise err[0]
    ctx._chk(rc)
    accepted = bool(ok.value)
    if accepted and hasattr(transcript, "exhausted") and not transcript.exhausted():
        accepted = False
    return (accepted, acc) if want_accumulator else accepted


def verify_batch(pk: ProvingKey, instances_per_proof: Sequence, proofs: Sequence[bytes], rng=None, want_rejected: bool = False,
                 want_acc: bool = False, kind: Optional[int] = None):
    """h2hip_plonk_verify_batch: every proof of `proofs` under pk's verifying key with one pairing; the points are decompressed and the scalar
    multiplications run on the GPU.  -> (accepted, rejected: list[bool] or None, acc: (2, 8) uint64 array (L, R) or None).  rng draws one
    combiner per proof in one call: ArrayRng / ChaChaRng / any object with fill_into(dst, n); None = a ChaChaRng seeded from os.urandom, host
    draws."""
    ctx = pk.ctx
    if kind is None:
        kind = _CIRCUIT_KINDS[type(pk.params)]
    vk, keep_vk = _vk_args("verify_batch", pk)
    if len(instances_per_proof) != len(proofs):
        raise ValueError("verify_batch: need one list of instance columns per proof")
    ni, count = pk.params.num_instance, len(proofs)
    inst = [[_fe(c) for c in cols] for cols in instances_per_proof]
    if any(len(cols) != ni for cols in inst):
        raise ValueError("verify_batch: need %d instance columns per proof" % ni)
    ip, il = _column_arrays([c for cols in inst for c in cols])
    bufs = [np.frombuffer(bytes(p), dtype=np.uint8).copy() if len(p) else np.zeros(1, dtype=np.uint8) for p in proofs]
    pp = (_vp * max(count, 1))(*[_vp(b.ctypes.data) for b in bufs])
    pl = (C.c_size_t * max(count, 1))(*[len(p) for p in proofs])
    if rng is None:
        import os

        rng = ChaChaRng(ctx.lib, os.urandom(32), device=False)
    err = []

    def _fill(_user, out, n):
        try:
            rng.fill_into(out, n)
        except BaseException as e:   # never unwind through the C frames
            err.append(e)
            C.memset(out, 0, 32 * n)

    cb = _RNG_FN(_fill)
    ok = C.c_int(0)
    rejected = np.zeros(max(count, 1), dtype=np.uint8) if want_rejected else None
    acc = np.zeros((2, 8), dtype=np.uint64) if want_acc else None
    rc = ctx.lib.h2hip_plonk_verify_batch(ctx.handle, kind, C.cast(C.byref(pk.params), _vp), *vk, count, ip if ni else None, il if ni else None, pp, pl,
                                          C.cast(cb, _vp), None, C.byref(ok), _ptr(rejected) if want_rejected else None,
                                          _ptr(acc) if want_acc else None)
    del keep_vk
    if err:
        raise err[0]
    ctx._chk(rc)
    return bool(ok.value), ([bool(v) for v in rejected[:count]] if want_rejected else None), acc


def verify_proofs(pk: ProvingKey, instances_per_proof: Sequence, proofs: Sequence[bytes], rng=None, want_rejected: bool = False):
    """verify_proof for a batch of proofs of one key (upstream's BatchVerifier): True iff every proof verifies; with want_rejected also the
    list of per-proof rejections.  instances_per_proof[i]: the instance columns of proof i."""
    ok, rejected, _ = verify_batch(pk, instances_per_proof, proofs, rng, want_rejected)
    return (ok, rejected) if want_rejected else ok


class BatchVerifier:
    """halo2_proofs::plonk::BatchVerifier: collect proofs with add_proof, decide them together with finalize"""

    def __init__(self):
        self.items = []

    def add_proof(self, instances: Sequence[np.ndarray], proof: bytes):
        self.items.append((list(instances), bytes(proof)))

    def finalize(self, pk: ProvingKey, rng=None) -> bool:
        return verify_proofs(pk, [i for i, _ in self.items], [p for _, p in self.items], rng)


class WitnessFailure(NamedTuple):
    """one failure of check_witness (h2hip_witness_failure): kind = "gate" (column = advice index of the gate column), "lookup" (column = lookup
    index in the key's order) or "copy" (column, row = permutation column and row; peer_* = sigma of that cell); row = the gate's / input's row"""
    kind: str
    column: int
    row: int
    peer_column: int = 0
    peer_row: int = 0

    def __str__(self) -> str:
        if self.kind == "gate":
            return "gate column %d not satisfied at row %d" % (self.column, self.row)
        if self.kind == "lookup":
            return "lookup %d: input at row %d is not in the table" % (self.column, self.row)
        return "copy: permutation column %d row %d != column %d row %d" % (self.column, self.row, self.peer_column, self.peer_row)


_KINDS = {WITNESS_GATE: "gate", WITNESS_LOOKUP: "lookup", WITNESS_COPY: "copy"}


def check_witness(pk: ProvingKey, advice: Sequence, instances: Sequence[np.ndarray] = (), max_failures: int = 64,
                  advice_on_device: bool = False, challenges: Optional[Sequence[int]] = None) -> tuple:
    """MockProver::run(k, &circuit, instances).verify() for the key's configuration, on the GPU (h2hip_plonk_check_witness): every advice
    column of the key (all phases of a PhasedCircuitParams key, advice index order; host (n,4) arrays or device pointers with advice_on_device),
    the instance columns.  Returns (exact number of failures, the first max_failures of them in canonical order: gate, lookup, copy; by column,
    then row).  challenges (the phases' challenges as ints, squeeze order): h2hip_plonk_check_witness_challenges, which also checks the RLC
    gates of an RlcCircuitParams key with challenge 0 (their failures are gate failures naming the RLC column's advice index)."""
    ctx, sh = pk.ctx, pk.shape
    n = 1 << pk.params.k
    if len(advice) != sh.num_advice_total:
        raise ValueError("check_witness: need %d advice columns" % sh.num_advice_total)
    adv, keep = _advice_args("check_witness", advice, n, advice_on_device)
    (ip, il), inst = _instance_args("check_witness", pk.params, instances)
    out = (WitnessFailureStruct * max(max_failures, 1))()
    total = C.c_size_t(0)
    if challenges is not None:
        ch = np.ascontiguousarray(np.concatenate([fr_limbs(int(c) % R_MOD).reshape(1, 4) for c in challenges]) if len(challenges) else
                                  np.zeros((0, 4), dtype=np.uint64))
        ctx._chk(ctx.lib.h2hip_plonk_check_witness_challenges(ctx.handle, pk.handle, adv, 1 if advice_on_device else 0, ip, il,
                                                              _ptr(ch) if len(ch) else None, len(ch),
                                                              C.cast(out, _vp) if max_failures else None, max_failures, C.byref(total)))
    else:
        ctx._chk(ctx.lib.h2hip_plonk_check_witness(ctx.handle, pk.handle, adv, 1 if advice_on_device else 0, ip, il,
                                                   C.cast(out, _vp) if max_failures else None, max_failures, C.byref(total)))
    del keep
    got = [WitnessFailure(_KINDS[f.kind], f.column, f.row, f.peer_column, f.peer_row) for f in out[: min(total.value, max_failures)]]
    return total.value, got


def assert_satisfied(pk: ProvingKey, advice: Sequence, instances: Sequence[np.ndarray] = (), max_failures: int = 16,
                     advice_on_device: bool = False) -> None:
    """MockProver::assert_satisfied: raises AssertionError naming the first failures (kind, column, row) when the witness does not satisfy the
    key's circuit"""
    total, fails = check_witness(pk, advice, instances, max_failures, advice_on_device)
    if total:
        more = "" if total <= len(fails) else "\n... and %d more" % (total - len(fails))
        raise AssertionError("witness not satisfied: %d failure%s\n" % (total, "" if total == 1 else "s") + "\n".join(map(str, fails)) + more)


# ---- argument marshalling of the device fills
def _col_array(columns: Sequence) -> C.Array:
    """the column pointer array of a fill (a missing column as NULL)"""
    return (_vp * max(len(columns), 1))(*[_vp(int(p)) if p else None for p in columns])


def _bp_array(break_points: Optional[Sequence[int]], num_columns: int):
    if break_points is None:
        return None
    assert len(break_points) == num_columns - 1, "one break point per column but the last"
    return (C.c_uint32 * max(len(break_points), 1))(*[int(b) for b in break_points])


def _dev_ptr(x):
    """a device pointer (or an object with data_ptr()) as c_void_p, None / 0 as NULL"""
    v = int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x or 0)
    return _vp(v) if v else None


def _as_table(units, build) -> C.Array:
    return units if isinstance(units, C.Array) else build(units)


def _struct_table(struct, units: Sequence) -> C.Array:
    return (struct * max(len(units), 1))(*[struct(*[int(x) for x in u]) for u in units])


def _raise_on(code: int, lib) -> None:
    """the raise of a library call made without a context"""
    if code != 0:
        raise H2HipError(code, lib.h2hip_last_error().decode(errors="replace"))


class RlcChainStruct(C.Structure):   # h2hip_rlc_chain
    _fields_ = [("column", C.c_uint32), ("row", C.c_uint32), ("len", C.c_uint32), ("flags", C.c_uint32), ("value_offset", C.c_uint64)]


RLC_CARRY = 1


def rlc_fill_chains(ctx: Context, columns: Sequence[int], usable_rows: int, values_dev, chains: Sequence, gamma: int, num_values: Optional[int] = None) -> None:
    """h2hip_rlc_fill_chains_dev: RlcChip::compute_rlc_fixed_len's cells for every piece of `chains`, written into the device columns
    `columns` (pointers to Fr columns, e.g. the column_ptrs of phase_witness_dev).  chains: (column, row, len, flags, value_offset) tuples, flags 0
    (head piece) or RLC_CARRY (continues the piece before it after a column break); values_dev: a device pointer (then num_values is required) or
    an object with data_ptr() / nbytes (a torch tensor of Montgomery limbs).  gamma: an int.  Stream-ordered on the context's stream."""
    if num_values is None:
        num_values = int(values_dev.numel() * values_dev.element_size()) // 32
    ctx._chk(ctx.lib.h2hip_rlc_fill_chains_dev(ctx.handle, _col_array(columns), len(columns), usable_rows, _dev_ptr(values_dev), num_values,
                                               _struct_table(RlcChainStruct, chains), len(chains), _ptr(fr_limbs(int(gamma) % R_MOD))))


class GateChainStruct(C.Structure):   # h2hip_gate_chain
    _fields_ = [("column", C.c_uint32), ("row", C.c_uint32), ("len", C.c_uint32), ("flags", C.c_uint32), ("a_offset", C.c_uint64),
                ("b_offset", C.c_uint64), ("a_stride", C.c_uint32), ("b_stride", C.c_uint32)]


GATE_CARRY, GATE_JOIN, GATE_START_A = 1, 2, 4


def gate_fill_chains(ctx: Context, columns: Sequence[int], usable_rows: int, a_dev, a_len: int, b_dev, b_len: int, chains: Sequence) -> None:
    """h2hip_gate_fill_chains_dev: the flex-gate chain cells s_0, a_1, b_1, s_1, ... (s_i = s_{i-1} + a_i * b_i: inner products, sums,
    select_by_indicator, select_from_idx) for every piece of `chains`, written into the device columns `columns` (pointers to Fr columns, e.g.
    the column_ptrs of phase_witness_dev).  chains: (column, row, len, flags, a_offset, b_offset, a_stride, b_stride) tuples, flags 0 (head piece),
    GATE_START_A (head piece whose first left operand is the start), GATE_CARRY (continues the piece before it after a column break) or GATE_JOIN
    (continues it directly below), or a ctypes array of GateChainStruct built once for a table used in every proof; operand i of a piece is
    element a_offset + i * a_stride of a_dev (b alike).  a_dev / b_dev: device pointers (or
    objects with data_ptr()) to a_len / b_len Fr elements; they may point into a column.  Stream-ordered on the context's stream."""
    arr = _as_table(chains, lambda c: _struct_table(GateChainStruct, c))
    ctx._chk(ctx.lib.h2hip_gate_fill_chains_dev(ctx.handle, _col_array(columns), len(columns), usable_rows, _dev_ptr(a_dev), a_len, _dev_ptr(b_dev), b_len, arr,
                                                len(chains)))


class RangeCheckStruct(C.Structure):   # h2hip_range_check
    _fields_ = [("column", C.c_uint32), ("row", C.c_uint32), ("a_offset", C.c_uint64), ("b_offset", C.c_uint64), ("lookup_slot", C.c_uint64)]


RANGE_LESS_THAN = 1


def range_check_table(units: Sequence) -> C.Array:
    """a ctypes table of h2hip_range_check from (column, row, a_offset, b_offset, lookup_slot) tuples: build it once for a layout used in every
    proof (a table of thousands of structs costs milliseconds to build)"""
    return _struct_table(RangeCheckStruct, units)


def range_check_layout(range_bits: int, lookup_bits: int, flags: int = 0, lib=None):
    """h2hip_range_check_layout -> (gate cells of one unit, its lookup cells, the offset of the last-limb cell inside the gate cells or None
    when the unit has no such cell of its own: one limb without the LESS_THAN prefix)"""
    lib = lib or load_library()
    cells, lookups, last = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0)
    code = lib.h2hip_range_check_layout(range_bits, lookup_bits, flags, C.byref(cells), C.byref(lookups), C.byref(last))
    _raise_on(code, lib)
    return cells.value, lookups.value, None if last.value == 0xFFFFFFFF else last.value


def range_fill_checks(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], lookup_columns: Sequence[int],
                      values_dev, values_len: int, range_bits: int, lookup_bits: int, units, shift_bits: int = 0, flags: int = 0) -> None:
    """h2hip_range_fill_checks_dev: the gate cells of RangeChip::_range_check at `range_bits` (behind check_less_than's / is_less_than's seven
    cells with RANGE_LESS_THAN) for every unit, written down the device columns `columns` from each unit's (column, row) across the break
    points, and the copies of the limbs into `lookup_columns` at each unit's queue position.  units: (column, row, a_offset, b_offset,
    lookup_slot) tuples or a table from range_check_table() built once; the checked value is values_dev[a_offset] (a + 2^shift_bits -
    values_dev[b_offset] with RANGE_LESS_THAN).  values_dev: a device pointer (or an object with data_ptr()), which may point into a column.
    Stream-ordered on the context's stream."""
    arr = _as_table(units, range_check_table)
    ctx._chk(ctx.lib.h2hip_range_fill_checks_dev(ctx.handle, _col_array(columns), len(columns), usable_rows, _bp_array(break_points, len(columns)),
                                                 _col_array(lookup_columns), len(lookup_columns), _dev_ptr(values_dev), values_len, range_bits, lookup_bits,
                                                 shift_bits, flags, C.cast(arr, _vp), len(units)))


class FpParamsStruct(C.Structure):   # h2hip_fp_params
    _fields_ = [("limb_bits", C.c_uint32), ("num_limbs", C.c_uint32), ("lookup_bits", C.c_uint32), ("flags", C.c_uint32), ("modulus", C.c_uint8 * 48)]


class FpMulStruct(C.Structure):   # h2hip_fp_mul
    _fields_ = [("column", C.c_uint32), ("row", C.c_uint32), ("a_offset", C.c_uint64), ("b_offset", C.c_uint64)]


class FpMulRangeStruct(C.Structure):   # h2hip_fp_mul_range
    _fields_ = [("cell_offset", C.c_uint32), ("num_cells", C.c_uint32), ("range_bits", C.c_uint32), ("result_index", C.c_uint32)]


def fp_params(limb_bits: int, num_limbs: int, lookup_bits: int, modulus: int, flags: int = 0) -> FpParamsStruct:
    """h2hip_fp_params for a non-native field of modulus p < 2^384 in num_limbs limbs of limb_bits bits"""
    return FpParamsStruct(limb_bits, num_limbs, lookup_bits, flags, (C.c_uint8 * 48)(*int(modulus).to_bytes(48, "little")))


def fp_mul_table(units: Sequence) -> C.Array:
    """a ctypes table of h2hip_fp_mul from (column, row, a_offset, b_offset) tuples: build it once for a layout used in every proof"""
    return _struct_table(FpMulStruct, units)


class _FusedKind(NamedTuple):
    """one kind of fused unit (a library call of a solve and a place kernel, with its layout and range-check functions)"""
    table: Callable          # the builder of its unit table
    layout: str              # the three library functions
    fill: str
    range_checks: str
    has_op: bool             # they take an op behind params
    max_ranges: int          # the layout function's ranges / out_cell_offsets buffers,
    max_outs: int
    valid: Callable          # (k, op) -> how many entries of each are valid
    results_per_unit: bool   # the layout function reports it
    groups: Callable         # (k, ranges) -> [(width, gaps)]: how the flat check array is cut into tables, in its order


def _by_width(_k: int, ranges: list) -> list:
    widths: dict = {}
    for r in ranges:
        widths[r[2]] = widths.get(r[2], 0) + 1             # (a dict keeps the order of first appearance)
    return list(widths.items())


def _fused_layout(kind: _FusedKind, params, op: int, lib) -> list:
    """the fields of the kind's layout tuple"""
    lib = lib or load_library()
    sizes = [C.c_size_t(0) for _ in range(4 if kind.results_per_unit else 3)]
    ranges, outs = (FpMulRangeStruct * kind.max_ranges)(), (C.c_uint32 * kind.max_outs)()
    code = getattr(lib, kind.layout)(C.cast(C.pointer(params), _vp), *([op] if kind.has_op else []), *[C.byref(x) for x in sizes], C.cast(ranges, _vp), outs)
    _raise_on(code, lib)
    nranges, nouts = kind.valid(params.num_limbs, op)
    return [x.value for x in sizes] + [[(r.cell_offset, r.num_cells, r.range_bits, r.result_index) for r in ranges[:nranges]], list(outs[:nouts])]


def _fused_fill(kind: _FusedKind, ctx: Context, columns, usable_rows, break_points, params, op, values_dev, values_len, results_dev, results_len, units, count) -> None:
    arr = _as_table(units, kind.table)
    ctx._chk(getattr(ctx.lib, kind.fill)(ctx.handle, _col_array(columns), len(columns), usable_rows, _bp_array(break_points, len(columns)),
                                         C.cast(C.pointer(params), _vp), *([op] if kind.has_op else []), _dev_ptr(values_dev), values_len,
                                         _dev_ptr(results_dev), results_len, C.cast(arr, _vp), len(units) if count is None else count))


def _fused_range_tables(kind: _FusedKind, break_points, num_columns, params, op, units, lookup_slots, lib) -> list:
    lib = lib or load_library()
    ranges = _fused_layout(kind, params, op, lib)[-2]
    count = len(lookup_slots)
    if not count or not ranges:
        return []
    arr = _as_table(units, kind.table)
    checks = (RangeCheckStruct * (len(ranges) * count))()
    code = getattr(lib, kind.range_checks)(_bp_array(break_points, num_columns), num_columns, C.cast(C.pointer(params), _vp), *([op] if kind.has_op else []),
                                           C.cast(arr, _vp), (C.c_uint64 * count)(*lookup_slots), count, C.cast(checks, _vp))
    _raise_on(code, lib)
    tables, at = [], 0
    for bits, gaps in kind.groups(params.num_limbs, ranges):
        tables.append((bits, (RangeCheckStruct * (gaps * count)).from_buffer(checks, C.sizeof(RangeCheckStruct) * at)))
        at += gaps * count
    return tables


def _fused_fill_with_ranges(kind: _FusedKind, ctx: Context, columns, usable_rows, break_points, lookup_columns, params, op, values_dev, values_len, results_dev,
                            results_len, units, lookup_slots, range_tables) -> None:
    assert results_dev, "the range checks read results_dev"
    arr = _as_table(units, kind.table)
    tables = range_tables if range_tables is not None else _fused_range_tables(kind, break_points, len(columns), params, op, arr, lookup_slots, ctx.lib)
    _fused_fill(kind, ctx, columns, usable_rows, break_points, params, op, values_dev, values_len, results_dev, results_len, arr, len(units))
    for bits, table in tables:
        range_fill_checks(ctx, columns, usable_rows, break_points, lookup_columns, results_dev, results_len, bits, params.lookup_bits, table)


# gap-major: the gaps of one width are consecutive (o_i, the last o, q_i + B, the last q, -c_i + 2^rb)
_FP_MUL = _FusedKind(fp_mul_table, "h2hip_fp_mul_layout", "h2hip_fp_mul_fill_dev", "h2hip_fp_mul_range_checks", False, 12, 5, lambda k, _op: (3 * k, k + 1), False,
                     lambda k, ranges: [(ranges[j0][2], j1 - j0) for j0, j1 in ((0, k - 1), (k - 1, k), (k, 2 * k - 1), (2 * k - 1, 2 * k), (2 * k, 3 * k))])


class FpMulLayout(NamedTuple):
    """h2hip_fp_mul_layout: the cells of one FpChip::mul unit, its own cells (the rest are the gaps of its range checks), the lookup cells of
    those checks, ranges = [(cell_offset, num_cells, range_bits, result_index)] of the 3 k gaps in context order (o, q, c: the lookup queue
    order) and the offsets of the o_i cells and of out_native"""
    num_cells: int
    num_own_cells: int
    num_lookup_cells: int
    ranges: list
    out_cell_offsets: list


def fp_mul_layout(params: FpParamsStruct, lib=None) -> FpMulLayout:
    return FpMulLayout(*_fused_layout(_FP_MUL, params, 0, lib))


def trace_seek(break_points: Optional[Sequence[int]], num_columns: int, column: int, row: int, offset: int, lib=None):
    """h2hip_trace_seek: the (column, row) of cell `offset` of a run laid down from (column, row) as assign_witnesses does (the cell on a break
    point: its first position; the cell behind it lies at row 1 of the next column)"""
    lib = lib or load_library()
    c, r = C.c_uint32(0), C.c_uint32(0)
    code = lib.h2hip_trace_seek(_bp_array(break_points, num_columns), num_columns, column, row, offset, C.byref(c), C.byref(r))
    _raise_on(code, lib)
    return c.value, r.value


def fp_mul_fill(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], params: FpParamsStruct, values_dev,
                values_len: int, results_dev, results_len: int, units, count: Optional[int] = None) -> None:
    """h2hip_fp_mul_fill_dev: the own cells of FpChip::mul (mul_no_carry::crt, then carry_mod::crt) for every unit, written down the device
    columns from each unit's (column, row) across the break points; the cells of the nine range checks are left as gaps.  units: (column, row,
    a_offset, b_offset) tuples or a table from fp_mul_table(); an operand is the k + 1 Fr of values_dev from its offset (k limbs, then the
    native residue).  results_dev (or None): 3 k + 1 Fr per unit — o_i, out_native, q_i + B, -c_i + 2^rb.  count: the units of a table
    to fill (default: all).  Stream-ordered on the context's stream."""
    _fused_fill(_FP_MUL, ctx, columns, usable_rows, break_points, params, 0, values_dev, values_len, results_dev, results_len, units, count)


def fp_mul_range_tables(break_points: Optional[Sequence[int]], num_columns: int, params: FpParamsStruct, units, lookup_slots: Sequence[int], lib=None) -> list:
    """h2hip_fp_mul_range_checks: [(width, range_check_table)] of the range checks of `units` ((column, row, a_offset, b_offset) tuples or a
    table from fp_mul_table()), five tables of one width each in context order (the checks of o_i, of the last o, of q_i + B, of the last q,
    of -c_i + 2^rb), all made by one library call: each check's (column, row) by trace_seek's walk from its unit's first cell, its value at
    results index u (3 k + 1) + result_index, its lookup_slot from lookup_slots[u].  Build it once for a layout used in every proof."""
    return _fused_range_tables(_FP_MUL, break_points, num_columns, params, 0, units, lookup_slots, lib)


def fp_mul_fill_with_ranges(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], lookup_columns: Sequence[int],
                            params: FpParamsStruct, values_dev, values_len: int, results_dev, results_len: int, units, lookup_slots: Sequence[int] = (),
                            range_tables: Optional[list] = None) -> None:
    """fp_mul_fill, then five range_fill_checks calls (one per group of gaps of one width) from results_dev: the whole run of every unit and
    its lookup cells.  units: (column, row, a_offset, b_offset) tuples or a table from fp_mul_table(); lookup_slots[u]: the queue position of
    unit u's first lookup cell (not read with range_tables, the result of fp_mul_range_tables() built once for the layout)."""
    _fused_fill_with_ranges(_FP_MUL, ctx, columns, usable_rows, break_points, lookup_columns, params, 0, values_dev, values_len, results_dev, results_len, units,
                            lookup_slots, range_tables)


class EcOpStruct(C.Structure):   # h2hip_ec_op
    _fields_ = [("column", C.c_uint32), ("row", C.c_uint32), ("p_offset", C.c_uint64), ("q_offset", C.c_uint64)]


EC_ADD_UNEQUAL, EC_DOUBLE, EC_SUB_UNEQUAL = 0, 1, 3   # (2 is no operation: the library refuses it as unknown)


def ec_op_table(units: Sequence) -> C.Array:
    """a ctypes table of h2hip_ec_op from (column, row, p_offset, q_offset) tuples: build it once for a layout used in every proof"""
    return _struct_table(EcOpStruct, units)


_EC = _FusedKind(ec_op_table, "h2hip_ec_layout", "h2hip_ec_fill_dev", "h2hip_ec_range_checks", True, 36, 15, lambda k, _op: (9 * k, 3 * (k + 1)), False, _by_width)


class EcLayout(NamedTuple):
    """h2hip_ec_layout: the cells of one ec_add_unequal / ec_double unit, its own cells (the rest are the gaps of its range checks), the lookup
    cells of those checks, ranges = [(cell_offset, num_cells, range_bits, result_index)] of the 9 k gaps in context order (the lookup queue
    order) and the offsets of the cells of x3, y3 and lambda (k limb cells and the native cell each)"""
    num_cells: int
    num_own_cells: int
    num_lookup_cells: int
    ranges: list
    out_cell_offsets: list


def ec_layout(params: FpParamsStruct, op: int, lib=None) -> EcLayout:
    return EcLayout(*_fused_layout(_EC, params, op, lib))


def ec_fill(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], params: FpParamsStruct, op: int, values_dev,
            values_len: int, results_dev, results_len: int, units, count: Optional[int] = None) -> None:
    """h2hip_ec_fill_dev: the own cells of ec_add_unequal (non-strict, op = EC_ADD_UNEQUAL), ec_sub_unequal (non-strict, EC_SUB_UNEQUAL: P - Q) or
    ec_double (EC_DOUBLE) for every unit, written down
    the device columns from each unit's (column, row) across the break points; the cells of the 9 k range checks are left as gaps.  units:
    (column, row, p_offset, q_offset) tuples or a table from ec_op_table(); a point is the 2 (k + 1) Fr of values_dev from its offset (x's k
    limbs and native residue, then y's).  results_dev (or None): 9 k + 3 Fr per unit — x3, y3 (a point a later call may read), lambda, then
    per reduction q_i + B and -c_i + 2^rb.  count: the units of a table to fill (default: all).  Stream-ordered on the context's stream."""
    _fused_fill(_EC, ctx, columns, usable_rows, break_points, params, op, values_dev, values_len, results_dev, results_len, units, count)


def ec_range_tables(break_points: Optional[Sequence[int]], num_columns: int, params: FpParamsStruct, op: int, units, lookup_slots: Sequence[int],
                    lib=None) -> list:
    """h2hip_ec_range_checks: [(width, range_check_table)] of the range checks of `units` ((column, row, p_offset, q_offset) tuples or a table
    from ec_op_table()), one table per distinct width in the order of first appearance among ec_layout's ranges, all made by one library call;
    inside a table the checks run unit by unit (rows and lookup slots ascend).  lookup_slots[u]: the queue position of unit u's first lookup
    cell.  Build it once for a layout used in every proof."""
    return _fused_range_tables(_EC, break_points, num_columns, params, op, units, lookup_slots, lib)


def ec_fill_with_ranges(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], lookup_columns: Sequence[int],
                        params: FpParamsStruct, op: int, values_dev, values_len: int, results_dev, results_len: int, units,
                        lookup_slots: Sequence[int] = (), range_tables: Optional[list] = None) -> None:
    """ec_fill, then one range_fill_checks call per width group from results_dev: the whole run of every unit and its lookup cells.
    lookup_slots[u]: the queue position of unit u's first lookup cell (not read with range_tables, the result of ec_range_tables() built once
    for the layout)."""
    _fused_fill_with_ranges(_EC, ctx, columns, usable_rows, break_points, lookup_columns, params, op, values_dev, values_len, results_dev, results_len, units,
                            lookup_slots, range_tables)


FP_CMP_REDUCE_A, FP_CMP_REDUCE_B, FP_CMP_EQUAL = 1, 2, 4
NO_CELL = 0xFFFFFFFF
_FP_CMP = _FusedKind(fp_mul_table, "h2hip_fp_cmp_layout", "h2hip_fp_cmp_fill_dev", "h2hip_fp_cmp_range_checks", True, 8, 3,
                     lambda k, op: (k * (bool(op & FP_CMP_REDUCE_A) + bool(op & FP_CMP_REDUCE_B)), 3), True, _by_width)


class FpCmpLayout(NamedTuple):
    """h2hip_fp_cmp_layout: the cells of one comparison unit (enforce_less_than_p of a and / or b, big_is_equal of the pair, by the mask), its
    own cells (the rest are the gaps of its range checks), their lookup cells, the results entries per unit, ranges = [(cell_offset,
    num_cells, range_bits, result_index)] of the gaps in context order, and the offsets of the final borrow cell of a's check, of b's and of
    the equality cell (NO_CELL where the mask has none)"""
    num_cells: int
    num_own_cells: int
    num_lookup_cells: int
    results_per_unit: int
    ranges: list
    out_cell_offsets: list


def fp_cmp_layout(params: FpParamsStruct, op: int, lib=None) -> FpCmpLayout:
    return FpCmpLayout(*_fused_layout(_FP_CMP, params, op, lib))


def fp_cmp_fill(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], params: FpParamsStruct, op: int, values_dev,
                values_len: int, results_dev, results_len: int, units, count: Optional[int] = None) -> None:
    """h2hip_fp_cmp_fill_dev: the own cells of FpChip's comparisons for every unit — by the mask `op`, enforce_less_than_p(a) (FP_CMP_REDUCE_A),
    enforce_less_than_p(b) (FP_CMP_REDUCE_B), big_is_equal(a, b) (FP_CMP_EQUAL), in this order — written down the device columns from each
    unit's (column, row) across the break points; the cells of the k range checks per enforced operand are left as gaps.  units: (column, row,
    a_offset, b_offset) tuples or a table from fp_mul_table().  results_dev (or None): per unit, for each enforced operand s_0 .. s_{k-1} and
    the final borrow, then for EQUAL the equality cell's value.  Stream-ordered on the context's stream."""
    _fused_fill(_FP_CMP, ctx, columns, usable_rows, break_points, params, op, values_dev, values_len, results_dev, results_len, units, count)


def fp_cmp_range_tables(break_points: Optional[Sequence[int]], num_columns: int, params: FpParamsStruct, op: int, units, lookup_slots: Sequence[int],
                        lib=None) -> list:
    """h2hip_fp_cmp_range_checks: [(width, range_check_table)] of the range checks of `units`: one table (they share the width pad + lb), unit
    by unit (rows and lookup slots ascend); none for a mask that enforces no operand.  Build it once for a layout used in every proof."""
    return _fused_range_tables(_FP_CMP, break_points, num_columns, params, op, units, lookup_slots, lib)


def fp_cmp_fill_with_ranges(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], lookup_columns: Sequence[int],
                            params: FpParamsStruct, op: int, values_dev, values_len: int, results_dev, results_len: int, units,
                            lookup_slots: Sequence[int] = (), range_tables: Optional[list] = None) -> None:
    """fp_cmp_fill, then the one range_fill_checks call from results_dev: the whole run of every unit and its lookup cells."""
    _fused_fill_with_ranges(_FP_CMP, ctx, columns, usable_rows, break_points, lookup_columns, params, op, values_dev, values_len, results_dev, results_len, units,
                            lookup_slots, range_tables)


def ec_fill_strict_with_ranges(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], lookup_columns: Sequence[int],
                               params: FpParamsStruct, op: int, cmp_mask: int, values_dev, values_len: int, results_dev, results_len: int,
                               cmp_results_dev, cmp_results_len: int, units, lookup_slots: Sequence[int], tables: Optional[tuple] = None):
    """ec_add_unequal / ec_sub_unequal with is_strict = true (op = EC_ADD_UNEQUAL or EC_SUB_UNEQUAL): for each unit the comparison of
    check_points_are_unequal over (P.x, Q.x) at the unit's (column, row) — cmp_mask = FP_CMP_EQUAL, plus FP_CMP_REDUCE_A for a non-strict P
    and FP_CMP_REDUCE_B for a non-strict Q — and the curve operation directly behind it (its position by trace_seek, its lookup slots
    continuing the comparison's): the reference's context order, in two fused calls and the range calls.  units: (column, row, p_offset,
    q_offset) tuples; lookup_slots[u]: the queue position of unit u's first lookup cell.  cmp_results_dev takes the comparison's results
    (fp_cmp_layout's results_per_unit per unit), results_dev the curve operation's.  tables: the third item of an earlier call's return
    value for the same layout (units and lookup_slots are then not walked again).
    -> ([(column, row)] of each unit's equality cell, which the circuit pins to 0; [(column, row)] of each curve operation's first cell;
    the tables)"""
    assert op in (EC_ADD_UNEQUAL, EC_SUB_UNEQUAL) and cmp_mask & FP_CMP_EQUAL and 0 < cmp_mask <= 7
    assert results_dev and cmp_results_dev, "the range checks read the results"
    if tables is None:
        lib, ncols = ctx.lib, len(columns)
        cl = fp_cmp_layout(params, cmp_mask, lib)
        ec_units = [trace_seek(break_points, ncols, c, r, cl.num_cells, lib) + (p, q) for c, r, p, q in units]
        eq_cells = [trace_seek(break_points, ncols, c, r, cl.out_cell_offsets[2], lib) for c, r, _p, _q in units]
        cmp_table, ec_table = fp_mul_table(list(units)), ec_op_table(ec_units)   # (P.x and Q.x lead their points: the comparison's operands)
        tables = (eq_cells, [(c, r) for c, r, _p, _q in ec_units],
                  (cmp_table, fp_cmp_range_tables(break_points, ncols, params, cmp_mask, cmp_table, lookup_slots, lib),
                   ec_table, ec_range_tables(break_points, ncols, params, op, ec_table, [s + cl.num_lookup_cells for s in lookup_slots], lib)))
    eq_cells, ec_cells, (cmp_table, cmp_ranges, ec_table, ec_ranges) = tables
    fp_cmp_fill_with_ranges(ctx, columns, usable_rows, break_points, lookup_columns, params, cmp_mask, values_dev, values_len, cmp_results_dev, cmp_results_len,
                            cmp_table, range_tables=cmp_ranges)
    ec_fill_with_ranges(ctx, columns, usable_rows, break_points, lookup_columns, params, op, values_dev, values_len, results_dev, results_len, ec_table,
                        range_tables=ec_ranges)
    return eq_cells, ec_cells, tables


class EcSelectStruct(C.Structure):   # h2hip_ec_select
    _fields_ = [("column", C.c_uint32), ("row", C.c_uint32), ("p_offset", C.c_uint64), ("q_offset", C.c_uint64), ("sel_offset", C.c_uint64)]


class BitsUnitStruct(C.Structure):   # h2hip_bits_unit
    _fields_ = [("column", C.c_uint32), ("row", C.c_uint32), ("a_offset", C.c_uint64)]


EC_SELECT, EC_SELECT_FROM_BITS = 0, 1


def ec_select_table(units: Sequence) -> C.Array:
    """a ctypes table of h2hip_ec_select from (column, row, p_offset, q_offset, sel_offset) tuples: build it once for a layout used in every proof"""
    return _struct_table(EcSelectStruct, units)


def bits_unit_table(units: Sequence) -> C.Array:
    """a ctypes table of h2hip_bits_unit from (column, row, a_offset) tuples"""
    return _struct_table(BitsUnitStruct, units)


# no gaps, no range checks: of the record, the table builder, the two library functions and the out_cell_offsets buffer are read
_EC_SELECT = _FusedKind(ec_select_table, "h2hip_ec_select_layout", "h2hip_ec_select_fill_dev", "", True, 0, 10, lambda k, _op: (0, 2 * (k + 1)), False,
                        lambda _k, _ranges: [])


class EcSelectLayout(NamedTuple):
    """h2hip_ec_select_layout: the cells of one selection unit and the offsets of the cells of the selected point (x's k limb cells and native
    cell, then y's)"""
    num_cells: int
    out_cell_offsets: list


def ec_select_layout(params: FpParamsStruct, op: int, window_bits: int = 0, lib=None) -> EcSelectLayout:
    lib = lib or load_library()
    kind = _EC_SELECT
    cells, outs = C.c_size_t(0), (C.c_uint32 * kind.max_outs)()
    code = getattr(lib, kind.layout)(C.cast(C.pointer(params), _vp), op, window_bits, C.byref(cells), outs)
    _raise_on(code, lib)
    return EcSelectLayout(cells.value, list(outs[:kind.valid(params.num_limbs, op)[1]]))


def ec_select_fill(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], params: FpParamsStruct, op: int,
                   window_bits: int, values_dev, values_len: int, results_dev, results_len: int, units, count: Optional[int] = None) -> None:
    """h2hip_ec_select_fill_dev: every cell of ec_select (op = EC_SELECT, window_bits = 0: sel ? P : Q, one GateChip::select per limb and
    native cell of x and y) or of ec_select_from_bits (EC_SELECT_FROM_BITS: bits_to_indicator over the window_bits little-endian bits from
    sel_offset, then select_by_indicator::crt over the 2^window_bits points packed from p_offset) for every unit, written down the device
    columns from each unit's (column, row) across the break points.  units: (column, row, p_offset, q_offset, sel_offset) tuples or a table
    from ec_select_table(); a point is the 2 (k + 1) Fr of values_dev from its offset.  results_dev (or None): 2 (k + 1) Fr per unit, the
    selected point as the operand ec_fill, fp_cmp_fill or a later selection reads.  Stream-ordered on the context's stream."""
    kind = _EC_SELECT
    arr = _as_table(units, kind.table)
    ctx._chk(getattr(ctx.lib, kind.fill)(ctx.handle, _col_array(columns), len(columns), usable_rows, _bp_array(break_points, len(columns)),
                                         C.cast(C.pointer(params), _vp), op, window_bits, _dev_ptr(values_dev), values_len, _dev_ptr(results_dev), results_len,
                                         C.cast(arr, _vp), len(units) if count is None else count))


def num_to_bits_layout(num_bits: int, lib=None):
    """h2hip_num_to_bits_layout -> (cells of one unit, the offset of the recomposed sum's cell); bit 0 sits at offset 0, bit i at 1 + 3 (i - 1)"""
    lib = lib or load_library()
    cells, at = C.c_size_t(0), C.c_uint32(0)
    code = lib.h2hip_num_to_bits_layout(num_bits, C.byref(cells), C.byref(at))
    _raise_on(code, lib)
    return cells.value, at.value


def num_to_bits_fill(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], values_dev, values_len: int,
                     results_dev, results_len: int, num_bits: int, units, count: Optional[int] = None) -> None:
    """h2hip_num_to_bits_fill_dev: every cell of GateChip::num_to_bits at `num_bits` for every unit, written down the device columns from each
    unit's (column, row) across the break points.  units: (column, row, a_offset) tuples or a table from bits_unit_table(); the value is
    values_dev[a_offset].  results_dev (or None): num_bits Fr per unit, the bits little-endian (consecutive units leave one bit string, which
    ec_select_fill reads).  Stream-ordered on the context's stream."""
    arr = _as_table(units, bits_unit_table)
    ctx._chk(ctx.lib.h2hip_num_to_bits_fill_dev(ctx.handle, _col_array(columns), len(columns), usable_rows, _bp_array(break_points, len(columns)),
                                                _dev_ptr(values_dev), values_len, _dev_ptr(results_dev), results_len, num_bits, C.cast(arr, _vp),
                                                len(units) if count is None else count))
