"""PoseidonHasher (halo2-base/src/poseidon/hasher/mod.rs) on the GPU, batched over messages: the reference's names over
h2hip_poseidon_spec_generate + h2hip_poseidon_set_spec + h2hip_poseidon_hash_batch_dev, so a caller brings no constants of their own.
For circuits that constrain the hash, `fill_hashes` writes every gate cell of hash_fix_len_array into device columns
(h2hip_poseidon_fill_hashes_dev) over the optimised spec of `optimized_spec`."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np

from .h2hip import Context, _ptr, load_library, poseidon_spec_generate
from .plonk import _as_table, _bp_array, _col_array, _dev_ptr, _raise_on

_vp = C.c_void_p
ABSORB_ONLY, WITH_CONSTS = 1, 2   # H2HIP_POSEIDON_*


class PoseidonHashStruct(C.Structure):   # h2hip_poseidon_hash
    _fields_ = [("column", C.c_uint32), ("row", C.c_uint32), ("input_offset", C.c_uint64), ("input_stride", C.c_uint32), ("flags", C.c_uint32)]


class OptimizedSpec(NamedTuple):
    """OptimizedPoseidonSpec as Montgomery-limb arrays: start (r_f/2 + 1, t, 4), partial (r_p, 4), end (r_f/2 - 1, t, 4), mds and pre_sparse_mds
    (t, t, 4), sparse (r_p, 2t - 1, 4): per partial round the SparseMDSMatrix row, then col_hat"""
    start: np.ndarray
    partial: np.ndarray
    end: np.ndarray
    mds: np.ndarray
    pre_sparse_mds: np.ndarray
    sparse: np.ndarray


def spec_optimize(t: int, r_f: int, r_p: int, round_constants: np.ndarray, mds: np.ndarray, lib=None) -> OptimizedSpec:
    """h2hip_poseidon_spec_optimize: the optimised form of a textbook spec (host only)"""
    lib = lib or load_library()
    rc, m = np.ascontiguousarray(round_constants, dtype=np.uint64).reshape(-1, 4), np.ascontiguousarray(mds, dtype=np.uint64).reshape(-1, 4)
    assert len(rc) == (r_f + r_p) * t and len(m) == t * t
    half = r_f // 2
    z = lambda *shape: np.zeros(shape + (4,), dtype=np.uint64)
    start, partial, end, pre, sparse = z(half + 1, t), z(max(r_p, 1)), z(max(half - 1, 1), t), z(t, t), z(max(r_p, 1), 2 * t - 1)
    code = lib.h2hip_poseidon_spec_optimize(t, r_f, r_p, _ptr(rc), _ptr(m), _ptr(start), _ptr(partial), _ptr(end), _ptr(pre), _ptr(sparse))
    _raise_on(code, lib)
    return OptimizedSpec(start, partial[:r_p], end[:half - 1], m.reshape(t, t, 4).copy(), pre, sparse[:r_p])


def set_optimized_spec(ctx: Context, t: int, r_f: int, r_p: int, spec: OptimizedSpec) -> None:
    """h2hip_poseidon_set_optimized_spec: the spec fill_hashes writes traces of, resident on the context"""
    arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in spec]
    pad = np.zeros((1, 4), dtype=np.uint64)   # (an empty array still needs an address)
    ctx._chk(ctx.lib.h2hip_poseidon_set_optimized_spec(ctx.handle, t, r_f, r_p, *[_ptr(a if a.size else pad) for a in arrs]))


def trace_layout(t: int, r_f: int, r_p: int, length: int, flags: int = 0, lib=None):
    """h2hip_poseidon_trace_layout -> (cells one unit writes, the offsets of the t final-state cells inside them; [1] is the digest)"""
    lib = lib or load_library()
    n, offs = C.c_size_t(0), (C.c_uint32 * t)()
    code = lib.h2hip_poseidon_trace_layout(t, r_f, r_p, length, flags, C.byref(n), offs)
    _raise_on(code, lib)
    return n.value, list(offs)


def hash_table(units: Sequence) -> C.Array:
    """a ctypes table of h2hip_poseidon_hash from (column, row, input_offset, input_stride, flags) tuples: build it once for a layout used in
    every proof (a table of thousands of structs costs milliseconds to build)"""
    return (PoseidonHashStruct * max(len(units), 1))(*[PoseidonHashStruct(*[int(x) for x in u]) for u in units])


class PoseidonHasher:
    def __init__(self, ctx: Context, t: int, r_f: int, r_p: int):
        self.ctx, self.t, self.r_f, self.r_p = ctx, t, r_f, r_p
        self.round_constants, self.mds = poseidon_spec_generate(t, r_f, r_p, ctx.lib)
        self._optimized: Optional[OptimizedSpec] = None

    @classmethod
    def new(cls, ctx: Context, t: int, r_f: int, r_p: int) -> "PoseidonHasher":
        return cls(ctx, t, r_f, r_p)

    def _select(self):
        # the spec is resident per context: (re)select this hasher's before each batch, another hasher may share the context
        self.ctx.poseidon_set_spec(self.t, self.r_f, self.r_p, self.round_constants, self.mds)

    def hash_fix_len_array(self, inputs: np.ndarray) -> np.ndarray:
        """inputs (n, len, 4) -> digests (n, 4); one message (len, 4) -> one digest (4,)"""
        a = np.asarray(inputs, dtype=np.uint64)
        self._select()
        return self.ctx.poseidon_hash(a[None])[0] if a.ndim == 2 else self.ctx.poseidon_hash(a)

    def hash_var_len_array(self, inputs: np.ndarray, lens) -> np.ndarray:
        """inputs (n, max_len, 4), lens (n,) -> digests (n, 4) of inputs[i, :lens[i]]; one message (max_len, 4) with an integer len -> (4,)"""
        a = np.asarray(inputs, dtype=np.uint64)
        self._select()
        if a.ndim == 2:
            return self.ctx.poseidon_hash(a[None], np.array([lens], dtype=np.uint32))[0]
        return self.ctx.poseidon_hash(a, np.asarray(lens, dtype=np.uint32))

    def merkle_tree(self, leaves: np.ndarray) -> np.ndarray:
        self._select()
        return self.ctx.poseidon_merkle_tree(leaves)

    # ---- the in-circuit form
    def optimized_spec(self) -> OptimizedSpec:
        """OptimizedPoseidonSpec::new::<R_F, R_P, 0>() of this hasher, derived once"""
        if self._optimized is None:
            self._optimized = spec_optimize(self.t, self.r_f, self.r_p, self.round_constants, self.mds, self.ctx.lib)
        return self._optimized

    def select_optimized(self) -> None:
        """make this hasher's optimised spec the context's (fill_hashes does not: a caller with one hasher selects once, not per level)"""
        set_optimized_spec(self.ctx, self.t, self.r_f, self.r_p, self.optimized_spec())

    def trace_layout(self, length: int, flags: int = 0):
        return trace_layout(self.t, self.r_f, self.r_p, length, flags, self.ctx.lib)

    def fill_hashes(self, ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], inputs_dev, inputs_len: int,
                    length: int, hashes, states_in_dev=None, states_out_dev=None) -> None:
        """h2hip_poseidon_fill_hashes_dev: the gate cells of len(hashes) hash_fix_len_array units over `length` inputs each, written down the
        device columns `columns` from each unit's (column, row) across the break points, stream-ordered.  hashes: (column, row, input_offset,
        input_stride, flags) tuples or a table from hash_table() built once; input i of a unit is inputs_dev[input_offset + i * input_stride].
        select_optimized() must have been called on this context."""
        fill_hashes(ctx, columns, usable_rows, break_points, inputs_dev, inputs_len, length, hashes, states_in_dev, states_out_dev)


def fill_hashes(ctx: Context, columns: Sequence[int], usable_rows: int, break_points: Optional[Sequence[int]], inputs_dev, inputs_len: int, length: int,
                hashes, states_in_dev=None, states_out_dev=None) -> None:
    arr = _as_table(hashes, hash_table)
    ctx._chk(ctx.lib.h2hip_poseidon_fill_hashes_dev(ctx.handle, _col_array(columns), len(columns), usable_rows, _bp_array(break_points, len(columns)),
                                                    _dev_ptr(inputs_dev), inputs_len, length, _dev_ptr(states_in_dev), _dev_ptr(states_out_dev),
                                                    C.cast(arr, _vp), len(hashes)))
