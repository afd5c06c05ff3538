"""PoseidonHasher (halo2-base/src/poseidon/hasher/mod.rs) on the GPU, batched over messages: the reference's names over
h2hip_poseidon_spec_generate + h2hip_poseidon_set_spec + h2hip_poseidon_hash_batch_dev, so a caller brings no constants of their own."""
from __future__ import annotations

import numpy as np

from .h2hip import Context, poseidon_spec_generate


class PoseidonHasher:
    def __init__(self, ctx: Context, t: int, r_f: int, r_p: int):
        self.ctx, self.t, self.r_f, self.r_p = ctx, t, r_f, r_p
        self.round_constants, self.mds = poseidon_spec_generate(t, r_f, r_p, ctx.lib)

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
