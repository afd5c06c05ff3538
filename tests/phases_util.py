"""Shared by the multi-phase tests (CPU-emulated and GPU): a BaseConfig circuit whose later phases hold RLC chains over the earlier phases'
cells, proven by libh2hip (h2hip_plonk_create_proof_phased) and by the test-side CPU prover (tests/shape_oracle.py) on the same SRS and RNG
stream.

Layout of the circuit (every gate column is enabled on row 0, so keygen's selector rule holds):
  - a phase-0 gate column holds blocks [a, b, c, a + b*c] of small values (all of them inside the range table);
  - a gate column of phase p > 0 holds blocks [v_i, rlc_i, gamma, rlc_{i+1}] with rlc_{i+1} = v_i + rlc_i * gamma: v_i is a copy of a cell of
    phase p - 1, gamma is the last challenge squeezed so far (a constant when there is none) and is copied along the column, rlc_{i+1} is
    copied into the next block;
  - a dedicated lookup-advice column holds copies of phase-0 gate column 0's first cells (range-checked).
"""
import numpy as np

from halo2_lib_amd import plonk as PL
from oracle import bn254 as O
from tests import shape_oracle as SO
from tests.dyn_lookup_util import oracle_pk, rng_budget, srs, vk_from_gpu
from tests.shape_oracle import oracle_verify
from tests.util import PreDrawnRng, R

NO_CHALLENGE_GAMMA = 7


class PhasedCircuit:
    def __init__(self, params: PL.PhasedCircuitParams, seed: int, instance: bool = False, bad_lookup: bool = False):
        self.params, self.seed, self.bad_lookup = params, seed, bad_lookup
        self.sh = SO.Shape.phased(params)
        sh = self.sh
        self.n, self.u = sh.n, sh.usable_rows
        self.blocks = self.u // 4
        self.phase_cols = sh.phase_cols
        g = list(params.num_advice_per_phase)
        self.gate_phase = [p for p in range(3) for _ in range(g[p])]       # phase of each gate column
        G = len(self.gate_phase)
        self.G = G
        self.lookup_cols = [c for c in range(G, sh.num_advice_total)]
        self.lookup_phase = {c: p for p, cols in enumerate(self.phase_cols) for c in cols if c >= G}
        self.gamma_seen = []                                                 # the challenges every witness call received
        rng = np.random.default_rng(seed)
        self.small = {}
        for c in range(G):
            if self.gate_phase[c] == 0:
                a, b, cc = (rng.integers(0, 4, size=self.blocks) for _ in range(3))
                vals = []
                for i in range(self.blocks):
                    vals += [int(a[i]), int(b[i]), int(cc[i]), int(a[i] + b[i] * cc[i])]
                self.small[c] = vals
        self.copies = []
        # later-phase gate columns: v_i copied from the column before it (index c - 1), the chain and gamma along the column
        for c in range(G):
            if self.gate_phase[c] == 0:
                continue
            for i in range(self.blocks):
                self.copies.append(((("advice", c), 4 * i), (("advice", c - 1), 4 * i + 3)))
                if i:
                    self.copies.append(((("advice", c), 4 * i + 2), (("advice", c), 2)))
                    self.copies.append(((("advice", c), 4 * i + 1), (("advice", c), 4 * i - 1)))
        self.nlk = min(8, self.blocks * 4)
        for c in self.lookup_cols:
            for j in range(self.nlk):
                self.copies.append(((("advice", c), j), (("advice", 0), j)))
        self.instances = []
        if instance:
            self.instances = [[self.small[0][3], self.small[0][0]]]
            self.copies.append(((("advice", 0), 3), (("instance", 0), 0)))
            self.copies.append(((("advice", 0), 0), (("instance", 0), 1)))
        self.fixed = self._fixed()

    def _fixed(self):
        sh, n = self.sh, self.n
        cols = [np.zeros(n, dtype=object) for _ in range(sh.num_fixed_total)]
        if self.params.lookup_bits >= 0 and sh.table_col is not None:
            cols[sh.table_col][: 1 << self.params.lookup_bits] = list(range(1 << self.params.lookup_bits))
        if sh.q_lookup_col is not None:
            cols[sh.q_lookup_col][: 4 * self.blocks] = 1
        for qc, _a in sh.gates:
            for i in range(self.blocks):
                cols[qc][4 * i] = 1
        return [O.ints_to_limbs([int(v) for v in c], R) for c in cols]

    def _column(self, vals):
        col = [0] * self.n
        col[: len(vals)] = [v % R for v in vals]
        return O.ints_to_limbs(col, R)

    def _gate_values(self, c, prev_vals, challenges):
        gamma = challenges[-1] if challenges else NO_CHALLENGE_GAMMA
        vals, rlc = [], 0
        for i in range(self.blocks):
            v = prev_vals[4 * i + 3]
            nxt = (v + rlc * gamma) % R
            vals += [v, rlc, gamma, nxt]
            rlc = nxt
        return vals

    def _lookup_values(self):
        vals = self.small[0][: self.nlk]
        if self.bad_lookup:
            vals = list(vals)
            vals[1] = 1 << 40   # outside the table (and unequal to its copy: the proof must not get that far)
        return vals

    def phase_values(self, phase, challenges):
        """the integer values of phase `phase`'s columns (index order) given the challenges so far"""
        out, vals = [], {}
        for c in range(self.G):
            if self.gate_phase[c] == 0:
                vals[c] = self.small[c]
        for p in range(phase + 1):
            for c in range(self.G):
                if self.gate_phase[c] == p and p > 0:
                    vals[c] = self._gate_values(c, vals[c - 1], challenges if p == phase else challenges[: self._ch_before(p)])
        for c in self.phase_cols[phase]:
            out.append(vals[c] if c < self.G else self._lookup_values() if self.lookup_phase.get(c) == phase else [])
        return out

    def _ch_before(self, p):
        return sum(self.sh.phase_challenges[:p])

    def advice0(self):
        return [self._column(v) for v in self.phase_values(0, [])]

    def witness(self, phase, challenges):
        self.gamma_seen.append((phase, list(challenges)))
        return [self._column(v) for v in self.phase_values(phase, challenges)]

    def instance_arrays(self):
        return [O.ints_to_limbs(v, R) for v in self.instances]


def prove_both(ctx, params, seed, instance=False, rng_seed=None, oracle_prover=True, threads=2, witness=None, circuit=PhasedCircuit):
    """keygen + create_proof on libh2hip and (oracle_prover) on the test prover, for a circuit class with PhasedCircuit's interface
    (rlc_checks.RlcCircuit).  -> dict(gpk, kzg, params, vk, got, want, circ, budget, seen, seed)"""
    circ = circuit(params, seed, instance=instance)
    kzg, srs_params = srs(ctx, params.k, seed)
    gpk = PL.keygen(kzg, params, circ.fixed, circ.copies)
    sh, gs = circ.sh, gpk.shape
    assert (gs.degree, gs.extended_k, gs.blinding_factors, gs.usable_rows, gs.num_perm_sets, gs.num_fixed_total, gs.num_advice_total, gs.num_lookups,
            gs.num_perm_columns) == (sh.degree, sh.extended_k, 6, sh.usable_rows, sh.num_perm_sets, sh.num_fixed_total, sh.num_advice_total,
                                     len(sh.lookups), len(sh.perm_columns))
    budget = rng_budget(sh)
    rs = 1000 + seed if rng_seed is None else rng_seed
    got = PL.create_proof(gpk, circ.advice0(), circ.instance_arrays(), PreDrawnRng(budget, rs), phase_witness=witness or circ.witness)
    lib_seen = list(circ.gamma_seen)
    want, vk = None, None
    if oracle_prover:
        pk = oracle_pk(sh, srs_params, circ.fixed, circ.copies, threads)
        assert pk.vk.transcript_repr == gpk.transcript_repr, "verifying keys differ (fixed / permutation commitments)"
        circ.gamma_seen.clear()
        want = SO.create_proof(srs_params, pk, circ.advice0(), circ.instances, PreDrawnRng(budget, rs), threads, phase_witness=circ.witness)
        assert circ.gamma_seen == lib_seen, "the witness callback saw different challenges (%s vs %s)" % (lib_seen, circ.gamma_seen)
        vk = pk.vk
    else:
        vk = vk_from_gpu(sh, gpk)
    return dict(gpk=gpk, kzg=kzg, params=srs_params, vk=vk, got=got, want=want, circ=circ, budget=budget, seen=lib_seen, seed=seed)


def first_phase1_commitment(circ) -> int:
    """byte offset of the first commitment of phase 1 in the proof (the advice commitments come phase by phase)"""
    return 32 * len(circ.phase_cols[0])


SHAPES = {
    "a": dict(g=[1, 1], la=[1, 1], ch=[1]),
    "b": dict(g=[2, 1], la=[0, 1], ch=[1]),
    "c": dict(g=[2, 1, 1], la=[1, 0, 1], ch=[1, 1, 0]),
    "d": dict(g=[1, 1], la=[1, 1], ch=[]),
    "e": dict(g=[1, 1], la=[1, 1], ch=[1], instance=True),
}


def shape_params(name, k, lookup_bits, num_fixed=1):
    s = SHAPES[name]
    return PL.PhasedCircuitParams.new(k, s["g"], s["la"], num_fixed, 1 if s.get("instance") else 0, lookup_bits, s["ch"]), s.get("instance", False)


__all__ = ["PhasedCircuit", "prove_both", "oracle_verify", "first_phase1_commitment", "SHAPES", "shape_params", "PreDrawnRng", "R"]
