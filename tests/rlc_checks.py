"""RLC circuits (h2hip_rlc_circuit_params: BaseConfig followed by RLC columns with the gate q_rlc * (a[r] * gamma + a[r+1] - a[r+2]), gamma =
challenge 0), shared by tests/test_rlc.py (the CPU-emulated build) and tests/test_rlc_gpu.py: every check takes a ctx.

  - the device fill h2hip_rlc_fill_chains_dev and the quotient kernel h2hip_quotient_rlc_gate_batch_dev against their definitions, computed here
    in Python integers;
  - RlcCircuit: the multi-phase test circuit of tests/phases_util.py with RLC columns, proven by libh2hip and by tests/shape_oracle.py on the
    same SRS and RNG stream;
  - soundness (a phase-1 witness computed from another gamma), the refusals, and that multi-phase keys prove as before.
"""
import ctypes as C

import numpy as np

from halo2_lib_amd import plonk as PL
from oracle import bn254 as O
from tests import phases_util as PU
from tests import shape_oracle as SO
from tests.dyn_lookup_util import rng_budget, srs, vk_from_gpu
from tests.phases_util import PhasedCircuit
from tests.shape_oracle import oracle_verify
from tests.util import PreDrawnRng, R, fr, full_range_fr, rand_fr

_vp = C.c_void_p
CARRY = PL.RLC_CARRY
ERR_INVALID = -1
SENTINEL = np.array([0xDEADBEEF0BADF00D, 0x0123456789ABCDEF, 0xFEEDFACECAFEBABE, 0x0FFFFFFFFFFFFFFF], dtype=np.uint64)   # (no Fr: never read as one)


FILL_GAMMAS = [0, 1, R - 1, 0x2B1A3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % R]
EMU_K = 7   # the emulated build's soundness, refusal and before / after checks (several keys and proofs each); its proof-byte checks run at k = 10


def _table(ptrs):
    return (_vp * max(len(ptrs), 1))(*[_vp(int(p)) for p in ptrs])


def _ints(limbs):
    return O.limbs_to_ints(np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4), R)


# ------------------------------------------------------------------------------------------------ the fill's definition
def rlc_cells(pieces, values, gamma):
    """{(column, row): value} of RlcChip::compute_rlc_fixed_len's cells for (column, row, len, flags, value_offset) pieces over integer values:
    a head piece is v_0, v_1, r_1, v_2, r_2, ...; a carry piece r_prev, v_0, r_0', v_1, r_1', ... with r_prev the last r of the piece before it"""
    cells, r = {}, None
    for (col, row, ln, flags, off) in pieces:
        v = values[off:off + ln]
        if flags & CARRY:
            cells[(col, row)] = r
            for i in range(ln):
                r = (r * gamma + v[i]) % R
                cells[(col, row + 2 * i + 1)] = v[i]
                cells[(col, row + 2 * i + 2)] = r
        else:
            r = v[0]
            cells[(col, row)] = r
            for i in range(1, ln):
                r = (r * gamma + v[i]) % R
                cells[(col, row + 2 * i - 1)] = v[i]
                cells[(col, row + 2 * i)] = r
    return cells


def fill_case():
    """The pieces of check 1 and their values.  Lengths 1, 2, 3; 255, 256, 257; 2047, 2048, 2049 (the scan's tile is 2048 values); one chain of
    70,001; 5,000 chains of lengths drawn from 1..40; a carry piece after a short head and one after the long head.  Two columns of 2^18 rows:
    these chains have 2 len - 1 cells each, about 354,000 in all, more than the 2^18 - 7 usable rows of one column, so the long chain and
    the carry pieces lie in column 1 and every other chain in column 0.  Values uniform over [0, r), offsets in shuffled order."""
    k = 18
    u = (1 << k) - 7
    g = np.random.default_rng(0x51C)
    lens = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049] + [int(v) for v in g.integers(1, 41, size=5000)]
    order = g.permutation(len(lens))
    pieces, row0, row1, off = [], 0, 0, 0
    # (list position matters only for carries: the long head and its carry first, so that the scan's first tiles hold one segment)
    pieces.append((1, row1, 70001, 0, off))
    row1, off = row1 + 2 * 70001 - 1, off + 70001
    pieces.append((1, row1 + 3, 3000, CARRY, off))          # carry after the long head, three rows further down
    row1, off = row1 + 3 + 2 * 3000 + 1, off + 3000
    for j, idx in enumerate(order):
        ln = lens[idx]
        pieces.append((0, row0, ln, 0, off))
        row0, off = row0 + 2 * ln - 1 + (j % 3), off + ln   # gaps of 0..2 untouched rows between chains
        if j == 7:                                           # carry after a short head: continues chain j in column 1
            pieces.append((1, row1 + 1, 5, CARRY, off))
            row1, off = row1 + 1 + 11, off + 5
    assert row0 <= u and row1 <= u, (row0, row1, u)
    # a second reference to an earlier value range (a chain may re-read values) and a one-value carry
    pieces.append((1, row1 + 2, 4, 0, 17))
    pieces.append((1, row1 + 2 + 7 + 2, 1, CARRY, 99))
    assert row1 + 2 + 7 + 2 + 3 <= u
    return k, u, pieces, off


def check_fill(ctx, gamma):
    """h2hip_rlc_fill_chains_dev over fill_case(): every addressed cell equals the Horner value, every other cell keeps the sentinel"""
    k, u, pieces, nvals = fill_case()
    n = 1 << k
    raw = full_range_fr(nvals, 0xA11)
    values = _ints(raw)
    cells = rlc_cells(pieces, values, gamma % R)
    want = [np.tile(SENTINEL, (n, 1)), np.tile(SENTINEL, (n, 1))]
    for c in (0, 1):
        rows = sorted(r for (cc, r) in cells if cc == c)
        want[c][rows] = fr([cells[(c, r)] for r in rows])
    sent = np.tile(SENTINEL, (n, 1))
    d_cols = [ctx.to_device(sent), ctx.to_device(sent)]
    d_vals = ctx.to_device(raw)
    try:
        PL.rlc_fill_chains(ctx, d_cols, u, d_vals, pieces, gamma, num_values=nvals)
        ctx.sync()
        for c in (0, 1):
            got = ctx.download(d_cols[c], (n, 4))
            if not np.array_equal(got, want[c]):
                bad = np.nonzero((got != want[c]).any(axis=1))[0]
                raise AssertionError("column %d: %d cells differ, first rows %s (gamma = %#x)" % (c, len(bad), bad[:8].tolist(), gamma))
    finally:
        for p in d_cols + [d_vals]:
            ctx.free(p)


def check_fill_rejections(ctx):
    """every refusal of h2hip_rlc_fill_chains_dev: H2HIP_ERR_INVALID, the sentinel everywhere, and the context fills correctly afterwards"""
    import halo2_lib_amd as H

    n, u, nvals = 64, 57, 40
    raw = full_range_fr(nvals, 0xB22)
    sent = np.tile(SENTINEL, (n, 1))
    d_cols = [ctx.to_device(sent), ctx.to_device(sent)]
    d_vals = ctx.to_device(raw)
    ok = (0, 0, 3, 0, 0)
    bad = {
        "column index out of range": [ok, (2, 0, 3, 0, 0)],
        "head leaves the usable rows": [ok, (1, u - 4, 3, 0, 0)],          # 5 cells from row u - 4
        "carry leaves the usable rows": [ok, (1, u - 6, 3, CARRY, 0)],     # 7 cells from row u - 6
        "len == 0": [ok, (1, 0, 0, 0, 0)],
        "values past num_values": [ok, (1, 0, 3, 0, nvals - 2)],
        "value offset past num_values": [ok, (1, 0, 1, 0, nvals + 1)],
        "carry on piece 0": [(0, 0, 3, CARRY, 0)],
    }
    try:
        for what, pieces in bad.items():
            try:
                PL.rlc_fill_chains(ctx, d_cols, u, d_vals, pieces, 5, num_values=nvals)
            except H.H2HipError as e:
                assert e.code == ERR_INVALID, (what, e.code)
            else:
                raise AssertionError("%s was accepted" % what)
            ctx.sync()
            for p in d_cols:
                assert np.array_equal(ctx.download(p, (n, 4)), sent), "%s: a cell was written" % what
        # the largest pieces that still fit, then everything is as the definition says
        pieces = [(0, u - 5, 3, 0, 0), (1, u - 7, 3, CARRY, 3), (0, 0, 1, 0, nvals - 1)]
        PL.rlc_fill_chains(ctx, d_cols, u, d_vals, pieces, 5, num_values=nvals)
        ctx.sync()
        cells = rlc_cells(pieces, _ints(raw), 5)
        for c in (0, 1):
            want = sent.copy()
            rows = sorted(r for (cc, r) in cells if cc == c)
            want[rows] = fr([cells[(c, r)] for r in rows])
            assert np.array_equal(ctx.download(d_cols[c], (n, 4)), want), "column %d after the refusals" % c
    finally:
        for p in d_cols + [d_vals]:
            ctx.free(p)


# ------------------------------------------------------------------------------------------------ the quotient kernel's definition
def check_quotient_rlc_gate(ctx, ek, k, count, sampled=None):
    """h2hip_quotient_rlc_gate_batch_dev against acc = acc * y + q_j[i] * (a_j[i] * gamma + a_j[i + s] - a_j[i + 2 s]) folded over the jobs in
    order, in Python integers, from a non-zero accumulator.  sampled = None: every point; else that many random points plus the last 2 s
    points, where the rotations wrap."""
    ne, s = 1 << ek, 1 << (ek - k)
    acc0 = rand_fr(ne, 900 + ek)
    # distinct (q, a) pairs would be 130 columns at count = 65: the jobs are distinct pairs drawn from a pool of at most 9 columns
    pool = [rand_fr(ne, 1000 + 10 * ek + 2 * j) for j in range(min(2 * count, 9))]
    pairs = [(q, a) for q in range(len(pool)) for a in range(len(pool))]
    jobs = [pairs[int(i)] for i in np.random.default_rng(count).permutation(len(pairs))[:count]]
    assert len(jobs) == count
    ch = rand_fr(2, 77 + ek)
    gamma, y = _ints(ch[0:1])[0], _ints(ch[1:2])[0]
    if sampled is None:
        pts = np.arange(ne)
    else:
        pts = np.unique(np.concatenate([np.random.default_rng(ek).integers(0, ne, size=sampled), np.arange(ne - 2 * s, ne)]))
    acc = _ints(acc0[pts])
    at = [[_ints(c[(pts + r * s) % ne]) for r in range(3)] for c in pool]
    for (qi, ai) in jobs:
        q, (a0, a1, a2) = at[qi][0], at[ai]
        acc = [(v * y + q[i] * (a0[i] * gamma + a1[i] - a2[i])) % R for i, v in enumerate(acc)]
    want = fr(acc)
    d_pool = [ctx.to_device(c) for c in pool]
    d_acc = ctx.to_device(acc0)
    try:
        ctx._chk(ctx.lib.h2hip_quotient_rlc_gate_batch_dev(ctx.handle, _vp(d_acc), _table([d_pool[q] for q, _ in jobs]), _table([d_pool[a] for _, a in jobs]),
                                                           count, ek, k, ch[0:1].ctypes.data_as(_vp), ch[1:2].ctypes.data_as(_vp)))
        got = ctx.download(d_acc, (ne, 4))[pts]
        if not np.array_equal(got, want):
            bad = pts[np.nonzero((got != want).any(axis=1))[0]]
            raise AssertionError("rlc gate (%d, %d) x %d: %d points differ, first %s" % (ek, k, count, len(bad), bad[:8].tolist()))
    finally:
        for p in d_pool + [d_acc]:
            ctx.free(p)


# ------------------------------------------------------------------------------------------------ the test circuit
class RlcCircuit(PhasedCircuit):
    """PhasedCircuit(params.base) plus the RLC columns.  RLC column j (advice index rlc[j]) holds, from row 0: the chain [1, 0], whose third
    cell is gamma (1 and 0 are copies of constants); a chain over copies of non-zero phase-0 cells; a chain whose head piece is followed by a
    carry piece in column (j + 1) mod nr, the break cell copied; and a long chain down to the end of the usable rows.  q_rlc is enabled on every
    row that starts a (r, v, r') triple, row 0 included.  Every gamma cell equals column 0's; a phase-1 flex-gate column takes its gamma cell
    (which it multiplies by) from there: the sound form of phases_util.PhasedCircuit."""

    GAMMA_ROW = 2

    def __init__(self, params: PL.RlcCircuitParams, seed: int, instance: bool = False):
        super().__init__(params.base, seed, instance=instance)
        self.rparams = params
        self.params = params
        self.sh = SO.Shape.rlc(params)
        self.phase_cols = self.sh.phase_cols
        self.nr = params.num_rlc_advice
        self.rlc = list(self.sh.rlc_advice)
        u = self.u
        src = [i for i, v in enumerate(self.small[0]) if v != 0]     # the phase-0 cells the chains copy are non-zero: every r then depends on gamma
        assert len(src) >= 8
        self.values, self.value_cells, self.pieces = [1, 0], [None, None], []
        g = np.random.default_rng(seed + 5)

        def take(ln):
            off = len(self.values)
            for i in g.integers(0, len(src), size=ln):
                self.values.append(self.small[0][src[int(i)]])
                self.value_cells.append(src[int(i)])
            return off

        long_len = (u - 28 - 2) // 2
        for j in range(self.nr):
            self.pieces.append((j, 0, 2, 0, 0))
            self.pieces.append((j, 3, 5, 0, take(5)))
            self.pieces.append((j, 12, 3, 0, take(3)))
            self.pieces.append(((j + 1) % self.nr, 20, 2, CARRY, take(2)))
            self.pieces.append((j, 28, long_len, 0, take(long_len)))
        assert 28 + 2 * long_len - 1 <= u - 1
        # copies: the chains' value cells, the constants, the break cells, the gamma cells
        one_row, zero_row = 1, 0
        const = ("fixed", self.sh.constant_cols[0])
        self.gate_rows = {j: [] for j in range(self.nr)}
        prev = None
        for (j, row, ln, flags, off) in self.pieces:
            col = ("advice", self.rlc[j])
            carry = bool(flags & CARRY)
            vrows = [row + 2 * i + 1 for i in range(ln)] if carry else [row] + [row + 2 * i - 1 for i in range(1, ln)]
            for i, vr in enumerate(vrows):
                cell = self.value_cells[off + i]
                if cell is None:
                    self.copies.append(((col, vr), (const, one_row if self.values[off + i] == 1 else zero_row)))
                else:
                    self.copies.append(((col, vr), (("advice", 0), cell)))
            if carry:
                pj, prow, pln, pflags, _ = prev
                last = prow + (2 * pln if pflags & CARRY else 2 * pln - 2)
                self.copies.append(((col, row), (("advice", self.rlc[pj]), last)))
                self.gate_rows[j] += [row + 2 * i for i in range(ln)]
            else:
                self.gate_rows[j] += [row + 2 * i for i in range(ln - 1)]
            prev = (j, row, ln, flags, off)
        for j in range(1, self.nr):
            self.copies.append(((("advice", self.rlc[j]), self.GAMMA_ROW), (("advice", self.rlc[0]), self.GAMMA_ROW)))
        for c in range(self.G):
            if self.gate_phase[c] == 1:   # the phase-1 flex gate's gamma cell (copied along that column) is the RLC gate's
                self.copies.append(((("advice", c), 2), (("advice", self.rlc[0]), self.GAMMA_ROW)))
        self.fixed = self._fixed()

    def _fixed(self):
        if not hasattr(self, "gate_rows"):
            return None
        sh = self.sh
        base = super()._fixed()                       # (sized by self.sh: the q_rlc columns come out zero)
        one = fr([1])[0]
        base[sh.constant_cols[0]][1] = one            # constants: row 0 holds 0, row 1 holds 1
        for j, qc in enumerate(sh.q_rlc_cols):
            base[qc][self.gate_rows[j]] = one
        return base

    def rlc_columns(self, gamma):
        """the RLC columns' integer values for this gamma"""
        cells = rlc_cells(self.pieces, self.values, gamma % R)
        cols = [[0] * self.n for _ in range(self.nr)]
        for (j, r), v in cells.items():
            cols[j][r] = v
        return cols

    def phase_values(self, phase, challenges):
        out = super().phase_values(phase, challenges) if phase < len(self.rparams.base.phase_columns()) else []
        base_cols = self.rparams.base.phase_columns()
        out = out[: len(base_cols[phase])] if phase < len(base_cols) else []
        if phase == 1:
            out = out + self.rlc_columns(challenges[0])
        return out

    def all_advice(self, challenges):
        """every advice column (advice index order) for check_witness"""
        cols = [None] * self.sh.num_advice_total
        for ph, pcols in enumerate(self.phase_cols):
            vals = self.phase_values(ph, list(challenges[: sum(self.sh.phase_challenges[:ph])]) if ph else [])
            for c, v in zip(pcols, vals):
                cols[c] = self._column(v)
        return cols

    def enabled_rlc_rows(self):
        """(advice index, row) of every enabled RLC gate, canonical order"""
        return [(self.rlc[j], r) for j in range(self.nr) for r in sorted(self.gate_rows[j])]


def shape_a(k, lookup_bits):
    """one phase-0 gate column with q_lookup, one RLC column"""
    return PL.RlcCircuitParams.new(k, [1], [1], 1, 0, lookup_bits, [1], 1), False


def shape_b(k, lookup_bits):
    """2 + 1 gate columns in phases 0 and 1, 1 + 1 lookup-advice columns, one instance column, two RLC columns"""
    return PL.RlcCircuitParams.new(k, [2, 1], [1, 1], 1, 1, lookup_bits, [1], 2), True


def free(r):
    r["gpk"].free()
    r["kzg"].free()


def check_proof_bytes(ctx, params, instance, seed, threads=2):
    """check 3: the library's proof equals the test prover's byte for byte; both verifiers accept it and reject a flipped bit"""
    r = PU.prove_both(ctx, params, seed, instance=instance, threads=threads, circuit=RlcCircuit)
    try:
        circ, got = r["circ"], r["got"]
        assert got == r["want"], "proof bytes differ from tests/shape_oracle.py's"
        assert r["seen"][0][0] == 1 and len(r["seen"][0][1]) >= 1
        inst = circ.instance_arrays()
        assert oracle_verify(r["params"], r["vk"], circ.instances, got), "the test verifier rejects the proof"
        assert PL.verify_proof(r["gpk"], inst, got), "h2hip_plonk_verify_proof_rlc rejects the proof"
        total, fails = PL.check_witness(r["gpk"], circ.all_advice(r["seen"][0][1]), inst, challenges=r["seen"][0][1])
        assert total == 0, fails
        bad = bytearray(got)
        bad[32 * len(circ.phase_cols[0]) + 32 * (len(circ.phase_cols[1]) - 1) + 3] ^= 1   # the last RLC column's commitment
        assert not oracle_verify(r["params"], r["vk"], circ.instances, bytes(bad))
        assert not PL.verify_proof(r["gpk"], inst, bytes(bad))
    finally:
        free(r)


def check_soundness(ctx, k, lookup_bits, seed):
    """check 4 on shape A: phase 1 computed from gamma + 1 proves but does not verify, and check_witness names exactly the enabled RLC rows"""
    params, inst = shape_a(k, lookup_bits)
    circ_box = []

    def cheat(phase, challenges):   # the prover picks another gamma: nothing but the RLC gate ties the cells to the transcript's challenge
        c = circ_box[0]
        c.gamma_seen.append((phase, list(challenges)))
        return [c._column(v) for v in c.phase_values(phase, [(challenges[0] + 1) % R] + list(challenges[1:]))]

    circ = RlcCircuit(params, seed, instance=inst)
    circ_box.append(circ)
    kzg, srs_params = srs(ctx, params.k, seed)
    gpk = PL.keygen(kzg, params, circ.fixed, circ.copies)
    try:
        budget = rng_budget(circ.sh)
        proof = PL.create_proof(gpk, circ.advice0(), [], PreDrawnRng(budget, 3 + seed), phase_witness=cheat)
        gamma = circ.gamma_seen[-1][1][0]
        vk = vk_from_gpu(circ.sh, gpk)
        assert not PL.verify_proof(gpk, [], proof), "h2hip_plonk_verify_proof_rlc accepts a proof made with another gamma"
        assert not oracle_verify(srs_params, vk, [], proof), "the test verifier accepts a proof made with another gamma"
        want = circ.enabled_rlc_rows()
        total, fails = PL.check_witness(gpk, circ.all_advice([(gamma + 1) % R]), [], max_failures=len(want) + 8, challenges=[gamma])
        assert total == len(want) and [(f.kind, f.column, f.row) for f in fails] == [("gate", c, r) for c, r in want]
        # the honest witness: zero failures, a proof both verifiers accept
        good = circ.all_advice([gamma])
        assert PL.check_witness(gpk, good, [], challenges=[gamma])[0] == 0
        proof = PL.create_proof(gpk, circ.advice0(), [], PreDrawnRng(budget, 3 + seed), phase_witness=circ.witness)
        assert PL.verify_proof(gpk, [], proof) and oracle_verify(srs_params, vk, [], proof)
        # one flipped r_i: the gate that produces it and the gate that consumes it; at a chain's end only the first
        col = circ.rlc[0]
        for row, expect in ((7, [5, 7]), (11, [9])):   # the chain at rows 3..11: r_2 at row 7, the last r at row 11
            bad = [c.copy() for c in good]
            bad[col][row, 0] ^= np.uint64(1)
            total, fails = PL.check_witness(gpk, bad, [], challenges=[gamma])
            gates = [(f.column, f.row) for f in fails if f.kind == "gate"]
            assert gates == [(col, r) for r in expect], (row, gates)
            assert total == len(expect) + sum(f.kind == "copy" for f in fails)
    finally:
        gpk.free()
        kzg.free()


def check_limits(ctx, k, lookup_bits, seed):
    """check 5: the refusals, each H2HIP_ERR_INVALID, and a correct proof from the same context (and, where one exists, key) afterwards"""
    import halo2_lib_amd as H

    def invalid(fn, what):
        try:
            fn()
        except H.H2HipError as e:
            assert e.code == ERR_INVALID, (what, e.code, str(e))
            return str(e)
        raise AssertionError("%s was accepted" % what)

    new = PL.RlcCircuitParams.new
    invalid(lambda: PL.shape_of(ctx, new(k, [1], [1], 1, 0, lookup_bits, [1], 0)), "num_rlc_advice = 0")
    invalid(lambda: PL.shape_of(ctx, new(k, [1], [1], 1, 0, lookup_bits, [1], 65)), "num_rlc_advice = 65")
    invalid(lambda: PL.shape_of(ctx, new(k, [1], [1], 1, 0, lookup_bits, [0], 1)), "no challenge after phase 0")
    invalid(lambda: PL.shape_of(ctx, new(k, [1], [1], 1, 0, lookup_bits, [0, 1], 1)), "the only challenge after phase 1")
    assert PL.shape_of(ctx, new(k, [1], [1], 1, 0, lookup_bits, [1], 64)).num_advice_total == 65
    # phase 2 has columns and phase 1 only the RLC columns: contiguous, because they count
    assert PL.shape_of(ctx, new(k, [1, 0, 1], [1, 0, 0], 1, 0, lookup_bits, [1, 1], 1)).num_advice_total == 3
    params, _ = shape_b(k, lookup_bits)
    circ = RlcCircuit(params, seed, instance=True)
    kzg, srs_params = srs(ctx, k, seed)
    one = fr([1])[0]
    try:
        fx = [c.copy() for c in circ.fixed]
        fx[circ.sh.q_rlc_cols[1]][circ.u - 2] = one
        assert "q_rlc" in invalid(lambda: PL.keygen(kzg, params, fx, circ.copies), "q_rlc on row usable_rows - 2")
        fx = [c.copy() for c in circ.fixed]
        fx[circ.sh.q_rlc_cols[0]][:] = 0
        fx[circ.sh.q_rlc_cols[0]][1] = one           # row 1: none of the q_enable columns (rows 0, 4, 8, ...) shares it
        invalid(lambda: PL.keygen(kzg, params, fx, circ.copies), "a q_rlc disjoint from a q_enable")
        gpk = PL.keygen(kzg, params, circ.fixed, circ.copies)
        try:
            def _allgather(_user, local, nbytes, out):
                C.memmove(out, local, nbytes)
                return 0

            cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(_allgather)
            comm = C.c_void_p()
            ctx._chk(ctx.lib.h2hip_comm_init_callback(1, 0, C.cast(cb, C.c_void_p), None, C.byref(comm)))
            try:
                rc = ctx.lib.h2hip_plonk_pk_set_sharding(gpk.handle, comm, kzg.g.handle, kzg.g_lagrange.handle, 0, 1 << k, 0xFFFF)
                assert rc == ERR_INVALID and b"one GPU" in ctx.lib.h2hip_last_error(), rc
            finally:
                ctx.lib.h2hip_comm_destroy(comm)
            adv0, inst = circ.advice0(), circ.instance_arrays()
            budget = rng_budget(circ.sh)
            arr = (_vp * len(adv0))(*[_vp(c.ctypes.data) for c in adv0])
            ip = (_vp * 1)(_vp(inst[0].ctypes.data))
            il = (C.c_size_t * 1)(len(inst[0]))
            buf = np.zeros(gpk.proof_size(), dtype=np.uint8)
            plen = C.c_size_t(0)
            rng = PL.ChaChaRng(ctx.lib, 1)
            rc = ctx.lib.h2hip_plonk_create_proof(ctx.handle, gpk.handle, arr, 0, ip, il, C.cast(ctx.lib.h2hip_chacha_rng_fill, _vp),
                                                  C.cast(C.pointer(rng.state), _vp), buf.ctypes.data_as(_vp), buf.nbytes, C.byref(plen), None)
            assert rc == ERR_INVALID, rc
            proof = PL.create_proof(gpk, adv0, inst, PreDrawnRng(budget, 9), phase_witness=circ.witness)
            gamma = circ.gamma_seen[-1][1]
            full = circ.all_advice(gamma)
            msg = invalid(lambda: PL.check_witness(gpk, full, inst), "h2hip_plonk_check_witness on an RLC key")
            assert "h2hip_plonk_check_witness_challenges" in msg
            invalid(lambda: PL.check_witness(gpk, full, inst, challenges=[]), "check_witness without challenge 0")
            # the key and the context prove a correct witness afterwards
            assert PL.check_witness(gpk, full, inst, challenges=gamma)[0] == 0
            again = PL.create_proof(gpk, adv0, inst, PreDrawnRng(budget, 9), phase_witness=circ.witness)
            assert again == proof and PL.verify_proof(gpk, inst, again)
            assert oracle_verify(srs_params, vk_from_gpu(circ.sh, gpk), circ.instances, again)
        finally:
            gpk.free()
    finally:
        kzg.free()


def check_phased_keys_unmoved(ctx, k, lookup_bits):
    """check 6: a multi-phase key (h2hip_plonk_keygen_phased) proven before and after RLC proofs on the same context: identical bytes"""
    pparams, _ = PU.shape_params("a", k, lookup_bits)
    pc = PU.PhasedCircuit(pparams, 31)
    kzg, _ = srs(ctx, k, 31)
    ppk = PL.keygen(kzg, pparams, pc.fixed, pc.copies)
    try:
        budget = rng_budget(pc.sh)
        before = PL.create_proof(ppk, pc.advice0(), [], PreDrawnRng(budget, 12), phase_witness=pc.witness)
        assert PL.verify_proof(ppk, [], before)
        for params, inst in (shape_a(k, lookup_bits), shape_b(k, lookup_bits)):
            r = PU.prove_both(ctx, params, 40 + params.num_rlc_advice, instance=inst, oracle_prover=False, circuit=RlcCircuit)
            try:
                assert PL.verify_proof(r["gpk"], r["circ"].instance_arrays(), r["got"])
            finally:
                free(r)
        after = PL.create_proof(ppk, pc.advice0(), [], PreDrawnRng(budget, 12), phase_witness=pc.witness)
        assert after == before
        assert PL.check_witness(ppk, _phased_advice(pc), [])[0] == 0
    finally:
        ppk.free()
        kzg.free()


def _phased_advice(pc):
    """every advice column of a PhasedCircuit (advice index order) for the challenges its last proof saw"""
    cols = [None] * pc.sh.num_advice_total
    seen = {ph: ch for ph, ch in pc.gamma_seen}
    for ph, pcols in enumerate(pc.phase_cols):
        for c, v in zip(pcols, pc.phase_values(ph, seen.get(ph, []))):
            cols[c] = pc._column(v)
    return cols


def check_device_fill_proof(ctx, k, lookup_bits, seed):
    """shape B with phase 1 written on the device — the RLC columns by rlc_fill_chains from values resident before the proof, the other
    phase-1 columns uploaded in place — gives the bytes of the same proof with host-computed columns"""
    params, inst = shape_b(k, lookup_bits)
    r = PU.prove_both(ctx, params, seed, instance=inst, oracle_prover=False, circuit=RlcCircuit)
    circ, gpk = r["circ"], r["gpk"]
    d_vals = ctx.to_device(fr(circ.values))
    calls = []
    try:
        assert PL.verify_proof(gpk, circ.instance_arrays(), r["got"]) and oracle_verify(r["params"], r["vk"], circ.instances, r["got"])

        def on_device(phase, challenges, ptrs):
            assert phase == 1 and len(ptrs) == len(circ.phase_cols[1])
            others = circ.phase_values(1, challenges)[: len(ptrs) - circ.nr]
            for p, v in zip(ptrs, others):
                ctx.upload(p, np.ascontiguousarray(circ._column(v)[: circ.u]))
            PL.rlc_fill_chains(ctx, ptrs[len(ptrs) - circ.nr:], circ.u, d_vals, circ.pieces, challenges[0], num_values=len(circ.values))
            calls.append(phase)

        got = PL.create_proof(gpk, circ.advice0(), circ.instance_arrays(), PreDrawnRng(r["budget"], 1000 + seed), phase_witness_dev=on_device)
        assert calls == [1]
        assert got == r["got"], "the proof with device-filled RLC columns differs from the one with host-computed columns"
    finally:
        ctx.free(d_vals)
        free(r)


def check_struct_layouts():
    """h2hip_rlc_circuit_params and h2hip_rlc_chain: the same fields in the header, the Rust sys crate and ctypes"""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "h2hip.h")).read()
    rs = open(os.path.join(root, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    cmap = {"uint32_t": "u32", "uint64_t": "u64", "h2hip_phased_circuit_params": "h2hip_phased_circuit_params"}

    def py(t):
        return {C.c_uint32: "u32", C.c_uint64: "u64", PL.PhasedCircuitParams: "h2hip_phased_circuit_params"}[t]

    for name, cls in (("h2hip_rlc_circuit_params", PL.RlcCircuitParams), ("h2hip_rlc_chain", PL.RlcChainStruct)):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s\s*;" % (name, name), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        c_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                ty, names = decl.split(None, 1)
                c_fields += [(nm.strip(), cmap[ty]) for nm in names.split(",")]
        rs_body = re.search(r"pub struct %s\s*\{(.*?)\}" % name, rs, flags=re.S).group(1)
        rs_fields = [(m.group(1), m.group(2) or "%sx%s" % (m.group(3), m.group(4)))
                     for m in re.finditer(r"pub ([a-z_]+): (?:([a-z0-9_]+)|\[([a-z0-9]+); (\d+)\])", rs_body)]
        py_fields = [(n, py(t)) for n, t in cls._fields_]
        assert c_fields == py_fields, (name, c_fields, py_fields)
        if name == "h2hip_rlc_circuit_params":   # the Rust struct holds the nested struct's fields in place (the same layout)
            flat = lambda t: ("%sx%d" % (flat(t._type_), t._length_)) if issubclass(t, C.Array) else {C.c_uint32: "u32", C.c_int32: "i32"}[t]
            c_fields = [(n, flat(t)) for n, t in PL.PhasedCircuitParams._fields_] + c_fields[1:]
        assert c_fields == rs_fields, (name, c_fields, rs_fields)
    assert re.search(r"#define H2HIP_RLC_CARRY 1\b", hdr) and "pub const H2HIP_RLC_CARRY: u32 = 1;" in rs and PL.RLC_CARRY == 1
