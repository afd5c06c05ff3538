"""In-circuit Poseidon traces filled on the device (h2hip_poseidon_fill_hashes_dev: every flex-gate cell PoseidonHasher::hash_fix_len_array
writes), shared by tests/test_poseidon_trace.py (the CPU-emulated build) and tests/test_poseidon_trace_gpu.py: every check takes a ctx.

The definition is restated here in Python integers over halo2_lib_amd.virtual_region.Context: the optimised-spec derivation (hasher/spec.rs:
108-175, mds.rs:118-171), PoseidonState.permutation with len = None (hasher/state.rs:35-161, 214-250) and fix_len_array_squeeze (hasher/mod.rs:
344-361) on a chip with add, mul, mul_add, sum and inner_product in the reference's cell order (flex_gate/mod.rs:158-277, 412-435, 940-1010).

  0  the restatement itself: its final states equal the textbook sponge (tests/poseidon_hash_oracle.H over oracle/poseidon.py) and the golden KATs;
  A  the fill against the definition over sentinel-filled columns (a stray write fails), states_out and trace_layout alike;
  B  independent answers: the golden permutation KATs through states_in + ABSORB_ONLY, digests against hash_batch and H;
  C  h2hip_poseidon_spec_optimize against the Python derivation, element for element; the refusal of a row that begins with 1;
  D  column breaks: the same virtual run laid down by virtual_region.assign_witnesses and by the fill;
  E  every refusal: H2HIP_ERR_INVALID, its reason in h2hip_last_error, the columns untouched;
  F  a BaseConfig proof whose hash cells two fill calls write (the Merkle root of four leaves as the instance).
"""
import ctypes as C
import functools
import json
import os
import re

import numpy as np

import halo2_lib_amd as H
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import poseidon as PS
from halo2_lib_amd import virtual_region as VR
from oracle import bn254 as O
from oracle import plonk as P
from tests import poseidon_hash_oracle as PO
from tests.dyn_lookup_util import rng_budget, srs, vk_from_gpu
from tests.rlc_checks import SENTINEL
from tests.util import PreDrawnRng, R, fr, full_range_fr

_vp = C.c_void_p
AO, WC = PS.ABSORB_ONLY, PS.WITH_CONSTS
ERR_INVALID = -1
BLOCK = 64   # poseidon_trace.hip: units (lanes) per workgroup; the grid is one row of workgroups
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = VR.GateChip


def _ints(limbs):
    return O.limbs_to_ints(np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4), R)


# ------------------------------------------------------------------------------------------------ the optimised spec, in integers
def _mat_mul(a, b):
    t = len(a)
    return [[sum(a[i][k] * b[k][j] for k in range(t)) % R for j in range(t)] for i in range(t)]


def _mat_vec(a, v):
    return [sum(x * y for x, y in zip(row, v)) % R for row in a]


def _transpose(a):
    return [list(r) for r in zip(*a)]


def _det(m):
    """Laplace expansion (t - 1 <= 4): deliberately not the elimination the library uses"""
    if len(m) == 1:
        return m[0][0] % R
    return sum((-1) ** j * m[0][j] * _det([row[:j] + row[j + 1:] for row in m[1:]]) for j in range(len(m))) % R


def _inverse(m):
    """adjugate / determinant"""
    t, d = len(m), pow(_det(m), -1, R)
    minor = lambda i, j: [row[:j] + row[j + 1:] for k, row in enumerate(m) if k != i]
    return [[(-1) ** (i + j) * _det(minor(j, i)) * d % R for j in range(t)] for i in range(t)]


def _factorise(m):
    """mds.rs:118-171 -> (M', (row, col_hat)): w_hat by Cramer's rule, as there"""
    t = len(m)
    w = [m[i][0] for i in range(1, t)]
    hat = [row[1:] for row in m[1:]]
    dinv = pow(_det(hat), -1, R)
    w_hat = []
    for j in range(t - 1):
        hj = [row[:] for row in hat]
        for i in range(t - 1):
            hj[i][j] = w[i]
        w_hat.append(_det(hj) * dinv % R)
    prime = [[1 if i == j else 0 for j in range(t)] for i in range(t)]
    for i in range(t - 1):
        for j in range(t - 1):
            prime[i + 1][j + 1] = hat[i][j]
    return prime, ([m[0][0]] + w_hat, m[0][1:])


class OptSpec:
    """OptimizedPoseidonSpec from the textbook arrays (spec.rs:108-175)"""

    def __init__(self, t, r_f, r_p, constants, mds):
        self.t, self.r_f, self.r_p, self.mds = t, r_f, r_p, [list(r) for r in mds]
        half, inv = r_f // 2, _inverse(mds)
        self.start = [list(constants[0])] + [_mat_vec(inv, constants[r]) for r in range(1, half)]
        acc = list(constants[half + r_p])
        self.partial = [0] * r_p
        for i in range(r_p):
            tmp = _mat_vec(inv, acc)
            self.partial[r_p - 1 - i] = tmp[0]
            tmp[0] = 0
            acc = [(a + c) % R for a, c in zip(tmp, constants[half + r_p - 1 - i])]
        self.start.append(_mat_vec(inv, acc))
        self.end = [_mat_vec(inv, constants[r]) for r in range(half + r_p + 1, r_f + r_p)]
        mt = _transpose(mds)
        a, sparse = mt, []
        for _ in range(r_p):
            prime, pp = _factorise(a)
            a = _mat_mul(mt, prime)
            sparse.append(pp)
        self.sparse = sparse[::-1]
        self.pre_sparse_mds = _transpose(a)

    def arrays(self):
        """the six arrays of halo2_lib_amd.poseidon.OptimizedSpec, Montgomery limbs"""
        t = self.t
        lim = lambda vals, *shape: fr(vals).reshape(shape + (4,)) if vals else np.zeros(shape + (4,), dtype=np.uint64)
        flat = lambda rows: [v for row in rows for v in row]
        return PS.OptimizedSpec(lim(flat(self.start), len(self.start), t), lim(self.partial, self.r_p), lim(flat(self.end), len(self.end), t),
                                lim(flat(self.mds), t, t), lim(flat(self.pre_sparse_mds), t, t),
                                lim([v for row, hat in self.sparse for v in row + hat], self.r_p, 2 * t - 1))


@functools.lru_cache(maxsize=None)
def opt_spec(t):
    sp = PO.spec(t)
    return OptSpec(t, sp.r_f, sp.r_p, sp.constants, sp.mds)


# ------------------------------------------------------------------------------------------------ the trace's definition
def chip_sum(ctx, a):
    """GateInstructions::sum (flex_gate/mod.rs:412-435): | a0 | a1 1 a0+a1 | a2 1 a0+a1+a2 | ..."""
    a = [VR._q(v) for v in a]
    if not a:
        return ctx.load_zero()
    if len(a) == 1:
        return ctx.assign_region_last([a[0]], [])
    s, cells = a[0].value, [a[0]]
    for x in a[1:]:
        s = (s + x.value) % R
        cells += [x, VR.Constant(1), VR.Witness(s)]
    return ctx.assign_region_last(cells, [3 * i for i in range(len(a) - 1)])


def chip_inner_product(ctx, a, b):
    """GateChip::inner_product; the right operand of a Poseidon matrix row never starts with Constant(1)"""
    assert not (isinstance(b[0], VR.Constant) and b[0].value == 1)
    return G.inner_product(ctx, a, b)


def _default_state(ctx, t):
    """PoseidonState::default (state.rs:20-27)"""
    return [ctx.load_constant(v) for v in PO.init_state(t)]


def _x5(ctx, x, c):
    x2 = G.mul(ctx, x, x)
    x4 = G.mul(ctx, x2, x2)
    return G.mul_add(ctx, x, x4, VR.Constant(c))


def _apply_mds(ctx, s, m):
    return [chip_inner_product(ctx, list(s), [VR.Constant(c) for c in row]) for row in m]


def permutation(ctx, s, inputs, o):
    """PoseidonState::permutation(inputs, None) (state.rs:35-83): s and inputs are AssignedValues; returns the new state"""
    t, half = o.t, o.r_f // 2
    s = list(s)
    pre = o.start[0]
    s[0] = G.add(ctx, s[0], VR.Constant(pre[0]))
    for i, inp in enumerate(inputs):
        s[i + 1] = chip_sum(ctx, [VR.Existing(s[i + 1]), VR.Existing(inp), VR.Constant(pre[i + 1])])
    for i, k in enumerate(range(len(inputs) + 1, t)):
        s[k] = G.add(ctx, s[k], VR.Constant((1 + pre[k]) % R if i == 0 else pre[k]))
    for r in range(1, half):
        s = [_x5(ctx, x, c) for x, c in zip(s, o.start[r])]
        s = _apply_mds(ctx, s, o.mds)
    s = [_x5(ctx, x, c) for x, c in zip(s, o.start[half])]
    s = _apply_mds(ctx, s, o.pre_sparse_mds)
    for c, (row, hat) in zip(o.partial, o.sparse):
        s[0] = _x5(ctx, s[0], c)
        first = chip_inner_product(ctx, list(s), [VR.Constant(v) for v in row])
        s = [first] + [G.mul_add(ctx, s[0], VR.Constant(h), x) for h, x in zip(hat, s[1:])]
    for cs in o.end:
        s = [_x5(ctx, x, c) for x, c in zip(s, cs)]
        s = _apply_mds(ctx, s, o.mds)
    s = [_x5(ctx, x, 0) for x in s]
    return _apply_mds(ctx, s, o.mds)


def fix_len_array_squeeze(ctx, s, inputs, o, absorb_only=False):
    """hasher/mod.rs:344-361; absorb_only leaves out the permutation of the empty chunk (the compact-chunk forms, mod.rs:262-288)"""
    rate = o.t - 1
    for at in range(0, len(inputs), rate):
        s = permutation(ctx, s, inputs[at:at + rate], o)
    if len(inputs) % rate == 0 and not absorb_only:
        s = permutation(ctx, s, [], o)
    return s


def unit_trace(t, inputs, flags, state_in=None):
    """-> (the unit's cells in order, its final state, the offsets of the final-state cells) for integer inputs, by the definition"""
    o = opt_spec(t)
    ctx = VR.Context(True, "trace", 0, VR.CopyConstraintManager())
    s = _default_state(ctx, t) if flags & WC else [VR.AssignedValue(v) for v in PO.init_state(t)]
    if state_in is not None:
        s = [VR.AssignedValue(v % R) for v in state_in]
    before = len(ctx.advice)
    s = fix_len_array_squeeze(ctx, s, [VR.AssignedValue(v % R) for v in inputs], o, bool(flags & AO))
    assert len(ctx.advice) > before
    n = len(ctx.advice)
    ip = 1 + 3 * t
    offs = [n - (t - 1 - i) * ip - 1 for i in range(t)]
    assert [ctx.advice[f] for f in offs] == [x.value for x in s]
    return ctx.advice, [x.value for x in s], offs


def check_restatement():
    """0: the definition's final states equal the textbook sponge and the golden permutation KATs (CPU only)"""
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_reference_kats.json")))
    for t in (3, 5):
        sp, rate = PO.spec(t), t - 1
        vals = _ints(full_range_fr(3 * rate, 0x51 + t))
        for ln in (0, 1, rate - 1, rate, rate + 1, 2 * rate):
            cells, state, offs = unit_trace(t, vals[:ln], 0)
            assert state[1] == PO.H(sp, vals[:ln]), (t, ln)
            # the same from the permutation alone: the state after absorbing, without the empty chunk
            if ln and ln % rate == 0:
                _, st, _ = unit_trace(t, vals[:ln], AO)
                assert sp.absorb_and_permute(st, []) == state
        kat = kats["t%d" % t]
        _, state, _ = unit_trace(t, [int(v) for v in kat["inputs"]], AO, state_in=[int(v) for v in kat["state_in"]])
        assert state == [int(v) for v in kat["state_out"]], t
        cells3, _, _ = unit_trace(t, vals[:rate], 0)
        assert len(cells3) == 2 * len(unit_trace(t, [], 0)[0]) + 3 * rate


# ------------------------------------------------------------------------------------------------ placement
def place(col, row, ncells, bps, ncols):
    """the (column, row) of every cell of a run of ncells from (col, row), break copies included, as assign_witnesses lays a thread down:
    -> ([(cell index, column, row)], the position behind the run)"""
    out = []
    for i in range(ncells):
        out.append((i, col, row))
        if bps is not None and col < ncols - 1 and row == bps[col]:
            col, row = col + 1, 0
            out.append((i, col, row))
        row += 1
    return out, (col, row)


def _select(ctx, t):
    hs = PS.PoseidonHasher.new(ctx, t, *PO.SPECS[t])
    hs.select_optimized()
    return hs


def _inputs_pool(nvals, seed):
    vals = _ints(full_range_fr(nvals, seed, edges=False))
    vals[0:3] = [0, 1, R - 1]
    for j in range(3, nvals, 7):
        vals[j] = (0, 1, R - 1)[j % 3]
    return vals, fr(vals)


def _compare(ctx, d_cols, want, what):
    for c, p in enumerate(d_cols):
        got = ctx.download(p, want[c].shape)
        if not np.array_equal(got, want[c]):
            bad = np.nonzero((got != want[c]).any(axis=1))[0]
            raise AssertionError("%s: column %d: %d cells differ, first rows %s" % (what, c, len(bad), bad[:8].tolist()))


def check_fill(ctx, t, count, lens, with_states=(False, True)):
    """A: per len one call without and one with states_in_dev (and states_out_dev), `count` units over three columns whose flags cycle through
    0, ABSORB_ONLY, WITH_CONSTS and both, input strides through 1, 0 and 3; the inputs are the first rows of column 0 itself.  Every addressed
    cell equals the definition's, every other keeps its sentinel, states_out and trace_layout equal the definition's."""
    hs = _select(ctx, t)
    rate, ni = t - 1, 64
    in_int, in_raw = _inputs_pool(ni, 0xA0 + t)
    st_int, st_raw = _inputs_pool(count * t, 0xB0 + t)
    for ln in lens:
        for given in with_states:
            units, traces, rows = [], [], [ni + 3, 2, 0]
            for j in range(count):
                flags = ((0, AO, WC, AO | WC) if ln else (0, WC))[j % (4 if ln else 2)]
                stride = (1, 0, 3)[j % 3]
                off = (5 * j) % (ni - 3 * max(ln - 1, 0))
                ins = [in_int[off + i * stride] for i in range(ln)]
                cells, state, offs = unit_trace(t, ins, flags, st_int[j * t:(j + 1) * t] if given else None)
                ncells, loffs = hs.trace_layout(ln, flags)
                assert (ncells, loffs) == (len(cells), offs), (t, ln, flags, ncells, len(cells), loffs, offs)
                col = j % 3
                units.append((col, rows[col], off, stride, flags))
                traces.append((cells, state))
                rows[col] += len(cells) + (j % 2)
            n = max(rows) + 9
            want = [np.tile(SENTINEL, (n, 1)) for _ in range(3)]
            want[0][:ni] = in_raw
            for (col, row, _o, _s, _f), (cells, _st) in zip(units, traces):
                want[col][row:row + len(cells)] = fr(cells)
            d_cols = [ctx.to_device(c) for c in want]
            for (col, row, _o, _s, _f), (cells, _st) in zip(units, traces):
                want[col][row:row + len(cells)] = SENTINEL
            for c in range(3):
                ctx.upload(d_cols[c], want[c])
            for (col, row, _o, _s, _f), (cells, _st) in zip(units, traces):
                want[col][row:row + len(cells)] = fr(cells)
            d_in = ctx.to_device(st_raw) if given else 0
            d_out = ctx.to_device(np.tile(SENTINEL, (count * t, 1)))
            try:
                hs.fill_hashes(ctx, d_cols, n - 2, None, d_cols[0], ni, ln, units, d_in, d_out)
                ctx.sync()
                _compare(ctx, d_cols, want, "t = %d, len = %d, states_in %s" % (t, ln, given))
                assert _ints(ctx.download(d_out, (count * t, 4))) == [v for (_c, st) in traces for v in st], (t, ln, given)
            finally:
                for p in d_cols + [d_out] + ([d_in] if given else []):
                    ctx.free(p)


# ------------------------------------------------------------------------------------------------ B: independent answers
def check_independent(ctx):
    """the golden t3 / t5 permutation KATs through states_in_dev + ABSORB_ONLY with len = RATE; the digest cells of random messages equal
    h2hip_poseidon_hash_batch_dev's digests and the textbook sponge H's"""
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_reference_kats.json")))
    for t in (3, 5):
        hs = _select(ctx, t)
        rate, kat = t - 1, kats["t%d" % t]
        ncells, offs = hs.trace_layout(rate, AO)
        d_col = ctx.to_device(np.tile(SENTINEL, (ncells + 16, 1)))
        d_in, d_st = ctx.to_device(fr([int(v) for v in kat["inputs"]])), ctx.to_device(fr([int(v) for v in kat["state_in"]]))
        d_out = ctx.malloc(32 * t)
        try:
            hs.fill_hashes(ctx, [d_col], ncells + 9, None, d_in, rate, rate, [(0, 4, 0, 1, AO)], d_st, d_out)
            want = [int(v) for v in kat["state_out"]]
            assert _ints(ctx.download(d_out, (t, 4))) == want, t
            col = ctx.download(d_col, (ncells + 16, 4))
            assert _ints(col[[4 + f for f in offs]]) == want, t
        finally:
            for p in (d_col, d_in, d_st, d_out):
                ctx.free(p)
        # digests: 6 messages per length
        sp = PO.spec(t)
        for ln in (1, rate, 2 * rate + 1):
            nmsg = 6
            raw = full_range_fr(nmsg * ln, 0xD1 + ln)
            msgs = np.ascontiguousarray(raw).reshape(nmsg, ln, 4)
            ncells, offs = hs.trace_layout(ln, 0)
            d_cols = [ctx.to_device(np.tile(SENTINEL, (3 * ncells + 16, 1))) for _ in range(2)]
            d_in = ctx.to_device(raw)
            try:
                units = [(j % 2, (j // 2) * ncells + 1, j * ln, 1, 0) for j in range(nmsg)]
                hs.fill_hashes(ctx, d_cols, 3 * ncells + 9, None, d_in, nmsg * ln, ln, units)
                cols = [ctx.download(p, (3 * ncells + 16, 4)) for p in d_cols]
            finally:
                for p in d_cols + [d_in]:
                    ctx.free(p)
            digests = np.stack([cols[c][row + offs[1]] for (c, row, _o, _s, _f) in units])
            assert np.array_equal(digests, hs.hash_fix_len_array(msgs)), (t, ln)
            ints = _ints(raw)
            assert _ints(digests) == [PO.H(sp, ints[j * ln:(j + 1) * ln]) for j in range(nmsg)], (t, ln)


# ------------------------------------------------------------------------------------------------ C: the optimised spec
def check_spec_optimize(ctx):
    """h2hip_poseidon_spec_optimize equals the Python derivation element for element, for both t; a hand-made spec whose MDS row starts with 1
    is refused with that reason by both entries"""
    for t in (3, 5):
        hs = PS.PoseidonHasher.new(ctx, t, *PO.SPECS[t])
        got, want = hs.optimized_spec(), opt_spec(t).arrays()
        for name, g, w in zip(PS.OptimizedSpec._fields, got, want):
            assert g.shape == w.shape and np.array_equal(g, w), (t, name)
    t, (r_f, r_p) = 3, PO.SPECS[3]
    o = opt_spec(t)
    good = o.arrays()
    bad_mds = [list(r) for r in o.mds]
    bad_mds[1][0] = 1
    for what, spec in (("mds", good._replace(mds=fr([v for r in bad_mds for v in r]).reshape(t, t, 4))),
                       ("pre_sparse_mds", good._replace(pre_sparse_mds=fr([v for r in bad_mds for v in r]).reshape(t, t, 4))),
                       ("sparse", good._replace(sparse=np.concatenate([good.sparse[:5], fr([1] + [7] * (2 * t - 2)).reshape(1, 2 * t - 1, 4), good.sparse[6:]])))):
        try:
            PS.set_optimized_spec(ctx, t, r_f, r_p, spec)
        except H.H2HipError as e:
            assert e.code == ERR_INVALID and "begins with 1" in str(e), (what, str(e))
        else:
            raise AssertionError("a spec whose %s row begins with 1 was accepted" % what)
    sp = PO.spec(t)
    try:
        PS.spec_optimize(t, r_f, r_p, fr([c for row in sp.constants for c in row]), fr([v for r in bad_mds for v in r]), ctx.lib)
    except H.H2HipError as e:
        assert e.code == ERR_INVALID and "begins with 1" in str(e), str(e)
    else:
        raise AssertionError("h2hip_poseidon_spec_optimize accepted an MDS row that begins with 1")
    PS.set_optimized_spec(ctx, t, r_f, r_p, good)


# ------------------------------------------------------------------------------------------------ D: column breaks
def check_breaks(ctx, case):
    """the same virtual run (a filler of plain cells, then the units back to back) laid into columns of 1,500 usable rows by
    virtual_region.assign_witnesses and by the fill from each unit's first cell.  t = 3, len = 2: a unit of 4,506 cells crosses at least two
    breaks.  `first`: a break on the unit's first cell.  `middle_last_behind`: a break on the first cell of an S-box gate in the middle of the
    first permutation, a break on the unit's last cell, and a second unit that starts right behind that break (row 1 of the next column)."""
    t, ln, u = 3, 2, 1500
    hs = _select(ctx, t)
    n0, _ = hs.trace_layout(ln, 0)
    n1, _ = hs.trace_layout(ln, AO)
    assert (n0, n1) == (4506, 2256)
    if case == "first":
        filler, flags, bps = 7, [0], [7, 1400, 1300, 1450]
    else:
        gate = 4 + 7 * ln + 12 * 5                       # the first cell of the sixth mul gate of the first full round's S-boxes
        rest = n0 - (gate + 1) - 1490 - 1480              # what is left for the fourth column: the last of them sits on its break point
        filler, flags, bps = 0, [0, AO], [gate, 1490, 1480, rest, 1490]
        assert 0 < rest < u
    ncols = len(bps) + 1
    in_int, in_raw = _inputs_pool(8, 0xE1)
    thread = VR.Context(True, "gate", 0, VR.CopyConstraintManager())
    thread.advice += list(range(100, 100 + filler))
    pos, units = place(0, 0, filler, bps, ncols)[1], []
    for j, f in enumerate(flags):
        cells, _st, _ = unit_trace(t, in_int[2 * j:2 * j + 2], f)
        thread.advice += cells
        units.append((pos[0], pos[1], 2 * j, 1, f))
        cells_at, pos = place(pos[0], pos[1], len(cells), bps, ncols)
    if case != "first":
        assert units[1][:2] == (4, 1) and cells_at[-1][1:] == (5, 766)
    region = VR.Region(u + 9, ncols)
    VR.assign_witnesses([thread], list(range(ncols)), region, bps)
    want = [np.tile(SENTINEL, (u + 9, 1)) for _ in range(ncols)]
    for c in range(ncols):
        rows = sorted(region.advice[c])
        want[c][rows] = fr([region.advice[c][r] for r in rows])
    start = [np.tile(SENTINEL, (u + 9, 1)) for _ in range(ncols)]
    if filler:
        start[0][:filler] = want[0][:filler]
    d_cols = [ctx.to_device(c) for c in start]
    d_in = ctx.to_device(in_raw)
    try:
        hs.fill_hashes(ctx, d_cols, u, bps, d_in, 8, ln, units)
        ctx.sync()
        _compare(ctx, d_cols, want, "breaks (%s)" % case)
    finally:
        for p in d_cols + [d_in]:
            ctx.free(p)


# ------------------------------------------------------------------------------------------------ E: the refusals
def check_rejections(ctx, fresh_ctx):
    """one case per refusal of include/h2hip.h's list: H2HIP_ERR_INVALID, the reason in h2hip_last_error, the sentinel everywhere; then a
    good call from the same context"""
    t, ln = 3, 2
    n, u, ni = 4700, 4600, 16
    in_int, in_raw = _inputs_pool(ni, 0xF1)
    sent = np.tile(SENTINEL, (n, 1))
    d_cols = [fresh_ctx.to_device(sent) for _ in range(3)]
    d_in = fresh_ctx.to_device(in_raw)
    ok = (0, 0, 0, 1, AO)                                 # 2,256 cells: rows 0..2255 of column 0
    try:
        PS.fill_hashes(fresh_ctx, d_cols, u, None, d_in, ni, ln, [ok])
    except H.H2HipError as e:
        assert e.code == ERR_INVALID and "no optimised spec" in str(e), str(e)
    else:
        raise AssertionError("a fill without an optimised spec was accepted")
    for p in d_cols + [d_in]:
        fresh_ctx.free(p)
    hs = _select(ctx, t)
    d_cols = [ctx.to_device(sent) for _ in range(3)]
    d_in = ctx.to_device(in_raw)
    d_st = ctx.to_device(fr(list(range(1, 3 * t + 1))))
    cells = 2256
    try:
        def refused(what, reason, call):
            try:
                call()
            except H.H2HipError as e:
                assert e.code == ERR_INVALID, (what, e.code)
                msg = ctx.lib.h2hip_last_error().decode()
                assert reason in msg, (what, msg)
            else:
                raise AssertionError("%s was accepted" % what)
            ctx.sync()
            for p in d_cols:
                assert np.array_equal(ctx.download(p, (n, 4)), sent), "%s: a cell was written" % what

        fill = lambda units, cols=None, usable=u, bps=None, inp=None, ilen=ni, length=ln, st_in=0, st_out=0: (
            lambda: PS.fill_hashes(ctx, cols or d_cols, usable, bps, d_in if inp is None else inp, ilen, length, units, st_in, st_out))
        refused("unknown flags", "unknown flags", fill([ok, (1, 0, 0, 1, 4)]))
        refused("len == 0 with ABSORB_ONLY", "without a permutation", fill([(1, 0, 0, 1, AO)], length=0))
        refused("column index out of range", "column index", fill([ok, (3, 0, 0, 1, AO)]))
        refused("a NULL column", "column index", fill([ok, (1, 0, 0, 1, AO)], cols=[d_cols[0], 0, d_cols[2]]))
        refused("a run that leaves the usable rows", "usable rows", fill([ok, (1, u - cells + 1, 0, 1, AO)]))
        refused("a run that leaves the last column", "last column", fill([ok, (2, u - cells + 1, 0, 1, AO)], bps=[u - 1, u - 1]))
        refused("a run that breaks into a NULL column", "column index", fill([(0, 100, 0, 1, AO)], cols=[d_cols[0], 0, d_cols[2]], bps=[200, 5]))
        refused("a break point >= usable_rows", "break point", fill([ok], bps=[10, u]))
        refused("inputs past inputs_len", "inputs lie outside", fill([ok, (1, 0, ni - 1, 1, AO)]))
        refused("inputs past inputs_len by the stride", "inputs lie outside", fill([ok, (1, 0, 0, ni, AO)]))
        refused("an offset that wraps in 64 bits", "inputs lie outside", fill([ok, (1, 0, (1 << 64) - 1, 1, AO)]))
        refused("two units overlap", "overlap", fill([ok, (0, cells - 1, 0, 1, AO)]))
        refused("a break copy inside another unit", "overlap", fill([(1, 0, 0, 1, AO), (0, 20, 0, 1, AO)], bps=[30, u - 1], usable=u))
        refused("inputs inside cells this call writes", "operand range", fill([(1, 0, 5, 1, AO)], inp=d_cols[1], ilen=u))
        refused("states_in inside cells this call writes", "operand range", fill([(1, 0, 0, 1, AO)], st_in=d_cols[1] + 32 * 40))
        refused("states_out inside cells this call writes", "overlap", fill([(1, 0, 0, 1, AO)], st_out=d_cols[1] + 32 * 40))
        refused("inputs_dev NULL", "NULL argument", lambda: PS.fill_hashes(ctx, d_cols, u, None, 0, ni, ln, [ok]))
        cols = (_vp * 3)(*[_vp(int(p)) for p in d_cols])
        refused("hashes NULL", "NULL argument",
                lambda: ctx._chk(ctx.lib.h2hip_poseidon_fill_hashes_dev(ctx.handle, cols, 3, u, None, _vp(int(d_in)), ni, ln, None, None, None, 1)))
        refused("columns NULL", "NULL argument",
                lambda: ctx._chk(ctx.lib.h2hip_poseidon_fill_hashes_dev(ctx.handle, None, 3, u, None, _vp(int(d_in)), ni, ln, None, None,
                                                                        C.cast(PS.hash_table([ok]), _vp), 1)))
        for what, args in (("trace_layout: unknown flags", (ln, 8)), ("trace_layout: no permutation", (0, AO))):
            try:
                hs.trace_layout(*args)
            except H.H2HipError as e:
                assert e.code == ERR_INVALID, what
            else:
                raise AssertionError(what + " was accepted")
        # count == 0 needs nothing
        PS.fill_hashes(ctx, d_cols, u, None, 0, 0, ln, [])
        # the largest unit that still fits (its last cell on row u - 1), inputs that end with inputs_len, a unit that ends on its break point
        units = [(0, u - cells, ni - 2, 1, AO), (1, 30, 0, ni - 1, AO)]
        bps = [u - 1, 30 + 100]
        hs.fill_hashes(ctx, d_cols, u, bps, d_in, ni, ln, units, d_st, 0)
        ctx.sync()
        want = [np.tile(SENTINEL, (n, 1)) for _ in range(3)]
        for j, (col, row, off, stride, f) in enumerate(units):
            tr, _st, _ = unit_trace(t, [in_int[off], in_int[off + stride]], f, list(range(1 + j * t, 1 + (j + 1) * t)))
            for i, c, r in place(col, row, len(tr), bps, 3)[0]:
                want[c][r] = fr([tr[i]])[0]
        _compare(ctx, d_cols, want, "after the refusals")
    finally:
        for p in d_cols + [d_in, d_st]:
            ctx.free(p)


# ------------------------------------------------------------------------------------------------ F: inside a proof
def _merkle_program(builder, leaves, o):
    """the Merkle root of four leaves: three 2-to-1 hashes (hash_fix_len_array from a PoseidonState::default of its own each), the root as the
    instance.  -> the thread offsets of every unit's first cell and of the three digests"""
    ctx = builder.main()
    cells = [ctx.load_witness(v) for v in leaves]
    starts, digests = [], []

    def hash2(a, b):
        starts.append(len(ctx.advice))
        s = fix_len_array_squeeze(ctx, _default_state(ctx, o.t), [a, b], o)
        digests.append(len(ctx.advice) - (o.t - 2) * (1 + 3 * o.t) - 1)
        assert ctx.advice[digests[-1]] == s[1].value
        return s[1]

    left, right = hash2(cells[0], cells[1]), hash2(cells[2], cells[3])
    root = hash2(left, right)
    builder.assigned_instances = [[root]]
    return starts, digests


def check_proof(ctx, k, seed):
    """F: a BaseConfig circuit built through the Context mirror; keygen from the mirror's selectors and copies; the advice is device columns
    whose hash cells two fill_hashes calls write, the second reading the first level's digest cells from their columns.  The proof has the
    bytes of the proof from the Python-computed advice, both verifiers accept it, check_witness finds nothing, and names the gate row once a
    trace cell is changed on the device."""
    t, lb = 3, 8
    o = opt_spec(t)
    hs = _select(ctx, t)
    leaves = _ints(full_range_fr(4, seed, edges=False))
    n = 1 << k
    max_rows = n - 9
    total = 4 + 3 * (t + hs.trace_layout(2, 0)[0])
    na = -(-total // (max_rows - 4)) + 1
    while True:                                        # the number of gate columns the layout fills (an empty one would have a disjoint selector)
        sh = P.Shape(k, na, 1, 1, 1, lb)
        kb = VR.BaseCircuitBuilder(False)
        starts, digests = _merkle_program(kb, leaves, o)
        advice_k, fixed, copies, instances, bps = kb.synthesize(sh)
        if len(bps) == na - 1:
            break
        na = len(bps) + 1
    assert na >= 2 and len(bps) >= 1
    pb = VR.BaseCircuitBuilder(True)
    pb.break_points = bps
    assert _merkle_program(pb, leaves, o) == (starts, digests)
    advice, _, _, _, _ = pb.synthesize(sh)
    assert all(np.array_equal(a, b) for a, b in zip(advice, advice_k))
    root = PO.merkle_tree(PO.spec(t), leaves)[1]
    assert _ints(instances[0]) == [root], "the circuit's instance is not the Merkle root"
    gate_cols = list(sh.gate_advice)
    assert gate_cols == list(range(na)) and len(advice) == na + 1
    # where every thread cell lies: the flat index c * n + r over one allocation of all gate columns
    cells_at, _ = place(0, 0, total, bps, na)
    first = {}
    for i, c, r in cells_at:
        first.setdefault(i, (c, r))
    flat = lambda i: first[i][0] * n + first[i][1]
    assert any(first[s][0] != first[s + t + 4505][0] for s in starts), "no break falls inside a trace"
    kzg, srs_params = srs(ctx, k, seed)
    gpk = PL.keygen(kzg, PL.BaseCircuitParams.new(k, na, 1, 1, 1, lb), fixed, copies)
    budget = rng_budget(sh)
    host = np.zeros((na * n, 4), dtype=np.uint64)
    host[0:4] = advice[0][0:4]                         # the leaves; every other gate cell is a trace cell
    d_gate = ctx.to_device(host)
    d_lookup = ctx.to_device(np.ascontiguousarray(advice[na]))
    d_cols = [d_gate + 32 * n * c for c in range(na)]
    try:
        want = PL.create_proof(gpk, advice, instances, PreDrawnRng(budget, 1000 + seed))
        level1 = PS.hash_table([first[starts[0]] + (0, 1, WC), first[starts[1]] + (2, 1, WC)])
        level2 = PS.hash_table([first[starts[2]] + (flat(digests[0]), flat(digests[1]) - flat(digests[0]), WC)])
        hs.fill_hashes(ctx, d_cols, sh.usable_rows, bps, d_gate, na * n, 2, level1)
        hs.fill_hashes(ctx, d_cols, sh.usable_rows, bps, d_gate, na * n, 2, level2)
        ctx.sync()
        got_cols = ctx.download(d_gate, (na, n, 4))
        for c in range(na):
            assert np.array_equal(got_cols[c], advice[c]), "gate column %d differs from the Python-computed advice" % c
        got = PL.create_proof(gpk, d_cols + [d_lookup], instances, PreDrawnRng(budget, 1000 + seed), advice_on_device=True)
        assert got == want, "the proof over device-filled hash cells differs from the one over the Python-computed advice"
        assert PL.verify_proof(gpk, instances, got), "h2hip_plonk_verify_proof rejects the proof"
        assert P.verify_proof(srs_params, vk_from_gpu(sh, gpk), [_ints(v) for v in instances], got), "the test verifier rejects the proof"
        total_f, fails = PL.check_witness(gpk, d_cols + [d_lookup], instances, advice_on_device=True)
        assert total_f == 0, fails
        # one trace cell changed on the device: the x^2 cell of the first S-box of the root's hash (the last cell of its gate)
        i = starts[2] + t + 4 + 7 * 2 + 3
        c, r = first[i]
        assert r >= 3 and first[i - 3] == (c, r - 3)
        ctx.upload(d_cols[c] + 32 * r, fr([(_ints(advice[c][r:r + 1])[0] + 1) % R]))
        total_f, fails = PL.check_witness(gpk, d_cols + [d_lookup], instances, advice_on_device=True)
        assert total_f >= 1 and any(f.kind == "gate" and f.column == c and f.row == r - 3 for f in fails), fails
    finally:
        ctx.free(d_gate)
        ctx.free(d_lookup)
        gpk.free()
        kzg.free()


# ------------------------------------------------------------------------------------------------ the struct in every layer
def check_struct_layout():
    """h2hip_poseidon_hash: the same fields in the header, the Rust sys crate and ctypes; the flag values alike"""
    hdr = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    rs = open(os.path.join(ROOT, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    body = re.search(r"typedef struct h2hip_poseidon_hash\s*\{(.*?)\}\s*h2hip_poseidon_hash\s*;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    cmap = {"uint32_t": "u32", "uint64_t": "u64"}
    c_fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            c_fields += [(nm.strip(), cmap[ty]) for nm in names.split(",")]
    rs_body = re.search(r"pub struct h2hip_poseidon_hash\s*\{(.*?)\}", rs, flags=re.S).group(1)
    rs_fields = re.findall(r"pub ([a-z_]+): ([a-z0-9]+)", rs_body)
    py_fields = [(nm, {C.c_uint32: "u32", C.c_uint64: "u64"}[ty]) for nm, ty in PS.PoseidonHashStruct._fields_]
    assert c_fields == rs_fields == py_fields, (c_fields, rs_fields, py_fields)
    assert C.sizeof(PS.PoseidonHashStruct) == 24
    for name, v in (("ABSORB_ONLY", 1), ("WITH_CONSTS", 2)):
        assert re.search(r"#define H2HIP_POSEIDON_%s %d\b" % (name, v), hdr) and "pub const H2HIP_POSEIDON_%s: u32 = %d;" % (name, v) in rs
        assert getattr(PS, name) == v
    for layer in ("halo2-lib_amd/host/halo2_proofs.hpp", "ffi/rust/h2hip-sys/src/safe.rs"):
        src = open(os.path.join(ROOT, layer)).read()
        for fn in ("h2hip_poseidon_fill_hashes_dev", "h2hip_poseidon_spec_optimize", "h2hip_poseidon_set_optimized_spec", "h2hip_poseidon_trace_layout"):
            assert fn in src, (layer, fn)
