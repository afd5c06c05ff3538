"""h2hip_plonk_check_witness at the edges of its kernels (halo2-lib_amd/csrc/witness_check.hip), shared by tests/test_witness_check.py (the
CPU-emulated build) and tests/test_witness_check_gpu.py: every check takes a ctx.  The reference everywhere is tests/witness_check_oracle.py
(plain Python integers and set membership); (total, failure tuples) are compared for equality, order included.

  1. range-lookup membership over the whole field: out-of-table inputs whose low limbs are a table entry's (check_range_membership);
  2. the failure list across mask blocks (8192 units each): dense and sparse patterns, max_failures at every block boundary, and the
     caller's buffer behind the records written (check_mask_blocks);
  3. dynamic lookups: inputs whose search key equals a table row's while the tuple differs, runs of table rows with one key
     (check_dyn_neighbours, check_dyn_runs);
  4. copy failures with permutation columns >= 256, a hand-built key whose gates reach the blinding rows, device advice with garbage
     behind the usable rows, RLC gates on the last row they may be enabled on (check_wide_copy_peers, check_hand_built_key,
     check_device_advice_garbage, check_rlc_gate_edge).

Keys are made by keygen from arrays written here: keygen and the checker take any fixed columns and copies, so most of these witnesses are
not honest ones and only the Python checker's verdict counts."""
import ctypes as C
import os
import re

import numpy as np

from halo2_lib_amd import halo2_proofs as HP
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import testing as T
from oracle import bn254 as O
from oracle import plonk as P
from tests import witness_check_oracle as W
from tests.dyn_lookup_util import oracle_shape, ram_circuit
from tests.util import R, edge_fr_values, fr, full_range_fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
BLOCK_UNITS = 8192   # WC_BLOCK_WORDS * 32 mask units per count / write workgroup
TOXIC_S = 0x1D0C0FFEE1234567890ABCDEF
_KINDS = {"gate": W.GATE, "lookup": W.LOOKUP, "copy": W.COPY}


class _Backend:
    def __init__(self, ctx):
        self.mul, self.add = ctx.fr_mul, ctx.fr_add


def _ints(col):
    return O.limbs_to_ints(np.ascontiguousarray(col), R)


def _col(vals):
    return np.array(fr([v % R for v in vals]))


def _put(col, cells):
    """a copy of the column with {row: value} written"""
    col = np.array(col)
    rows = sorted(cells)
    if rows:
        col[rows] = fr([cells[r] % R for r in rows])
    return col


def lib_check(pk, advice, instances=(), max_failures=1 << 12, **kw):
    total, fails = PL.check_witness(pk, advice, instances, max_failures, **kw)
    return total, [(_KINDS[f.kind], f.column, f.row, f.peer_column, f.peer_row) for f in fails]


def raw_check(ctx, pk, advice, instances, max_failures, pad=64):
    """the C entry over a failures_out of max_failures + pad records filled with 0xA5 bytes -> (total, the whole buffer as (records, 5) u32)"""
    keep = [np.ascontiguousarray(c, dtype=np.uint64) for c in advice]
    adv = (_vp * len(keep))(*[_vp(c.ctypes.data) for c in keep])
    inst = [np.ascontiguousarray(c, dtype=np.uint64) for c in instances]
    ip = (_vp * max(len(inst), 1))(*[_vp(c.ctypes.data) for c in inst])
    il = (C.c_size_t * max(len(inst), 1))(*[len(c) for c in inst])
    buf = np.full((max_failures + pad, 5), 0xA5A5A5A5, dtype=np.uint32)
    total = C.c_size_t(0)
    rc = ctx.lib.h2hip_plonk_check_witness(ctx.handle, pk.handle, adv, 0, ip, il, _vp(buf.ctypes.data), max_failures, C.byref(total))
    assert rc == 0, ctx.lib.h2hip_last_error()
    return total.value, buf


class BaseKey:
    """a BaseConfig key on ctx from testing.build_circuit's circuit; edit(sh, fixed) may rewrite the fixed columns, more_copies are appended"""

    def __init__(self, ctx, shape, seed=3, edit=None, more_copies=()):
        self.ctx, self.sh = ctx, P.Shape(*shape)
        self.circ = T.build_circuit(self.sh, seed, _Backend(ctx))
        self.fixed = [np.array(c) for c in self.circ.fixed]
        if edit is not None:
            edit(self.sh, self.fixed)
        self.copies = list(self.circ.copies) + list(more_copies)
        self.advice, self.instances = [np.array(c) for c in self.circ.advice], [np.array(c) for c in self.circ.instances]
        self.kzg = HP.ParamsKZG.setup(ctx, shape[0], TOXIC_S + seed)
        try:
            self.pk = PL.keygen(self.kzg, PL.BaseCircuitParams.new(*shape), self.fixed, self.copies)
        except Exception:
            self.kzg.free()
            raise

    def oracle(self, advice, instances=None):
        return W.check(self.sh, self.fixed, advice, self.instances if instances is None else instances, self.copies)

    def free(self):
        self.pk.free()
        self.kzg.free()


# ------------------------------------------------------------------------------------------------ 1. range lookups over the whole field
def range_values(lb):
    """(members, non-members by name) of the table 0 .. 2^lb - 1, canonical values: non-members whose limbs 0 or 0..1 are a table entry's
    (one bit set in limb j, j = 1..7), the top of the field, values at and above 2^252, and tests.util's edge patterns"""
    members = [0, 1, (1 << lb) - 1]
    non = [("above", 1 << lb), ("above", (1 << lb) + 1)]
    non += [("limb%d" % j, t + (1 << (32 * j))) for j in range(1, 8) for t in (0, 5, (1 << lb) - 1)]
    non += [("top", R - 1), ("top", R - (1 << lb)), ("top", (R + 1) // 2), ("wide", (1 << 252) + 1), ("wide", (1 << 253) + 3)]
    non += [("edge", v) for v in edge_fr_values() if v >= 1 << lb]
    assert all(0 <= v < R and v >= 1 << lb for _, v in non) and (1 << 224) + (1 << lb) < R
    return members, non


def _plant_rows(u, count, shift):
    """`count` distinct usable rows that begin with 0, 31, 32 and u - 1 (a mask word's first and last bit, the next word, the last usable row)"""
    rows = [0, 31, 32, u - 1]
    r = 1 + shift
    while len(rows) < count:
        if r not in rows:
            rows.append(r)
        r = (r + 7) % u
    assert len(set(rows)) == count and max(rows) < u
    return rows


def check_range_membership(ctx, k, lb, single):
    """shape (k, 2, 2, 1, 0, lb) (lookup-advice columns) or, single, (k, 1, 1, 1, 0, lb) (q_lookup * a on advice 0, q_lookup written here)"""
    members, non = range_values(lb)
    vals = [("member", v) for v in members] + non
    n, u = 1 << k, (1 << k) - 7
    assert len(vals) + 8 <= u
    off_rows = []

    def edit(sh, fixed):   # single: q_lookup = 1 exactly on the planted rows
        q = np.zeros((n, 4), dtype=np.uint64)
        q[_plant_rows(u, len(vals), 0)] = fr([1])[0]
        fixed[sh.q_lookup_col] = q

    b = BaseKey(ctx, (k, 1, 1, 1, 0, lb) if single else (k, 2, 2, 1, 0, lb), seed=5, edit=edit if single else None)
    try:
        sh = b.sh
        assert sh.usable_rows == u
        adv = list(b.advice)
        planted = {}   # (lookup index, row) -> (name, value)
        if single:
            assert len(sh.lookups) == 1 and sh.lookups[0][0] == sh.q_lookup_col
            rows = _plant_rows(u, len(vals), 0)
            cells = {r: v for r, (_, v) in zip(rows, vals)}
            planted = {(0, r): nv for r, nv in zip(rows, vals)}
            off_rows = [r for r in range(u) if r not in cells][5:9]   # q_lookup = 0 there: the input is 0, a member
            for r, v in zip(off_rows, [R - 1, 1 << 64, R - 1, 1 << 64]):
                cells[r] = v
            adv[0] = _put(adv[0], cells)
        else:
            assert [q for q, _, _ in sh.lookups] == [None, None]
            for li, la in enumerate(sh.lookup_advice):
                rows = _plant_rows(u, len(vals), 5 * li)
                order = vals[7 * li:] + vals[:7 * li]   # another value on rows 0, 31, 32, u - 1 of the second column
                adv[la] = _put(adv[la], {r: v for r, (_, v) in zip(rows, order)})
                planted.update({(li, r): nv for r, nv in zip(rows, order)})
        want = b.oracle(adv)
        failed = {(f[1], f[2]) for f in want[1] if f[0] == W.LOOKUP}
        # the input mix, on the checker alone: every non-member fails, every member passes, every limb j = 1..7 is represented
        for cell, (name, v) in planted.items():
            assert (cell in failed) == (name != "member"), (cell, name, hex(v))
        for j in range(1, 8):
            assert any(planted[c][0] == "limb%d" % j for c in failed if c in planted), j
        for li in range(len(sh.lookups)):
            assert {r for (l, r) in planted if l == li} >= {0, 31, 32, u - 1}
        assert all((0, r) not in failed for r in off_rows) and (not single or len(off_rows) == 4)
        got = lib_check(b.pk, adv, [], want[0] + 8)
        assert got == want, _first_difference(got, want)
    finally:
        b.free()


def _first_difference(got, want):
    if got[0] != want[0]:
        return "total %d, the checker says %d" % (got[0], want[0])
    for i, (g, w) in enumerate(zip(got[1], want[1])):
        if g != w:
            return "failure %d is %s, the checker says %s" % (i, g, w)
    return "%d failures listed, the checker lists %d" % (len(got[1]), len(want[1]))


# ------------------------------------------------------------------------------------------------ 2. the failure list across mask blocks
def mask_unit(sh, f):
    """the mask unit of a failure tuple: [gate columns][lookups][permutation columns] x stride, stride = usable rows rounded up to 32"""
    stride = (sh.usable_rows + 31) & ~31
    kind, col, row = f[0], f[1], f[2]
    G, L = len(sh.gates), len(sh.lookups)
    if kind == W.GATE:
        col = [a for _, a in sh.gates].index(col)
    elif kind == W.LOOKUP:
        col = G + col
    else:
        col = G + L + col
    return col * stride + row


def num_blocks(sh):
    stride = (sh.usable_rows + 31) & ~31
    units = (len(sh.gates) + len(sh.lookups) + len(sh.perm_columns)) * stride
    return (units + BLOCK_UNITS - 1) // BLOCK_UNITS


class MaskBlockCase:
    """A BaseConfig key whose all-zero witness is satisfied (the constants are zero; one copy joins instance row 5 to row 7 of the last
    advice column; a one-gate-column shape has q_lookup = 1 on every row), and the five failure patterns written over that witness."""
    INSTANCE_LEN = 6

    def __init__(self, ctx, shape):
        def edit(sh, fixed):
            for c in sh.constant_cols:
                fixed[c] = np.zeros_like(fixed[c])
            if sh.q_lookup_col is not None:
                fixed[sh.q_lookup_col] = np.tile(fr([1])[0], (sh.n, 1))

        sh = P.Shape(*shape)
        self.last_adv = sh.num_advice_total - 1
        self.b = BaseKey(ctx, shape, seed=3, edit=edit, more_copies=[((("instance", 0), 5), (("advice", self.last_adv), 7))])
        self.sh, self.u, self.n, self.lb = self.b.sh, self.b.sh.usable_rows, self.b.sh.n, shape[5]
        self.inputs = [a for _, a, _ in self.sh.lookups]   # the advice column of every lookup input
        self.zero = [np.zeros((self.n, 4), dtype=np.uint64) for _ in range(self.sh.num_advice_total)]
        self.inst0 = [np.zeros((self.INSTANCE_LEN, 4), dtype=np.uint64)]
        self.blocks = num_blocks(self.sh)
        assert self.b.oracle(self.zero, self.inst0) == (0, [])

    def free(self):
        self.b.free()

    def pattern(self, name):
        """-> (advice, instances)"""
        u, n, out = self.u, self.n, (1 << self.lb) + 3
        adv, inst = list(self.zero), list(self.inst0)
        if name == "a":     # every usable row of every lookup input column (and the rows behind them, which must not count)
            for a in self.inputs:
                adv[a] = _col([out] * n)
        elif name == "b":   # the first and the last bit of every mask word
            for a in self.inputs:
                adv[a] = _put(adv[a], {r: out for r in range(u) if r % 32 in (0, 31)})
        elif name == "c":
            for a in self.inputs:
                adv[a] = _put(adv[a], {0: out, u - 1: out})
        elif name == "d":   # gate column 0 and the far end of the permutation columns only
            copied = {r for l, rr in self.b.copies for (c, r) in (l, rr) if c == ("advice", 0)}
            m = u // 4
            ts = [t for t in list(range(3, 12)) + [m - 2] if 4 * t + 3 not in copied][:4]
            adv[0] = _put(adv[0], {4 * t + 3: 1 for t in ts})   # the d cell of gate t, read by that gate alone; 1 is a table member
            inst[0] = _put(inst[0], {5: 9})
        elif name == "e":   # every advice column an arithmetic pattern: gates, lookups (values 200 .. 296) and copies fail densely
            for c in range(len(adv)):
                adv[c] = _col([(3 * r + c) % 97 + 200 for r in range(n)])
        else:
            raise KeyError(name)
        return adv, inst

    def cuts(self, want):
        """c_b for every block b: the expected failures whose mask unit lies below 8192 (b + 1)"""
        units = [mask_unit(self.sh, f) for f in want[1]]
        assert units == sorted(units) and len(set(units)) == len(units)   # canonical order is mask order
        return [sum(1 for x in units if x < BLOCK_UNITS * (b + 1)) for b in range(self.blocks)]


def check_mask_blocks(ctx, case, name):
    adv, inst = case.pattern(name)
    want = case.b.oracle(adv, inst)
    total, u, sh = want[0], case.u, case.sh
    cuts = case.cuts(want)
    inner = sorted({c for c in cuts if 0 < c < total})
    assert total > 0 and all(f[2] < u for f in want[1])
    if name in ("a", "e"):
        assert len(inner) >= 2, cuts
    if name == "a":     # full words, and 25 bits in a column's last word (u = 2^k - 7)
        assert u % 32 == 25 and sum(1 for f in want[1] if f[0] == W.LOOKUP) == u * len(sh.lookups)
    if name == "d":     # an empty block between two non-empty ones
        per_block = [c - p for c, p in zip(cuts, [0] + cuts[:-1])]
        filled = [i for i, c in enumerate(per_block) if c]
        assert filled[0] == 0 and any(c == 0 for c in per_block[: filled[-1]]), per_block
        assert {f[0] for f in want[1]} == {W.GATE, W.COPY} and want[1][-1][1] == len(sh.perm_columns) - 1
    if name == "e":
        assert {f[0] for f in want[1]} == {W.GATE, W.LOOKUP, W.COPY}
    maxes = {0, 1, 2, 31, 32, 33, total - 1, total, total + 5}
    for c in cuts:
        maxes |= {c - 1, c, c + 1}
    for mx in sorted(m for m in maxes if m >= 0):
        got = lib_check(case.b.pk, adv, inst, mx)
        assert got == (total, want[1][: min(mx, total)]), (name, mx, _first_difference(got, (total, want[1][: min(mx, total)])))
    # the caller's buffer behind the records written: a cut inside block 1 (or the middle of the list) and one at c_0
    inside = (cuts[0] + cuts[1]) // 2 if cuts[1] > cuts[0] + 1 else max(total // 2, 1)
    for mx in sorted({inside, cuts[0], total + 3}):
        got_total, buf = raw_check(ctx, case.b.pk, adv, inst, mx)
        keep = min(mx, total)
        assert got_total == total
        assert [tuple(int(x) for x in rec) for rec in buf[:keep]] == want[1][:keep], (name, mx)
        assert (buf[keep:] == 0xA5A5A5A5).all(), "%s: max_failures = %d, a record behind the first %d was written" % (name, mx, keep)


# ------------------------------------------------------------------------------------------------ 3. dynamic lookups: equal keys
def theta_from_source():
    """wc_theta()'s canonical value, read from the kernel source so that these inputs cannot drift from the kernel silently"""
    src = open(os.path.join(ROOT, "halo2-lib_amd", "csrc", "witness_check.hip")).read()
    m = re.search(r"Fr wc_theta\(\) \{\s*Fr t = Fr::zero\(\);\s*t\.l\[0\] = 0x([0-9A-Fa-f]{1,8})u;\s*t\.l\[1\] = 0x([0-9A-Fa-f]{1,8})u;"
                  r"\s*t\.l\[2\] = 0x([0-9A-Fa-f]{1,8})u;\s*return fe_to_mont\(t\);\s*\}", src)
    assert m, "wc_theta() in witness_check.hip no longer has the form these tests read"
    return sum(int(m.group(i + 1), 16) << (32 * i) for i in range(3))


def tuple_hash(t, theta):
    acc = t[0]
    for v in t[1:]:
        acc = (acc * theta + v) % R
    return acc


def tuple_key(t, theta):
    """the search key: limbs 7 .. 1 of the hash (limb 0 of a table key is its row)"""
    return tuple_hash(t, theta) >> 32


class DynCase:
    """ram_circuit(10, 600, 300, key_cols, 2, seed): 300 enabled table rows then the all-zero disabled padding rows; both input sets are
    enabled on rows 0 .. 299, exactly where the table is, so a table row's tuple written into an input row of the same index keeps its last
    (fixed) component"""

    def __init__(self, ctx, key_cols, seed):
        self.m = m = key_cols
        self.circ, self.dp, advice, fixed, self.copies = ram_circuit(10, 600, 300, m, 2, seed)
        self.sh = oracle_shape(self.dp)
        self.u, self.n = self.sh.usable_rows, self.sh.n
        self.advice, self.fixed = [np.array(c) for c in advice], fixed
        en = [_ints(fixed[c][: self.u]) for c in range(3)]
        assert en[0] == en[1] == en[2] == [1] * 300 + [0] * (self.u - 300)
        self.en = en[0]
        self.theta = theta_from_source()
        self.delta = pow(self.theta, -1, R)   # on the last advice component: + 1 on the hash
        self.tab = [_ints(self.advice[j]) for j in range(m)]
        self.kzg = HP.ParamsKZG.setup(ctx, 10, TOXIC_S + seed)
        try:
            self.pk = PL.keygen(self.kzg, self.dp, fixed, self.copies)
        except Exception:
            self.kzg.free()
            raise

    def table_tuple(self, r, tab=None):
        tab = self.tab if tab is None else tab
        return tuple(tab[j][r] for j in range(self.m)) + (self.en[r],)

    def shifted(self, t, d):
        """the tuple t with d * theta^-1 added to its last advice component: hash + d"""
        return t[: self.m - 1] + ((t[self.m - 1] + d * self.delta) % R, t[self.m])

    def free(self):
        self.pk.free()
        self.kzg.free()


def check_dyn_neighbours(ctx, key_cols):
    """every input row r of set 0 holds table row r's tuple with hash + 1, of set 1 with hash + 5: the same search key, another tuple"""
    c = DynCase(ctx, key_cols, 70 + key_cols)
    try:
        m, u, n = c.m, c.u, c.n
        adv = list(c.advice)
        table = {c.table_tuple(r) for r in range(u)}
        for s, d in ((0, 1), (1, 5)):
            tuples = [c.shifted(c.table_tuple(r), d) for r in range(u)]
            same_key = sum(tuple_key(t, c.theta) == tuple_key(c.table_tuple(r), c.theta) for r, t in enumerate(tuples))
            assert same_key >= u - 1, same_key   # (limb 0 of a hash carries into limb 1 with probability d / 2^32)
            assert sum(t not in table for t in tuples) >= u - 1
            for j in range(m):
                adv[m * (1 + s) + j] = _col([t[j] for t in tuples] + [0] * (n - u))
        want = W.check(c.sh, c.fixed, adv, [], c.copies)
        assert sum(1 for f in want[1] if f[0] == W.LOOKUP) >= 2 * (u - 1)
        got = lib_check(c.pk, adv, [], want[0] + 8)
        assert got == want, _first_difference(got, want)
    finally:
        c.free()


def check_dyn_runs(ctx, key_cols):
    """table rows rewritten to T, T + delta, T + 2 delta (one key, three tuples), once among the memory rows and once inside the long run of
    identical padding tuples; the inputs are each of them, T + 3 delta, a padding tuple, and a table tuple with its last component + 1"""
    c = DynCase(ctx, key_cols, 80 + key_cols)
    try:
        m, u, th = c.m, c.u, c.theta
        adv = list(c.advice)
        mem_t, pad_t = c.table_tuple(10), c.table_tuple(400)
        assert pad_t == (0,) * (m + 1) and mem_t[m] == 1
        tab_cells = [dict() for _ in range(m)]
        for base_row, t in ((10, mem_t), (400, pad_t)):
            for i in range(3):
                for j, v in enumerate(c.shifted(t, i)[:m]):
                    tab_cells[j][base_row + i] = v
        for j in range(m):
            adv[j] = _put(adv[j], tab_cells[j])
        tab = [_ints(adv[j]) for j in range(m)]
        table = [c.table_tuple(r, tab) for r in range(u)]
        tset = set(table)
        # the cases meant: one key and three tuples in each run, the fourth not a table tuple, the padding run longer than 256 rows
        for t in (mem_t, pad_t):
            run = [c.shifted(t, i) for i in range(4)]
            assert len({tuple_key(x, th) for x in run}) == 1 and len(set(run)) == 4
            assert all(x in tset for x in run[:3]) and run[3] not in tset
        assert sum(x == pad_t for x in table) > 256 and table[401] != pad_t and table[399] == table[403] == pad_t
        near = table[299][: m - 1] + ((table[299][m - 1] + 1) % R, table[299][m])
        assert near not in tset
        in_cells = [[dict() for _ in range(m)] for _ in range(2)]
        for s, row0, t in ((0, 0, mem_t), (1, 500, pad_t)):   # set 0 rows 0..3 are enabled as the memory rows are, set 1 rows 500..503 are not
            for i in range(4):
                for j, v in enumerate(c.shifted(t, i)[:m]):
                    in_cells[s][j][row0 + i] = v
        for j, v in enumerate(near[:m]):
            in_cells[0][j][4] = v
        for s in range(2):
            for j in range(m):
                a = m * (1 + s) + j
                adv[a] = _put(adv[a], in_cells[s][j])
        want = W.check(c.sh, c.fixed, adv, [], c.copies)
        failed = {(f[1], f[2]) for f in want[1] if f[0] == W.LOOKUP}
        assert not failed & {(0, 0), (0, 1), (0, 2), (1, 500), (1, 501), (1, 502), (1, 600)} and failed >= {(0, 3), (0, 4), (1, 503)}
        got = lib_check(c.pk, adv, [], want[0] + 8)
        assert got == want, _first_difference(got, want)
    finally:
        c.free()


# ------------------------------------------------------------------------------------------------ 4. smaller cases
def check_wide_copy_peers(ctx, shape):
    """copies written here between the last five advice columns (permutation index >= 256) and the constant column: sigma's column is a
    16-bit value in the key and in the write kernel"""
    sh = P.Shape(*shape)
    A, u = sh.num_advice_total, sh.usable_rows
    hi = list(range(A - 5, A))
    pidx = {c: i for i, c in enumerate(sh.perm_columns)}
    assert all(pidx[("advice", a)] >= 256 for a in hi) and sh.lookup_advice[-5:] == hi
    const = ("fixed", sh.constant_cols[0])
    r0 = u - 20   # rows the circuit leaves zero and uncopied in the lookup-advice columns and the constant column
    more = [((const, r0), (("advice", hi[1]), r0 + 1)),                                           # a low column and one >= 256
            ((("advice", hi[0]), r0 + 2), (("advice", hi[4]), r0 + 3)),                           # two columns >= 256
            ((("advice", hi[2]), r0 + 4), (("advice", hi[3]), r0 + 5)), ((("advice", hi[3]), r0 + 5), (const, r0 + 6))]   # a cycle of 3
    b = BaseKey(ctx, shape, seed=4, more_copies=more)
    try:
        assert lib_check(b.pk, b.advice, []) == (0, [])   # (the checker agrees: below it finds the six copy failures and nothing else)
        adv = list(b.advice)
        for a, r in ((hi[1], r0 + 1), (hi[4], r0 + 3), (hi[3], r0 + 5)):   # one cell of each cycle; 1 is a table member
            adv[a] = _put(adv[a], {r: 1})
        want = b.oracle(adv)
        assert want[0] == 6 and all(f[0] == W.COPY for f in want[1])       # per cycle: the pranked cell and the cell whose successor it is
        assert sum(f[3] >= 256 for f in want[1]) >= 4 and sum(f[1] >= 256 and f[3] >= 256 for f in want[1]) >= 3
        assert any(f[1] == 0 and f[3] >= 256 for f in want[1])
        got = lib_check(b.pk, adv, [], 64)
        assert got == want, _first_difference(got, want)
    finally:
        b.free()


def check_hand_built_key(ctx):
    """(7, 2, 1, 1, 1, 5) with q_enable = 1 on every usable row of gate column 0 and on rows u-4 .. u-1 of gate column 1; copies: a
    self-loop, a cycle through three columns, a copy into row u - 1, an instance copy"""
    shape = (7, 2, 1, 1, 1, 5)
    sh = P.Shape(*shape)
    n, u = sh.n, sh.usable_rows
    one = fr([1])[0]
    fixed = [np.zeros((n, 4), dtype=np.uint64) for _ in range(sh.num_fixed_total)]
    fixed[sh.table_col][:32] = fr(list(range(32)))
    fixed[sh.constant_cols[0]][:4] = fr([3, 0, R - 1, 1 << 200])
    fixed[sh.q_enable_cols[0]][:u] = one
    fixed[sh.q_enable_cols[1]][u - 4:u] = one
    la = sh.lookup_advice[0]
    a0, a1 = ("advice", 0), ("advice", 1)
    copies = [((a0, 5), (a0, 5)),
              ((a0, 3), (a1, 9)), ((a1, 9), (("advice", la), 4)),
              ((a1, u - 1), (a0, 2)),
              ((("instance", 0), 0), (a1, 0)),
              ((("fixed", sh.constant_cols[0]), 2), (a1, 20))]
    kzg = HP.ParamsKZG.setup(ctx, 7, TOXIC_S + 9)
    pk = None
    try:
        pk = PL.keygen(kzg, PL.BaseCircuitParams.new(*shape), fixed, copies)
        g = np.random.default_rng(77)
        good = []   # satisfies a[r] + a[r+1] * a[r+2] = a[r+3] wherever three more usable rows exist
        for c in range(2):
            v = [int(x) for x in g.integers(0, 1 << 62, size=3)]
            for r in range(u - 3):
                v.append((v[r] + v[r + 1] * v[r + 2]) % R)
            good.append(_col(v + [0] * (n - u)))
        good.append(_col([r % 32 for r in range(n)]))
        inst_good = [np.array(good[1][:1])]
        cases = {"zero": ([np.zeros((n, 4), dtype=np.uint64) for _ in range(3)], [np.zeros((1, 4), dtype=np.uint64)]),
                 "full_range": ([full_range_fr(n, 500 + c) for c in range(3)], [full_range_fr(2, 510)]),
                 "recurrence": (good, inst_good)}
        for name, (adv, inst) in cases.items():
            want = W.check(sh, fixed, adv, inst, copies)
            gates = [(f[1], f[2]) for f in want[1] if f[0] == W.GATE]
            for c in range(2):   # rows u-3 .. u-1 reach the blinding rows: they fail whatever the values; row u-4 fails on values only
                assert {(c, u - 3), (c, u - 2), (c, u - 1)} <= set(gates), name
                assert ((c, u - 4) in gates) == (name == "full_range"), name
            if name != "full_range":
                assert len(gates) == 6
            assert any(f[0] == W.COPY and f[2] == u - 1 for f in want[1]) == (name != "zero")
            assert not any(f[0] == W.COPY and (f[1], f[2]) == (1 + 0, 5) for f in want[1])   # the self-loop never fails
            got = lib_check(pk, adv, inst, want[0] + 8)
            assert got == want, (name, _first_difference(got, want))
    finally:
        if pk is not None:
            pk.free()
        kzg.free()


def check_device_advice_garbage(ctx):
    """advice_on_device with rows u .. n-1 of every column filled with 0xFF... limbs or out-of-table values: those rows are ignored"""
    b = BaseKey(ctx, (7, 2, 2, 1, 1, 5), seed=3)
    try:
        sh, u, n = b.sh, b.sh.usable_rows, b.sh.n
        la = sh.lookup_advice[0]
        pranked = list(b.advice)
        pranked[0] = _put(pranked[0], {9: 12345, u - 1: 6})
        pranked[la] = _put(pranked[la], {u - 1: 1 << 64, 2: 77})
        for name, clean in (("honest", b.advice), ("pranked", pranked)):
            want = b.oracle(clean)
            assert (want[0] == 0) == (name == "honest")
            dirty = []
            for c, col in enumerate(clean):
                col = np.array(col)
                if c % 2 == 0:
                    col[u:] = np.uint64(0xFFFFFFFFFFFFFFFF)    # no field element at all
                else:
                    col[u:] = fr([(1 << 200) + c])[0]           # a field element outside every table
                dirty.append(col)
            host = lib_check(b.pk, dirty, b.instances, want[0] + 8)
            dev = [ctx.to_device(col) for col in dirty]
            try:
                got = lib_check(b.pk, dev, b.instances, want[0] + 8, advice_on_device=True)
            finally:
                for p in dev:
                    ctx.free(p)
            assert host == want, (name, _first_difference(host, want))
            assert got == want, (name, _first_difference(got, want))
    finally:
        b.free()


def check_rlc_gate_edge(ctx, k, lookup_bits):
    """h2hip_plonk_check_witness_challenges on rlc_checks.shape_a: the RLC gate reads rows r .. r + 2, so row u - 3 is the last it can hold on
    (a flex gate there reaches the blinding rows).  keygen refuses q_rlc on rows u - 2 and u - 1 (include/h2hip.h), so no key can carry
    them: those two refusals are asserted here, and the expected list for q_rlc on u - 5 (values that do not satisfy it) and u - 3
    (values that do) is written out by hand from the contract."""
    import halo2_lib_amd as H
    from tests import rlc_checks as RC
    from tests import shape_oracle as SO

    params, _ = RC.shape_a(k, lookup_bits)
    sh = SO.Shape.rlc(params)
    n, u = sh.n, sh.usable_rows
    one = fr([1])[0]
    gate_adv, rlc_adv = 0, sh.rlc_advice[0]
    q_enable, q_rlc = sh.q_enable_cols[0], sh.q_rlc_cols[0]
    assert sh.num_advice_total == 2 and rlc_adv == 1

    def fixed_with(rlc_rows):
        fixed = [np.zeros((n, 4), dtype=np.uint64) for _ in range(sh.num_fixed_total)]   # the table holds 0 alone; q_lookup is 0 everywhere
        fixed[q_enable][[0, u - 3]] = one   # the flex gate at u - 3 fails whatever the values; the selectors share row u - 3
        fixed[q_rlc][rlc_rows] = one
        return fixed

    kzg = HP.ParamsKZG.setup(ctx, k, TOXIC_S + 21)
    pk = None
    try:
        for rows in ([u - 3, u - 2, u - 1], [u - 3, u - 2], [u - 3, u - 1]):
            try:
                PL.keygen(kzg, params, fixed_with(rows), []).free()
            except H.H2HipError as e:
                assert e.code == RC.ERR_INVALID and "q_rlc" in str(e), str(e)
            else:
                raise AssertionError("keygen accepted q_rlc on rows %s" % rows)
        pk = PL.keygen(kzg, params, fixed_with([u - 5, u - 3]), [])
        gamma = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
        x, y = 1 << 250, R - 5
        cells = {u - 3: x, u - 2: y, u - 1: (x * gamma + y) % R}   # holds at u - 3; at u - 5: 0 * gamma + 0 - x != 0
        adv = [np.zeros((n, 4), dtype=np.uint64), _put(np.zeros((n, 4), dtype=np.uint64), cells)]
        want = (2, [(W.GATE, gate_adv, u - 3, 0, 0), (W.GATE, rlc_adv, u - 5, 0, 0)])   # the RLC gates behind the flex gates
        got = lib_check(pk, adv, [], 16, challenges=[gamma])
        assert got == want, got
        adv[1] = _put(adv[1], {u - 1: (x * gamma + y + 1) % R})   # now row u - 3 fails on its values
        want = (3, [(W.GATE, gate_adv, u - 3, 0, 0), (W.GATE, rlc_adv, u - 5, 0, 0), (W.GATE, rlc_adv, u - 3, 0, 0)])
        got = lib_check(pk, adv, [], 16, challenges=[gamma])
        assert got == want, got
    finally:
        if pk is not None:
            pk.free()
        kzg.free()
