"""Flex-gate chains filled on the device (h2hip_gate_fill_chains_dev: the cells s_0, a_1, b_1, s_1, ... with s_i = s_{i-1} + a_i * b_i of
GateChip's inner products, sums and selections), shared by tests/test_gate_chains.py (the CPU-emulated build) and tests/test_gate_chains_gpu.py:
every check takes a ctx.

  A  the fill against its definition, restated here in Python integers, over sentinel-filled columns (a stray write fails);
  B  every refusal: H2HIP_ERR_INVALID, its reason in h2hip_last_error, the columns untouched, a good call afterwards;
  C  the reference's own inner_product / inner_product_left / inner_product_with_sums answers (tests/golden/flex_gate_reference_kats.json);
  D  a chain broken over two columns by halo2_lib_amd/virtual_region.py's assign_witnesses against head + carry pieces from the same break point;
  E  SelectCircuit: an RLC circuit whose phase-1 gate columns hold select_by_indicator chains over the RLC chains' running sums, proven with
     phase 1 written by rlc_fill_chains + gate_fill_chains against the same proof with phase 1 computed in Python integers.
"""
import ctypes as C
import json
import os
import re

import numpy as np

from halo2_lib_amd import plonk as PL
from halo2_lib_amd import virtual_region as VR
from oracle import bn254 as O
from tests import rlc_checks as RC
from tests.dyn_lookup_util import rng_budget, srs, vk_from_gpu
from tests.util import PreDrawnRng, R, fr, full_range_fr

_vp = C.c_void_p
CARRY, JOIN, START_A = PL.GATE_CARRY, PL.GATE_JOIN, PL.GATE_START_A
ERR_INVALID = -1
SENTINEL = RC.SENTINEL
T = 2048   # pairs per scan tile (gate_chains.hip: 256 lanes x GATE_J = 8)
P = 512    # tiles one pass of the tile-totals level covers (its one workgroup's lanes; beyond it every lane takes a run of tiles)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ints(limbs):
    return O.limbs_to_ints(np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4), R)


def cell_count(ln, flags):
    return 3 * ln - 2 if flags & START_A else 3 * ln if flags & JOIN else 3 * ln + 1


# ------------------------------------------------------------------------------------------------ the fill's definition
def gate_cells(pieces, a, b):
    """{(column, row): value} of the four piece forms for (column, row, len, flags, a_offset, b_offset, a_stride, b_stride) pieces over integer
    operands: head 0, a_0, b_0, s_0, ...; START_A head a_0, a_1, b_1, s_1, ... (s_0 = a_0); carry s_prev, a_0, b_0, s_0', ...; join
    a_0, b_0, s_0', ... — s the running sum of the chain, which a head starts and carry and join pieces continue"""
    cells, s = {}, None

    def put(col, row, v):
        assert (col, row) not in cells, "the test's own pieces overlap at %s" % ((col, row),)
        cells[(col, row)] = v

    for (col, row, ln, flags, ao, bo, ast, bst) in pieces:
        first, r = 0, row + 1
        if flags & START_A:
            s = a[ao]
            put(col, row, s)
            first = 1
        elif flags & CARRY:
            put(col, row, s)
        elif flags & JOIN:
            r = row
        else:
            s = 0
            put(col, row, 0)
        for i in range(first, ln):
            av, bv = a[ao + i * ast], b[bo + i * bst]
            s = (s + av * bv) % R
            put(col, r, av)
            put(col, r + 1, bv)
            put(col, r + 2, s)
            r += 3
    return cells


def write_expected(want, pieces, a_raw, b_raw, a_int, b_int):
    """the same definition written straight into the (n, 4) limb columns `want`: the a and b cells are copies of the operands' limbs, so only
    the sums are converted (the calls of a million pairs would spend their time in a dict)"""
    s = None
    for (col, row, ln, flags, ao, bo, ast, bst) in pieces:
        ia, ib = ao + ast * np.arange(ln, dtype=np.int64), bo + bst * np.arange(ln, dtype=np.int64)
        first, r = 0, row + 1
        if flags & START_A:
            s = a_int[ao]
            want[col][row] = a_raw[ao]
            first = 1
        elif flags & CARRY:
            want[col][row] = fr([s])[0]
        elif flags & JOIN:
            r = row
        else:
            s = 0
            want[col][row] = 0
        sums = []
        for i in range(first, ln):
            s = (s + a_int[ia[i]] * b_int[ib[i]]) % R
            sums.append(s)
        m = ln - first
        if m:
            want[col][r:r + 3 * m:3] = a_raw[ia[first:]]
            want[col][r + 1:r + 1 + 3 * m:3] = b_raw[ib[first:]]
            want[col][r + 2:r + 2 + 3 * m:3] = fr(sums)
    return s


class _Layout:
    """pieces laid down the columns in list order: add() returns the piece's first position in the stream of pairs"""

    def __init__(self, first_free):
        self.rows, self.pieces, self.pos, self.prev = list(first_free), [], 0, None

    def add(self, col, ln, flags=0, gap=0):
        if flags & JOIN:
            col, row = self.prev
            assert self.rows[col] == row
        else:
            row = self.rows[col] + gap
        end = row + cell_count(ln, flags)
        self.pieces.append((col, row, ln, flags))
        self.rows[col], self.prev = end, (col, end)
        start, self.pos = self.pos, self.pos + ln
        return start


def _operand_pool(nvals, seed):
    """integers uniform over [0, r) with 0, 1 and r - 1 on about one position in eight, and their Montgomery limbs"""
    vals = _ints(full_range_fr(nvals, seed))
    g = np.random.default_rng(seed + 1)
    for p in g.integers(0, nvals, size=nvals // 8):
        vals[int(p)] = (0, 1, R - 1)[int(p) % 3]
    vals[0:3] = [0, 1, R - 1]
    return vals, fr(vals)


def _with_operands(pieces, na, nb, seed):
    """(column, row, len, flags) -> the 8-tuples: strides 0..3 on either operand in turn (all 16 pairs), offsets anywhere the reads fit"""
    g = np.random.default_rng(seed)
    out = []
    for j, (col, row, ln, flags) in enumerate(pieces):
        ast, bst = j % 4, (j // 4) % 4
        ao = int(g.integers(0, na - (ln - 1) * ast))
        bo = int(g.integers(0, nb - (ln - 1) * bst))
        out.append((col, row, ln, flags, ao, bo, ast, bst))
    return out


def fill_case():
    """Check A's one call.  Three columns of 2^16 rows; b_dev is column 2 itself, whose first NB rows hold the right operands (no piece
    writes them; carry pieces lie further down that column), a_dev a buffer of its own.  In stream order: a chain of T - 1 pairs; a
    one-pair chain at the last position of tile 0; a chain of T pairs from the first position of tile 1, which ends with the tile, and its
    carry piece; chains of T + 1 and 3 T + 5 pairs; chains of 2 pairs, START_A chains of 1 and 2 pairs; a filler up to the next tile start,
    then 300 chains of 1..9 pairs inside that tile; head + join; head + carry + join; a longer START_A chain with a carry."""
    n = 1 << 16
    u = n - 7
    na = nb = 24000
    lay = _Layout([0, 0, nb + 5])
    where = {}
    lay.add(0, T - 1)
    where["head at the last position of a tile"] = lay.add(0, 1, gap=1)
    where["head at the first position of a tile"] = lay.add(0, T, gap=2)
    where["carry after a piece that ends with its tile"] = lay.add(2, 2, CARRY)
    lay.add(0, T + 1)
    lay.add(1, 3 * T + 5, gap=3)
    lay.add(0, 2, gap=1)
    lay.add(0, 1, START_A)
    lay.add(0, 2, START_A, gap=2)
    lay.add(1, 2)
    lay.add(1, T - lay.pos % T, gap=1)            # filler: the next piece starts a tile
    where["300 chains in one tile"] = lay.pos
    g = np.random.default_rng(0x6A7E)
    for j, ln in enumerate(g.integers(1, 10, size=300)):
        lay.add(0, int(ln), START_A if j % 5 == 4 else 0, gap=j % 3)
    where["300 chains end"] = lay.pos
    lay.add(0, 5)
    lay.add(0, 4, JOIN)
    lay.add(1, 3, gap=2)
    lay.add(2, 4, CARRY, gap=1)
    lay.add(2, 2, JOIN)
    lay.add(1, 7, START_A)
    lay.add(2, 300, CARRY, gap=2)
    assert where["head at the last position of a tile"] == T - 1 and where["head at the first position of a tile"] == T
    assert where["carry after a piece that ends with its tile"] == 2 * T
    assert where["300 chains in one tile"] % T == 0 and where["300 chains end"] - where["300 chains in one tile"] <= T
    assert max(lay.rows) <= u, (lay.rows, u)
    return n, u, na, nb, _with_operands(lay.pieces, na, nb, 0x0DD)


def _expected_columns(n, ncols, pieces, a_raw, b_raw, a_int, b_int, b_column=None):
    want = [np.tile(SENTINEL, (n, 1)) for _ in range(ncols)]
    if b_column is not None:
        want[b_column][: len(b_raw)] = b_raw
    write_expected(want, pieces, a_raw, b_raw, a_int, b_int)
    return want


def _compare(ctx, d_cols, want, what):
    for c, p in enumerate(d_cols):
        got = ctx.download(p, want[c].shape)
        if not np.array_equal(got, want[c]):
            bad = np.nonzero((got != want[c]).any(axis=1))[0]
            raise AssertionError("%s: column %d: %d cells differ, first rows %s" % (what, c, len(bad), bad[:8].tolist()))


def check_fill(ctx):
    """A: h2hip_gate_fill_chains_dev over fill_case(): every addressed cell equals the definition's, every other cell keeps what it held"""
    n, u, na, nb, pieces = fill_case()
    a_int, a_raw = _operand_pool(na, 0xA1)
    b_int, b_raw = _operand_pool(nb, 0xB1)
    want = _expected_columns(n, 3, pieces, a_raw, b_raw, a_int, b_int, b_column=2)
    # the dict form of the definition gives the same columns (write_expected is what the calls of a million pairs use)
    cells = gate_cells(pieces, a_int, b_int)
    for c in range(3):
        ref = np.tile(SENTINEL, (n, 1))
        if c == 2:
            ref[:nb] = b_raw
        rows = sorted(r for (cc, r) in cells if cc == c)
        ref[rows] = fr([cells[(c, r)] for r in rows])
        assert np.array_equal(ref, want[c]), "the two statements of the definition differ in column %d" % c
    start = [np.tile(SENTINEL, (n, 1)) for _ in range(3)]
    start[2][:nb] = b_raw
    d_cols = [ctx.to_device(c) for c in start]
    d_a = ctx.to_device(a_raw)
    try:
        PL.gate_fill_chains(ctx, d_cols, u, d_a, na, d_cols[2], nb, pieces)
        ctx.sync()
        _compare(ctx, d_cols, want, "check A")
    finally:
        for p in d_cols + [d_a]:
            ctx.free(p)


def large_case(pairs):
    """`pairs` pairs as a one-pair chain, one chain of pairs - 4 (a head, join pieces and one carry piece into column 1, each of at most
    60,000 pairs over a pool of 2^16 operands) and a chain of 3"""
    na = nb = 1 << 16
    big = pairs - 4
    lens = [60000] * (big // 60000) + ([big % 60000] if big % 60000 else [])
    half = len(lens) // 2
    lay = _Layout([0, 0])
    lay.add(0, 1)
    for j, ln in enumerate(lens):
        if j == 0:
            lay.add(0, ln, gap=2)
        elif j == half:
            lay.add(1, ln, CARRY, gap=1)
        else:
            lay.add(0, ln, JOIN)
    lay.add(0, 3, gap=1)
    assert lay.pos == pairs
    g = np.random.default_rng(pairs)
    pieces = [(col, row, ln, flags, int(g.integers(0, na - ln)), int(g.integers(0, nb - ln)), 1, 1) for (col, row, ln, flags) in lay.pieces]
    return max(lay.rows) + 9, na, nb, pieces


def check_fill_large(ctx, pairs):
    """A, second call: the tile-totals level at `pairs` / T tiles ((P - 1) T, P T and (P + 1) T + 3 pairs: a lane of its workgroup takes one
    tile, every lane takes one, lanes take two)"""
    n, na, nb, pieces = large_case(pairs)
    a_int, a_raw = _operand_pool(na, 0xA2)
    b_int, b_raw = _operand_pool(nb, 0xB2)
    want = _expected_columns(n, 2, pieces, a_raw, b_raw, a_int, b_int)
    sent = np.tile(SENTINEL, (n, 1))
    d_cols = [ctx.to_device(sent), ctx.to_device(sent)]
    d_a, d_b = ctx.to_device(a_raw), ctx.to_device(b_raw)
    try:
        PL.gate_fill_chains(ctx, d_cols, n - 2, d_a, na, d_b, nb, pieces)
        ctx.sync()
        _compare(ctx, d_cols, want, "%d pairs" % pairs)
    finally:
        for p in d_cols + [d_a, d_b]:
            ctx.free(p)


# ------------------------------------------------------------------------------------------------ B: the refusals
def check_rejections(ctx):
    """one case per refusal of include/h2hip.h's list: H2HIP_ERR_INVALID, the reason in h2hip_last_error, the sentinel everywhere; then the
    largest pieces that still fit, from the same context"""
    import halo2_lib_amd as H

    n, u, nvals = 64, 57, 40
    a_int, a_raw = _operand_pool(nvals, 0xC1)
    b_int, b_raw = _operand_pool(nvals, 0xC2)
    sent = np.tile(SENTINEL, (n, 1))
    d_cols = [ctx.to_device(sent), ctx.to_device(sent), ctx.to_device(sent)]
    d_a, d_b = ctx.to_device(a_raw), ctx.to_device(b_raw)
    ok = (0, 0, 3, 0, 0, 0, 1, 1)                    # 10 cells: rows 0..9 of column 0
    big = 1 << 31
    bad = [
        ("unknown flags", "unknown piece flags", [ok, (1, 0, 3, 8, 0, 0, 1, 1)]),
        ("CARRY and JOIN", "more than one of", [ok, (0, 10, 3, CARRY | JOIN, 0, 0, 1, 1)]),
        ("START_A and CARRY", "more than one of", [ok, (1, 0, 3, START_A | CARRY, 0, 0, 1, 1)]),
        ("CARRY on piece 0", "piece 0", [(0, 0, 3, CARRY, 0, 0, 1, 1)]),
        ("JOIN on piece 0", "piece 0", [(0, 0, 3, JOIN, 0, 0, 1, 1)]),
        ("len == 0", "len == 0", [ok, (1, 0, 0, 0, 0, 0, 1, 1)]),
        ("column index out of range", "column index", [ok, (3, 0, 3, 0, 0, 0, 1, 1)]),
        ("head leaves the usable rows", "usable rows", [ok, (1, u - 9, 3, 0, 0, 0, 1, 1)]),               # 10 cells from row u - 9
        ("START_A head leaves the usable rows", "usable rows", [ok, (1, u - 6, 3, START_A, 0, 0, 1, 1)]),   # 7 cells from row u - 6
        ("carry leaves the usable rows", "usable rows", [ok, (1, u - 9, 3, CARRY, 0, 0, 1, 1)]),
        ("join leaves the usable rows", "usable rows", [(1, u - 12, 1, 0, 0, 0, 1, 1), (1, u - 8, 3, JOIN, 0, 0, 1, 1)]),   # 9 cells from row u - 8
        ("join one row too low", "join piece", [ok, (0, 11, 3, JOIN, 0, 0, 1, 1)]),
        ("join in another column", "join piece", [ok, (1, 10, 3, JOIN, 0, 0, 1, 1)]),
        ("left operands past a_len", "left operands", [ok, (1, 0, 3, 0, nvals - 2, 0, 1, 1)]),
        ("right operands past b_len by the stride", "right operands", [ok, (1, 0, 3, 0, 0, nvals - 5, 1, 3)]),
        ("an offset that wraps in 64 bits", "left operands", [ok, (1, 0, 3, 0, (1 << 64) - 1, 0, 1, 1)]),
        ("a stride that leaves 32 bits", "right operands", [ok, (1, 0, 3, 0, 0, 1, 1, 0xFFFFFFFF)]),
        ("two pieces overlap", "overlap", [ok, (0, 9, 3, 0, 0, 0, 1, 1)]),
        ("a piece inside another", "overlap", [(0, 0, 9, 0, 0, 0, 1, 1), (1, 0, 1, 0, 0, 0, 1, 1), (0, 4, 1, START_A, 0, 0, 1, 1)]),
    ]
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

        for what, reason, pieces in bad:
            refused(what, reason, lambda: PL.gate_fill_chains(ctx, d_cols, u, d_a, nvals, d_b, nvals, pieces))
        # more than 2^32 pairs: three constant-operand pieces in rows that only an (unreal) usable_rows of 2^40 holds; refused before any launch
        huge = [(0, 0, big, 0, 0, 0, 0, 0), (1, 0, big, 0, 0, 0, 0, 0), (2, 0, 1, 0, 0, 0, 0, 0)]
        refused("more than 2^32 pairs", "2^32 pairs", lambda: PL.gate_fill_chains(ctx, d_cols, 1 << 40, d_a, nvals, d_b, nvals, huge))
        # a NULL column, NULL operands, a NULL piece list
        refused("a NULL column", "column index", lambda: PL.gate_fill_chains(ctx, [d_cols[0], 0, d_cols[2]], u, d_a, nvals, d_b, nvals, [ok, (1, 0, 3, 0, 0, 0, 1, 1)]))
        refused("a_dev NULL", "NULL argument", lambda: PL.gate_fill_chains(ctx, d_cols, u, 0, nvals, d_b, nvals, [ok]))
        refused("b_dev NULL", "NULL argument", lambda: PL.gate_fill_chains(ctx, d_cols, u, d_a, nvals, 0, nvals, [ok]))
        cols = (_vp * 3)(*[_vp(int(p)) for p in d_cols])
        refused("chains NULL", "NULL argument",
                lambda: ctx._chk(ctx.lib.h2hip_gate_fill_chains_dev(ctx.handle, cols, 3, u, _vp(int(d_a)), nvals, _vp(int(d_b)), nvals, None, 1)))
        # operands inside cells this call writes: a_dev is column 1, read at rows 20..22 and 24..28, written at rows 18..27 / at rows 0..9
        refused("a operand range meets written cells", "operand range",
                lambda: PL.gate_fill_chains(ctx, d_cols, u, d_cols[1], u, d_b, nvals, [ok, (1, 18, 3, 0, 20, 0, 1, 1)]))
        refused("b operand range meets another piece's cells", "operand range",
                lambda: PL.gate_fill_chains(ctx, d_cols, u, d_a, nvals, d_cols[1], u, [(1, 0, 3, 0, 0, 0, 1, 1), (0, 0, 3, 0, 0, 9, 1, 2)]))
        # count == 0 needs nothing
        PL.gate_fill_chains(ctx, d_cols, u, 0, 0, 0, 0, [])
        # the largest pieces that still fit (each form ends on row u - 1), a START_A piece of one pair whose b_offset is the last element, and
        # operands that end with a_len / b_len
        pieces = [(0, u - 10, 3, 0, nvals - 3, nvals - 7, 1, 3), (1, u - 10, 3, CARRY, nvals - 5, 0, 2, 0), (2, u - 7, 3, START_A, 0, nvals - 3, 0, 1),
                  (2, 0, 1, 0, 1, 2, 3, 3), (2, 4, 3, JOIN, 5, 6, 1, 1), (0, 0, 1, START_A, nvals - 1, nvals - 1, 1, 1)]
        PL.gate_fill_chains(ctx, d_cols, u, d_a, nvals, d_b, nvals, pieces)
        ctx.sync()
        _compare(ctx, d_cols, _expected_columns(n, 3, pieces, a_raw, b_raw, a_int, b_int), "after the refusals")
    finally:
        for p in d_cols + [d_a, d_b]:
            ctx.free(p)


# ------------------------------------------------------------------------------------------------ C: the reference's answers
def check_reference_kats(ctx):
    """inner_product, inner_product_left and inner_product_with_sums of tests/golden/flex_gate_reference_kats.json through both head forms:
    the last cell is the recorded result, the s cells the recorded sums.  START_A is the reference's "b starts with Constant(1)" form
    (flex_gate/mod.rs:953-962): where only a starts with 1 the operands swap sides, as the inner product allows."""
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "flex_gate_reference_kats.json")))["cases"]
    val = lambda v: (R - v["neg"]) % R if isinstance(v, dict) else v % R
    cases = [c for c in kats if c["op"] in ("inner_product", "inner_product_left", "inner_product_with_sums")]
    assert {c["op"] for c in cases} == {"inner_product", "inner_product_left", "inner_product_with_sums"}
    n = 64
    for c in cases:
        a, b = [val(v) for v in c["inputs"][0]], [val(v) for v in c["inputs"][1]]
        ln = len(a)
        for form in (0, START_A):
            if form == START_A and b[0] != 1:
                assert a[0] == 1, c
                a, b = b, a
            d_col = ctx.to_device(np.tile(SENTINEL, (n, 1)))
            d_a, d_b = ctx.to_device(fr(a)), ctx.to_device(fr(b))
            try:
                PL.gate_fill_chains(ctx, [d_col], n - 7, d_a, ln, d_b, ln, [(0, 2, ln, form, 0, 0, 1, 1)])
                got = _ints(ctx.download(d_col, (n, 4))[2:2 + cell_count(ln, form)])
            finally:
                for p in (d_col, d_a, d_b):
                    ctx.free(p)
            sums = got[3::3] if form == 0 else got[0::3]
            if c["op"] == "inner_product_with_sums":
                assert sums == [val(v) for v in c["expected"]], (c, form, sums)
            else:
                assert got[-1] == val(c["expected"]), (c, form, got[-1])
                assert got[-1] == sums[-1]


# ------------------------------------------------------------------------------------------------ D: column breaks
def chain_stream(ln, start_a, a, b):
    """the flat cell stream of one chain, as GateChip writes it into a Context"""
    if start_a:
        s, out, first = a[0], [a[0]], 1
    else:
        s, out, first = 0, [0], 0
    for i in range(first, ln):
        s = (s + a[i] * b[i]) % R
        out += [a[i], b[i], s]
    return out


def split_at_break(column_after, row, ln, start_a, break_row, ao, bo):
    """the head and carry pieces of a chain of ln pairs whose first cell is at (0, row) when the column is left at break_row and the chain
    goes on from row 0 of column_after: the break must fall on an s cell behind which pairs remain (there a carry piece starts)"""
    # a plain head's s cells are at row + 3 k for k = 1 .. ln (k pairs done); a START_A head's at row + 3 k for k = 0 .. ln - 1 (k + 1 done, a_0 included)
    k, rem = divmod(break_row - row, 3)
    done = k + 1 if start_a else k
    if rem or not 1 <= done < ln:
        raise ValueError("the break at row %d is not on an s cell of the chain at row %d with pairs left behind it" % (break_row, row))
    return [(0, row, done, START_A if start_a else 0, ao, bo, 1, 1), (column_after, 0, ln - done, CARRY, ao + done, bo + done, 1, 1)]


def check_column_break(ctx, start_a):
    """a thread of three chains laid over two columns by assign_witnesses with the break on an s cell of the second; the device columns from
    head / head + carry / head pieces equal the mirror's"""
    lens = [4, 9, 3]
    a_int, a_raw = _operand_pool(sum(lens), 0xD1)
    b_int, b_raw = _operand_pool(sum(lens), 0xD2)
    thread = VR.Context(True, "gate", 0, VR.CopyConstraintManager())
    starts, offs, off = [], [], 0
    for ln in lens:
        starts.append(len(thread.advice))
        offs.append(off)
        thread.advice += chain_stream(ln, start_a, a_int[off:off + ln], b_int[off:off + ln])
        off += ln
    break_row = starts[1] + 3 * 4                         # an s cell inside the second chain
    n = 64
    region = VR.Region(n, 2)
    VR.assign_witnesses([thread], [0, 1], region, [break_row])
    form = START_A if start_a else 0
    pieces = [(0, starts[0], lens[0], form, offs[0], offs[0], 1, 1)]
    pieces += split_at_break(1, starts[1], lens[1], start_a, break_row, offs[1], offs[1])
    carry_cells = cell_count(pieces[-1][2], CARRY)
    pieces.append((1, carry_cells, lens[2], form, offs[2], offs[2], 1, 1))
    want = [np.tile(SENTINEL, (n, 1)) for _ in range(2)]
    for c in range(2):
        rows = sorted(region.advice[c])
        want[c][rows] = fr([region.advice[c][r] for r in rows])
    assert len(region.advice[0]) == break_row + 1 and len(region.advice[1]) == len(thread.advice) - break_row
    d_cols = [ctx.to_device(np.tile(SENTINEL, (n, 1))) for _ in range(2)]
    d_a, d_b = ctx.to_device(a_raw), ctx.to_device(b_raw)
    try:
        PL.gate_fill_chains(ctx, d_cols, n - 7, d_a, len(a_int), d_b, len(b_int), pieces)
        ctx.sync()
        _compare(ctx, d_cols, want, "column break (start_a = %s)" % start_a)
    finally:
        for p in d_cols + [d_a, d_b]:
            ctx.free(p)
    for bad_row in (break_row + 1, starts[1] + 3 * lens[1] if not start_a else starts[1] + 3 * (lens[1] - 1)):
        try:
            split_at_break(1, starts[1], lens[1], start_a, bad_row, 0, 0)
        except ValueError:
            pass
        else:
            raise AssertionError("split_at_break accepted row %d" % bad_row)


# ------------------------------------------------------------------------------------------------ E: inside a proof
class SelectCircuit(RC.RlcCircuit):
    """RlcCircuit(num_advice_per_phase [1, 2], lookup advice in phase 0, one RLC column) whose two phase-1 gate columns (advice 1 and 2)
    hold select_by_indicator chains over the RLC column's running sums r: chain c picks r[len_c - 1] of one RLC chain as
    sum_i r_i * bit_i with bit_i = (i == len_c - 1).  Every chain starts with the constant 0; its a cells are copies of the r cells (stride 2
    in the RLC column), its b cells copies of indicator bits in the phase-0 gate column (stride 1), q_enable is set on every third row.

      over the chain [1, 0]                       max 2,        len 2   column 1
      over the chain of 5                         max 5,        len 3   column 1
      over the chain of 5                         max 1,        len 1   column 1   (a chain of one pair)
      over the chain of 3 + its carry piece of 2  max 5,        len 4   column 1   (a head piece and a join piece: the r cells change place)
      over the long chain                         max long_len, len long_len   column 1 from there to its last usable rows, then a carry
                                                                                   piece from row 0 of column 2

    The indicator bits replace the first rows of the phase-0 column (blocks [a, b, c, a + b c] of bits: all zero, or 0 0 1 0 / 0 1 0 0 where
    a chain's set bit falls — a run is moved down a row or two until it does); the RLC chains' values, copies of phase-0 cells, follow."""

    def __init__(self, params, seed, chains=None):
        """chains: (pairs, len, [(first r row in the RLC column, count), ...]) per select chain, laid down the phase-1 gate columns in order
        (default: the five chains above)"""
        super().__init__(params, seed)
        assert self.nr == 1 and self.gate_phase[0] == 0 and set(self.gate_phase[1:]) == {1}
        u, rlc = self.u, self.rlc[0]
        gcols = list(range(1, self.G))
        heads = {p[1]: p for p in self.pieces if not p[3] & RC.CARRY}
        long_len = heads[28][2]
        if chains is None:
            chains = [(2, 2, [(0, 2)]), (5, 3, [(3, 5)]), (1, 1, [(3, 1)]), (5, 4, [(12, 3), (22, 2)]), (long_len, long_len, [(28, long_len)])]
        # ---- the indicator bits in the phase-0 column
        bits, self.bit_rows, last_block = [], [], -1
        for (mx, ln, _src) in chains:
            while (len(bits) + ln - 1) % 4 not in (1, 2) or (len(bits) + ln - 1) // 4 == last_block:   # the set bit on position 1 or 2 of a block of its own
                bits.append(0)
            self.bit_rows.append(len(bits))
            last_block = (len(bits) + ln - 1) // 4
            bits += [1 if i == ln - 1 else 0 for i in range(mx)]
        bits += [0] * (-len(bits) % 4)
        assert len(bits) <= 4 * self.blocks - 64, "the bits leave no phase-0 cells for the RLC chains' values"
        for i in range(0, len(bits), 4):
            assert bits[i + 3] == bits[i] + bits[i + 1] * bits[i + 2]
        self.small[0] = bits + list(self.small[0][len(bits):])
        self.values = [v if c is None else self.small[0][c] for v, c in zip(self.values, self.value_cells)]
        # ---- the select pieces: (column, row, len, flags, a_offset, b_offset, a_stride, b_stride), a over the RLC column, b over the phase-0 column
        self.gate_pieces, self.last_cells = [], []
        gi, row = 0, 0
        for (mx, ln, src), b0 in zip(chains, self.bit_rows):
            done = 0
            for (r0, cnt) in src:
                form = JOIN if done else 0
                take = min(cnt, (u - row - (0 if form else 1)) // 3)
                assert take >= 1
                self.gate_pieces.append((gcols[gi], row, take, form, r0, b0 + done, 2, 1))
                row += cell_count(take, form)
                if take < cnt:                              # the column is full: the break cell again at the top of the next one
                    assert row > u - 3
                    gi, row = gi + 1, cell_count(cnt - take, CARRY)
                    self.gate_pieces.append((gcols[gi], 0, cnt - take, CARRY, r0 + 2 * take, b0 + done + take, 2, 1))
                done += cnt
            self.last_cells.append((gcols[gi], row - 1))
        self.chains = chains
        # ---- copies: none of the parents' on the phase-1 gate columns; the chains' instead
        gadv = {("advice", c) for c in gcols}
        self.copies = [c for c in self.copies if not any(cell[0] in gadv for cell in c)]
        const0 = (("fixed", self.sh.constant_cols[0]), 0)
        self.q_rows = {c: [] for c in gcols}
        prev_last = None
        for (col, row, ln, flags, ao, bo, ast, bst) in self.gate_pieces:
            adv = ("advice", col)
            r = row
            if flags & CARRY:
                self.copies.append(((adv, row), prev_last))
                r += 1
            elif not flags & JOIN:
                self.copies.append(((adv, row), const0))
                r += 1
            for i in range(ln):
                self.copies.append(((adv, r + 3 * i), (("advice", rlc), ao + i * ast)))
                self.copies.append(((adv, r + 3 * i + 1), (("advice", 0), bo + i * bst)))
                self.q_rows[col].append(r + 3 * i - 1)
            prev_last = (adv, r + 3 * ln - 1)
        assert all(self.q_rows[c][:1] == [0] for c in gcols)           # keygen's selector rule: every gate column enabled on row 0
        self.fixed = self._fixed()

    def _fixed(self):
        if not hasattr(self, "q_rows"):
            return None
        base = super()._fixed()
        one = fr([1])[0]
        for (qc, ac) in self.sh.gates:
            if ac in self.q_rows:
                base[qc][:] = 0
                base[qc][self.q_rows[ac]] = one
        return base

    def select_columns(self, gamma):
        """the phase-1 gate columns' integer values, from the definition over the RLC column's integers"""
        cells = gate_cells(self.gate_pieces, self.rlc_columns(gamma)[0], self.small[0])
        cols = {c: [0] * self.n for c in range(1, self.G)}
        for (c, r), v in cells.items():
            cols[c][r] = v
        return [cols[c] for c in range(1, self.G)]

    def phase_values(self, phase, challenges):
        out = super().phase_values(phase, challenges)
        if phase == 1:
            out = self.select_columns(challenges[0]) + out[self.G - 1:]
        return out

    def selected(self, gamma):
        """r[len - 1] of every select chain, from the RLC column in Python integers"""
        r = self.rlc_columns(gamma)[0]
        out = []
        for (mx, ln, src) in self.chains:
            rows = [r0 + 2 * i for (r0, cnt) in src for i in range(cnt)]
            out.append(r[rows[ln - 1]])
        return out


def select_params(k, lookup_bits):
    return PL.RlcCircuitParams.new(k, [1, 2], [1, 0], 1, 0, lookup_bits, [1], 1)


def check_select_proof(ctx, k, lookup_bits, seed):
    """E: the proof with phase 1 written on the device (rlc_fill_chains, then gate_fill_chains with a_dev the RLC column and b_dev the resident
    phase-0 column) has the bytes of the proof with phase 1 computed in Python integers and uploaded; both verifiers accept it, check_witness
    finds no failure, every chain's last cell is r[len - 1]"""
    params = select_params(k, lookup_bits)
    circ = SelectCircuit(params, seed)
    assert any(p[3] & CARRY for p in circ.gate_pieces) and any(p[3] & JOIN for p in circ.gate_pieces)
    assert {1, circ.chains[-1][0]} <= {ln for (_mx, ln, _src) in circ.chains}       # the lengths include 1 and the maximum
    kzg, srs_params = srs(ctx, k, seed)
    gpk = PL.keygen(kzg, params, circ.fixed, circ.copies)
    budget = rng_budget(circ.sh)
    n, u = circ.n, circ.u
    d_adv0 = [ctx.to_device(np.ascontiguousarray(c)) for c in circ.advice0()]
    d_vals = ctx.to_device(fr(circ.values))
    seen = {}
    try:
        want = PL.create_proof(gpk, circ.advice0(), [], PreDrawnRng(budget, 1000 + seed), phase_witness=circ.witness)
        challenges = circ.gamma_seen[-1][1]
        gamma = challenges[0]

        def on_device(phase, ch, ptrs):
            assert phase == 1 and len(ptrs) == 3 and ch[0] == gamma
            PL.rlc_fill_chains(ctx, ptrs[2:], u, d_vals, circ.pieces, ch[0], num_values=len(circ.values))
            # (the pieces name their columns by advice index: 0 is the phase-0 column, which no piece writes and every piece reads)
            PL.gate_fill_chains(ctx, [d_adv0[0]] + ptrs[:2], u, ptrs[2], u, d_adv0[0], u, circ.gate_pieces)
            ctx.sync()
            seen["columns"] = [ctx.download(p, (n, 4)) for p in ptrs[:2]]

        got = PL.create_proof(gpk, d_adv0, [], PreDrawnRng(budget, 1000 + seed), advice_on_device=True, phase_witness_dev=on_device)
        host_cols = [circ._column(v) for v in circ.select_columns(gamma)]
        for c in range(2):
            assert np.array_equal(seen["columns"][c][:u], host_cols[c][:u]), "phase-1 gate column %d differs from the definition's" % c
        assert got == want, "the proof with device-filled phase 1 differs from the one with phase 1 computed in Python integers"
        assert PL.verify_proof(gpk, [], got), "h2hip_plonk_verify_proof_rlc rejects the proof"
        assert RC.oracle_verify(srs_params, vk_from_gpu(circ.sh, gpk), [], got), "the test verifier rejects the proof"
        total, fails = PL.check_witness(gpk, circ.all_advice(challenges), [], challenges=challenges)
        assert total == 0, fails
        last = [_ints(seen["columns"][col - 1][row:row + 1])[0] for (col, row) in circ.last_cells]
        assert last == circ.selected(gamma), "a chain's last cell is not r[len - 1]"
        # a witness with one bit moved is caught: the selection really hangs on the phase-0 bits and the gates
        bad = circ.all_advice(challenges)
        bad[1][circ.gate_pieces[1][1] + 3, 0] ^= np.uint64(1)          # the first s cell of the second chain
        assert PL.check_witness(gpk, bad, [], challenges=challenges)[0] >= 1
    finally:
        for p in d_adv0 + [d_vals]:
            ctx.free(p)
        gpk.free()
        kzg.free()


# ------------------------------------------------------------------------------------------------ the struct in every layer
def check_struct_layout():
    """h2hip_gate_chain: the same fields in the header, the Rust sys crate and ctypes; the flag values alike"""
    hdr = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    rs = open(os.path.join(ROOT, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    body = re.search(r"typedef struct h2hip_gate_chain\s*\{(.*?)\}\s*h2hip_gate_chain\s*;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    cmap = {"uint32_t": "u32", "uint64_t": "u64"}
    c_fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            c_fields += [(nm.strip(), cmap[ty]) for nm in names.split(",")]
    rs_body = re.search(r"pub struct h2hip_gate_chain\s*\{(.*?)\}", rs, flags=re.S).group(1)
    rs_fields = re.findall(r"pub ([a-z_]+): ([a-z0-9]+)", rs_body)
    py_fields = [(nm, {C.c_uint32: "u32", C.c_uint64: "u64"}[t]) for nm, t in PL.GateChainStruct._fields_]
    assert c_fields == rs_fields == py_fields, (c_fields, rs_fields, py_fields)
    assert C.sizeof(PL.GateChainStruct) == 40
    for name, v in (("CARRY", 1), ("JOIN", 2), ("START_A", 4)):
        assert re.search(r"#define H2HIP_GATE_%s %d\b" % (name, v), hdr) and "pub const H2HIP_GATE_%s: u32 = %d;" % (name, v) in rs
        assert getattr(PL, "GATE_" + name) == v
    for layer in ("halo2-lib_amd/host/halo2_proofs.hpp", "ffi/rust/h2hip-sys/src/safe.rs"):
        assert "h2hip_gate_fill_chains_dev" in open(os.path.join(ROOT, layer)).read(), layer
