"""Point selections and scalar bits of an MSM trace filled on the device: EccChip's ec_select and ec_select_from_bits (h2hip_ec_select_fill_dev
with H2HIP_EC_SELECT / H2HIP_EC_SELECT_FROM_BITS) and GateChip::num_to_bits (h2hip_num_to_bits_fill_dev), shared by tests/test_ec_select.py
(the CPU-emulated build) and tests/test_ec_select_gpu.py: every check takes a ctx.  Every comparison is bit-exact and runs over sentinel-filled
columns and results, so untouched cells are checked too.

The definition is a Python-integer restatement over virtual_region.Context and GateChip of select::crt (bigint/select.rs:26-50), of
select_by_indicator::crt (bigint/select_by_indicator.rs:29-69) behind bits_to_indicator (flex_gate/mod.rs:609-656) and of num_to_bits
(flex_gate/mod.rs:1215-1241).

  A  the definition itself: table[sum b_i 2^i] for every boolean pattern, sel ? P : Q, the bits recompose, every gate holds for any input;
  B  the fills against the definition, the layouts and the result offsets;  C  unit counts around the workgroups (the GPU file);
  D  column breaks as assign_witnesses makes them;  E  chaining: bits -> selection -> addition -> selection with no host copy in between;
  F  the refusals;  G  a BaseConfig proof whose selections and bits the device calls write.
"""
import ctypes as C

import numpy as np

import halo2_lib_amd as H
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import virtual_region as VR
from oracle import plonk as P
from tests import ec_fill_checks as K
from tests.dyn_lookup_util import rng_budget, srs, vk_from_gpu
from tests.ec_fill_checks import CURVES, PARAMS, aff_add, multiples, point
from tests.fp_mul_checks import MODULI, SECP_P, Spec, _operand, _thread, own_mask
from tests.poseidon_trace_checks import _compare, _ints, place
from tests.rlc_checks import SENTINEL
from tests.util import PreDrawnRng, R, fr

_vp = C.c_void_p
ERR_INVALID = -1
SELECT, FROM_BITS, ADD = PL.EC_SELECT, PL.EC_SELECT_FROM_BITS, PL.EC_ADD_UNEQUAL
SOLVE_BLOCK, PLACE_BLOCK, BITS_BLOCK = 64, 256, 256   # ec_select.hip: lanes per workgroup of the per-unit, the per-(unit, segment) and the per-(unit, bit) kernel
PIECE = 2                                              # ec_select.cuh: entries of a chain per lane of the placing kernel
WINDOWS = {3: [1, 2, 4], 4: [2, 3]}                    # (k, w): both native branches on both sides of m = k
CELLS = {(3, 1): 60, (3, 2): 112, (3, 4): 424, (4, 2): 150, (4, 3): 272}
NUM_BITS = [1, 2, 64, 253, 254]


def from_bits_cells(k, w):
    m = 1 << w
    return (8 << w) - 12 + 2 * (k * (3 * m + 1) + (3 * k - 2 if m > k else 3 * m + 1))


def from_bits_segments(k, w):
    """lanes per unit of the placing kernel: the indicator's first four cells and its 2^w - 2 nodes, per coordinate the pieces of the chains
    (and of the native's chain where m <= k) and evaluate_native where m > k"""
    m = 1 << w
    pieces = -(-m // PIECE)
    return m - 1 + 2 * ((k if m > k else k + 1) * pieces + (1 if m > k else 0))


def edge_count(slots, edge, block=PLACE_BLOCK):
    """the unit count whose lanes (count times the unit's lanes) end `edge` lanes past a workgroup edge, past the first workgroup (slots odd)"""
    count = edge * pow(slots, -1, block) % block or block
    if count * slots <= block:
        count += block
    assert (count * slots - edge) % block == 0 and count * slots > block
    return count


# ------------------------------------------------------------------------------------------------ the definition
class Unit:
    pass


def _begin(ctx):
    u = Unit()
    u.start = len(ctx.advice)
    return u


def _end(ctx, u, out, offsets):
    """out: the result cells; offsets: where they lie in the thread (a witness-generation thread hands out no cell)"""
    u.end = len(ctx.advice)
    u.out_cells = out
    u.results = [c.value for c in out]
    u.out_offsets = [o - u.start for o in offsets]
    assert all(ctx.advice[o] == c.value for o, c in zip(offsets, out))
    return u


def _with_offsets(ctx, make, items):
    """[make(item)] and the thread offset of each one's last cell, the cell a gate function returns"""
    out, offsets = [], []
    for item in items:
        out.append(make(item))
        offsets.append(len(ctx.advice) - 1)
    return out, offsets


def ec_select(ctx, sp, pt, qt, sel):
    """ec_select(P, Q, sel) (ecc/mod.rs:402-415) of points given as 2 (k + 1) cells: select::crt on x, then on y (gate.select per limb, then
    on the natives)"""
    u = _begin(ctx)
    return _end(ctx, u, *_with_offsets(ctx, lambda ab: VR.GateChip.select(ctx, ab[0], ab[1], sel), list(zip(pt, qt))))


def select_by_indicator_crt(ctx, sp, crts, ind):
    """select_by_indicator::crt over CRT values given as k + 1 cells each -> (the k + 1 cells of the selected one, their thread offsets)"""
    k = sp.k
    limbs, offsets = _with_offsets(ctx, lambda j: VR.GateChip.select_by_indicator(ctx, [a[j] for a in crts], ind), range(k))
    if len(crts) > k:
        native = VR.RangeChip._inner_product_from_one(ctx, limbs, [VR.Constant(c) for c in sp.limb_bases])     # evaluate_native
    else:
        native = VR.GateChip.select_by_indicator(ctx, [a[k] for a in crts], ind)
    return limbs + [native], offsets + [len(ctx.advice) - 1]


def ec_select_from_bits(ctx, sp, table, bits):
    """ec_select_from_bits(points, sel) (ecc/mod.rs:442-456): bits_to_indicator, then ec_select_by_indicator; table: 2^len(bits) points of
    2 (k + 1) cells"""
    assert len(table) == 1 << len(bits)
    k = sp.k
    u = _begin(ctx)
    ind = VR.GateChip.bits_to_indicator(ctx, bits)
    x, x_at = select_by_indicator_crt(ctx, sp, [pt[:k + 1] for pt in table], ind)
    y, y_at = select_by_indicator_crt(ctx, sp, [pt[k + 1:] for pt in table], ind)
    return _end(ctx, u, x + y, x_at + y_at)


def num_to_bits(ctx, a, nb):
    u = _begin(ctx)
    bits = VR.GateChip.num_to_bits(ctx, a, nb)
    _end(ctx, u, bits, [u.start] + [u.start + 1 + 3 * (i - 1) for i in range(1, nb)])
    u.sum_offset = 3 * nb - 3
    return u


def gates_hold(ctx, cells=None):
    cells = ctx.advice if cells is None else cells
    return [s for s, q in enumerate(ctx.selector) if q and (cells[s] + cells[s + 1] * cells[s + 2] - cells[s + 3]) % R]


class Select:
    """what the checks need to know of a kind of unit.  A case is the unit's operand values: (P's 2 (k + 1), Q's, [sel])"""

    def __init__(self, sp):
        self.sp, self.nres, self.name = sp, 2 * (sp.k + 1), "select"

    def define(self, ctx, case, tag=0):
        p, q, s = case
        return ec_select(ctx, self.sp, _operand(p, 3 * tag), _operand(q, 3 * tag + 1), _operand(s, 3 * tag + 2)[0])

    def unit(self, col, row, at, case):
        """the unit whose operands lie at `at` of the values, in the case's order"""
        return (col, row, at, at + len(case[0]), at + len(case[0]) + len(case[1]))

    def layout(self, lib=None):
        return PL.ec_select_layout(self.sp.params(), SELECT, 0, lib)

    def fill(self, ctx, cols, usable, bps, d_vals, nvals, d_res, nres, units):
        PL.ec_select_fill(ctx, cols, usable, bps, self.sp.params(), SELECT, 0, d_vals, nvals, d_res, nres, units)


class FromBits:
    """... (the table's m points flat, the w bits)"""

    def __init__(self, sp, w):
        self.sp, self.w, self.nres, self.name = sp, w, 2 * (sp.k + 1), "from_bits w = %d" % w

    def define(self, ctx, case, tag=0):
        table, bits = case
        pt = self.nres
        cells = _operand(table, 2 * tag)
        return ec_select_from_bits(ctx, self.sp, [cells[j * pt:(j + 1) * pt] for j in range(1 << self.w)], _operand(bits, 2 * tag + 1))

    def unit(self, col, row, at, case):
        return (col, row, at, 0, at + len(case[0]))

    def layout(self, lib=None):
        return PL.ec_select_layout(self.sp.params(), FROM_BITS, self.w, lib)

    def fill(self, ctx, cols, usable, bps, d_vals, nvals, d_res, nres, units):
        PL.ec_select_fill(ctx, cols, usable, bps, self.sp.params(), FROM_BITS, self.w, d_vals, nvals, d_res, nres, units)


class Bits:
    """... ([the value],)"""

    def __init__(self, nb):
        self.nb, self.nres, self.name = nb, nb, "num_to_bits %d" % nb

    def define(self, ctx, case, tag=0):
        return num_to_bits(ctx, _operand(case[0], tag)[0], self.nb)

    def unit(self, col, row, at, case):
        return (col, row, at)

    def layout(self, lib=None):
        return PL.num_to_bits_layout(self.nb, lib)

    def fill(self, ctx, cols, usable, bps, d_vals, nvals, d_res, nres, units):
        PL.num_to_bits_fill(ctx, cols, usable, bps, d_vals, nvals, d_res, nres, self.nb, units)


def unit_def(kind, case):
    """one unit on a thread of its own -> (the Unit, its cells)"""
    ctx, _chip, _ = _thread()
    u = kind.define(ctx, case)
    return u, list(ctx.advice)


# ------------------------------------------------------------------------------------------------ the pools
def _rng(*key):
    return np.random.default_rng([0x5E1] + [int(x) % (1 << 32) for x in key])


def _rand_point(sp, g):
    return point(sp, *(int.from_bytes(g.bytes(40), "little") % sp.p for _ in range(2)))


def edge_point(sp, j):
    """a point whose limb and native cells include 0, r - 1 and 2^n (no limbs: the fills compute over the cell values themselves)"""
    k = sp.k
    pt = point(sp, sp.p - 1 - j, 5 + j)
    pt[j % k] = (0, R - 1, 1 << sp.n)[j % 3]
    pt[k] = (R - 1, 0, 1 << sp.n)[j % 3]
    pt[k + 1 + (j + 1) % k] = (1 << sp.n, 0, R - 1)[j % 3]
    pt[2 * k + 1] = (0, 1 << sp.n, R - 1)[j % 3]
    return pt


def select_pool(sp, modulus):
    """(P, Q, [sel]) for sel in 0, 1, 2, r - 1 over random points, edge points, P = Q, and curve points where the modulus has a curve"""
    g = _rng(1, sp.n, sp.k, sp.p)
    pts = [_rand_point(sp, g) for _ in range(3)] + [edge_point(sp, j) for j in range(3)]
    if modulus in CURVES:
        pts += [point(sp, *m) for m in multiples(modulus, 2)]
    pairs = [(pts[j], pts[(j + 1) % len(pts)]) for j in range(len(pts))] + [(pts[3], pts[3])]
    return [(p, q, [sel]) for j, (p, q) in enumerate(pairs) for sel in ((0, 1, 2, R - 1) if j < 4 else ((0, 1)[j % 2], (2, R - 1)[j % 2]))]


def table_of(sp, w, modulus, which):
    """a table of 2^w points: random ones with edge points among them (which = 0), or curve multiples / other random ones (which = 1)"""
    m = 1 << w
    g = _rng(2, sp.n, sp.k, sp.p, w, which)
    if which and modulus in CURVES:
        return [v for mult in multiples(modulus, m) for v in point(sp, *mult)]
    pts = [_rand_point(sp, g) for _ in range(m)]
    if not which:
        for j in range(min(3, m)):
            pts[(2 * j + 1) % m] = edge_point(sp, j)
    return [v for pt in pts for v in pt]


def bit_patterns(w):
    """every boolean pattern (16 of them at w = 4), then patterns with bits that are none: 2 and r - 1 in every position"""
    pats = [[(v >> i) & 1 for i in range(w)] for v in range(1 << w)]
    for i in range(w):
        for bad in (2, R - 1):
            pat = [(i + j) % 2 for j in range(w)]
            pat[i] = bad
            pats.append(pat)
    pats.append([2] * w)
    pats.append([R - 1] + [2] * (w - 1))
    return pats


def from_bits_pool(sp, w, modulus):
    return [(table_of(sp, w, modulus, j % 2), pat) for j, pat in enumerate(bit_patterns(w))]


def bits_values(nb):
    """0, 1, 2^nb - 1 (mod r at nb = 254), r - 1, 2^nb where it is below r, a random value of nb bits"""
    g = _rng(3, nb)
    vals = [0, 1, ((1 << nb) - 1) % R, R - 1, int.from_bytes(g.bytes(32), "little") % min(1 << nb, R)]
    if (1 << nb) < R:
        vals.append(1 << nb)
    return vals


def bits_pool(nb):
    return [([v],) for v in bits_values(nb)]


# ------------------------------------------------------------------------------------------------ A: the definition itself
def check_definition():
    """the selected point is table[sum b_i 2^i] for every boolean pattern at w = 1 .. 4 and both k; sel ? P : Q for sel in {0, 1}; the bits
    of num_to_bits recompose to the value (and only to its low bits where it does not fit); every gate of every run holds, for bits, selectors
    and limbs that are none too; is cell for cell what select / select_by_indicator mean; the cell counts are the formulas'"""
    for n, k, lb in (PARAMS[0], PARAMS[-1]):
        for modulus in ("secp256k1_p", "bn254_q"):
            sp = Spec(n, k, lb, MODULI[modulus])
            pt = 2 * (k + 1)
            for w in range(1, 5):
                m = 1 << w
                kind = FromBits(sp, w)
                for table, pat in from_bits_pool(sp, w, modulus):
                    ctx, _chip, _ = _thread()
                    u = kind.define(ctx, (table, pat))
                    assert not gates_hold(ctx), (n, k, w, pat)
                    assert u.end - u.start == from_bits_cells(k, w) and ((k, w) not in CELLS or CELLS[(k, w)] == u.end - u.start)
                    if all(b in (0, 1) for b in pat):
                        v = sum(b << i for i, b in enumerate(pat))
                        want = [x % R for x in table[v * pt:(v + 1) * pt]]
                        if m > k:                                             # evaluate_native recomputes the native from the limbs
                            for c in range(2):
                                want[c * (k + 1) + k] = sum(x * b for x, b in zip(want[c * (k + 1):c * (k + 1) + k], sp.limb_bases)) % R
                        assert u.results == want, (n, k, w, pat)
                    # the copies: every Existing cell holds its source's value
                    assert all(ctx.advice[x.offset] == ctx.advice[y.offset] for x, y in ctx.copy_manager.advice_equalities if x.type_id == y.type_id == "fp")
            kind = Select(sp)
            for p, q, s in select_pool(sp, modulus):
                ctx, _chip, _ = _thread()
                u = kind.define(ctx, (p, q, s))
                assert not gates_hold(ctx) and u.end - u.start == 16 * (k + 1)
                if s[0] in (0, 1):
                    assert u.results == [x % R for x in (p if s[0] else q)]
                assert u.out_offsets == [8 * j + 7 for j in range(pt)]
    for nb in NUM_BITS + [5]:
        for (vals,) in bits_pool(nb):
            ctx, _chip, _ = _thread()
            u = Bits(nb).define(ctx, (vals,))
            v = vals[0]
            assert not gates_hold(ctx) and u.end - u.start == 7 * nb - 2
            assert all(b in (0, 1) for b in u.results) and sum(b << i for i, b in enumerate(u.results)) == v % (1 << nb)
            assert ctx.advice[u.start + u.sum_offset] == v % (1 << nb) and u.out_offsets == [0] + [1 + 3 * (i - 1) for i in range(1, nb)]
            assert (ctx.advice[u.start + u.sum_offset] != v) == (v >= (1 << nb)), "the truncated case has sum != value"
            a_cell, acc = ctx.copy_manager.advice_equalities[0]                # constrain_equal(a, acc): the first copy of the run
            assert (a_cell.type_id, acc.offset) == ("operand", u.start + u.sum_offset)


# ------------------------------------------------------------------------------------------------ B: the fills against the definition
def check_layouts(ctx):
    """h2hip_ec_select_layout and h2hip_num_to_bits_layout give the definition's run length and result offsets; the cell counts the header names"""
    for n, k, lb in PARAMS:
        for modulus, p in MODULI.items():
            sp = Spec(n, k, lb, p)
            kind = Select(sp)
            u, cells = unit_def(kind, select_pool(sp, modulus)[0])
            assert kind.layout(ctx.lib) == (len(cells), u.out_offsets) and len(cells) == 16 * (k + 1), (n, k, lb)
            for w in range(1, 9):
                kind = FromBits(sp, w)
                lay = kind.layout(ctx.lib)
                assert lay.num_cells == from_bits_cells(k, w), (k, w)
                if (k, w) in CELLS:
                    assert lay.num_cells == CELLS[(k, w)], (k, w, lay.num_cells)
                if w <= 4:
                    u, cells = unit_def(kind, from_bits_pool(sp, w, modulus)[1])
                    assert lay == (len(cells), u.out_offsets), (n, k, lb, w, lay, u.out_offsets)
    for nb in NUM_BITS + [5]:
        u, cells = unit_def(Bits(nb), ([3],))
        assert PL.num_to_bits_layout(nb, ctx.lib) == (len(cells), u.sum_offset) == (7 * nb - 2, 3 * nb - 3)


def check_fill(ctx, kind, pool, count):
    """`count` units per call over three gate columns (no breaks), until every case of the pool was a unit: every cell of every run equals
    the definition's, every other cell keeps the sentinel, results_dev holds the definition's result cells unit by unit"""
    lay = kind.layout(ctx.lib)
    vals, at = [], []
    for case in pool:
        at.append(len(vals))
        vals += [v % R for part in case for v in part]
    nres = kind.nres
    cache = {}
    done = 0
    d_vals = ctx.to_device(fr(vals))
    try:
        while done < len(pool):
            units, defs, rows = [], [], [1, 3, 0]
            for j in range(count):
                i = (done + j) % len(pool)
                if i not in cache:
                    cache[i] = unit_def(kind, pool[i])
                u, cells = cache[i]
                assert len(cells) == lay[0]
                col = j % 3
                units.append(kind.unit(col, rows[col], at[i], pool[i]))
                defs.append((u, cells))
                rows[col] += len(cells) + (j % 2)
            done += count
            rows_n = max(rows) + 9
            want = [np.tile(SENTINEL, (rows_n, 1)) for _ in range(3)]
            want_res = np.tile(SENTINEL, (count * nres + 2, 1))
            d_cols = [ctx.to_device(c) for c in want]
            d_res = ctx.to_device(want_res)
            for j, (unit, (u, cells)) in enumerate(zip(units, defs)):
                want[unit[0]][unit[1]:unit[1] + len(cells)] = fr(cells)
                want_res[j * nres:(j + 1) * nres] = fr(u.results)
            try:
                kind.fill(ctx, d_cols, rows_n - 2, None, d_vals, len(vals), d_res, count * nres, units)
                ctx.sync()
                what = "%s, count = %d" % (kind.name, count)
                _compare(ctx, d_cols, want, what + " (gate columns)")
                _compare(ctx, [d_res], [want_res], what + " (results)")
            finally:
                for ptr in d_cols + [d_res]:
                    ctx.free(ptr)
    finally:
        ctx.free(d_vals)


def check_select_fill(ctx, n, k, lb, modulus, count=5, pool=None):
    sp = Spec(n, k, lb, MODULI[modulus])
    check_fill(ctx, Select(sp), select_pool(sp, modulus) if pool is None else pool, count)


def check_from_bits_fill(ctx, n, k, lb, modulus, w, count=5, pool=None):
    sp = Spec(n, k, lb, MODULI[modulus])
    check_fill(ctx, FromBits(sp, w), from_bits_pool(sp, w, modulus) if pool is None else pool, count)


def check_bits_fill(ctx, nb, count=4, pool=None):
    pool = bits_pool(nb) if pool is None else pool
    if nb < 254:
        assert any(v[0][0] >= (1 << nb) for v in pool), "the pool holds a value that does not fit"
    check_fill(ctx, Bits(nb), pool, count)


def check_no_results(ctx):
    """results_dev = NULL: the cells are written all the same"""
    sp = Spec(88, 3, 8, SECP_P)
    for kind, pool in ((Select(sp), select_pool(sp, "secp256k1_p")[:2]), (FromBits(sp, 2), from_bits_pool(sp, 2, "secp256k1_p")[:2]), (Bits(5), bits_pool(5)[:2])):
        vals = [v % R for case in pool for part in case for v in part]
        u0, cells0 = unit_def(kind, pool[0])
        u1, cells1 = unit_def(kind, pool[1])
        per = len(vals) // 2
        units = [kind.unit(0, 2, 0, pool[0]), kind.unit(0, 3 + len(cells0), per, pool[1])]
        rows_n = 2 * len(cells0) + 12
        want = np.tile(SENTINEL, (rows_n, 1))
        want[2:2 + len(cells0)] = fr(cells0)
        want[3 + len(cells0):3 + 2 * len(cells0)] = fr(cells1)
        d_col, d_vals = ctx.to_device(np.tile(SENTINEL, (rows_n, 1))), ctx.to_device(fr(vals))
        try:
            kind.fill(ctx, [d_col], rows_n - 2, None, d_vals, len(vals), None, 0, units)
            ctx.sync()
            _compare(ctx, [d_col], [want], kind.name + " without results")
        finally:
            ctx.free(d_col)
            ctx.free(d_vals)


# ------------------------------------------------------------------------------------------------ D: column breaks
def _break_kind(name):
    sp = Spec(88, 3, 8, SECP_P)
    if name == "select":
        return Select(sp), select_pool(sp, "secp256k1_p")
    if name == "from_bits":
        return FromBits(sp, 2), from_bits_pool(sp, 2, "secp256k1_p")
    return Bits(5), bits_pool(5)


def break_cells(name):
    """the cells of a unit each case's breaks fall on, from the definition's own offsets.  from_bits is (k, w) = (3, 2): 20 indicator cells, per
    coordinate three chains of 13 cells (two pieces of two entries each) and evaluate_native's 7"""
    kind, pool = _break_kind(name)
    u, cells = unit_def(kind, pool[0])
    n = len(cells)
    if name == "select":
        return {"first": [0], "last": [n - 1], "in_select": [8 + 4], "two": [3, 8 * 5 + 6]}
    if name == "from_bits":
        ind = 20
        assert u.out_offsets[0] == ind + 12 and u.out_offsets[3] == ind + 3 * 13 + 6
        return {"first": [0], "last": [n - 1], "in_indicator": [4 + 8 + 3], "in_chain": [ind + 13 + 5], "on_a_piece_edge": [ind + 13 + 6], "before_native": [ind + 3 * 13 - 1],
                "in_native": [ind + 3 * 13 + 3], "two": [ind + 2, ind + 46 + 13 + 9]}
    return {"first": [0], "last": [n - 1], "in_chain": [6], "in_assert_bit": [3 * 5 - 2 + 4 + 2], "two": [4, 3 * 5 - 2 + 9]}


BREAK_CASES = [(name, case) for name in ("select", "from_bits", "bits") for case in break_cells(name)]


def check_breaks(ctx, name, case, ncols):
    """one thread (plain cells, then units of one kind back to back, each reading operands of its own) laid into ncols columns by
    virtual_region.assign_witnesses and by the fill from each unit's first cell, from the same break points.  Every break falls on the cell
    the case names (case "two": both breaks inside one unit, three columns)."""
    kind, pool = _break_kind(name)
    cells_at = break_cells(name)[case]
    if len(cells_at) == 2:
        assert ncols == 3
        targets = [(1, c) for c in cells_at]
    else:
        targets = [(1 + 2 * b, cells_at[0]) for b in range(ncols - 1)]
    filler = 50
    nunits = targets[-1][0] + 2
    thread, _chip, _ = _thread()
    thread.advice += list(range(100, 100 + filler))
    thread.selector += [False] * filler
    cases = [pool[(3 * j + 1) % len(pool)] for j in range(nunits)]
    defs = [kind.define(thread, case_, j) for j, case_ in enumerate(cases)]
    ncells = defs[0].end - defs[0].start
    assert all(u.end - u.start == ncells for u in defs)
    idx = [filler + unit * ncells + c for unit, c in targets]
    bps = [idx[0]] + [b - a for a, b in zip(idx, idx[1:])]
    total = len(thread.advice)
    usable = max(bps + [total - idx[-1]]) + 20
    at = place(0, 0, total, bps, ncols)[0]
    first = {}
    for i, c, r in at:
        first.setdefault(i, (c, r))
    for i, b, col in zip(idx, bps, range(ncols)):   # the break cell is the cell the case names
        assert (i, col, b) in at and (i, col + 1, 0) in at, (name, case, i)
    vals, offs = [], []
    for case_ in cases:
        offs.append(len(vals))
        vals += [v % R for part in case_ for v in part]
    units = [kind.unit(*first[u.start], offs[j], cases[j]) for j, u in enumerate(defs)]
    rows_n = usable + 9
    region = VR.Region(rows_n, ncols)
    VR.assign_witnesses([thread], list(range(ncols)), region, bps)
    want = [np.tile(SENTINEL, (rows_n, 1)) for _ in range(ncols)]
    for c in range(ncols):
        rows = sorted(region.advice[c])
        want[c][rows] = fr([region.advice[c][r] for r in rows])
    start = [np.tile(SENTINEL, (rows_n, 1)) for _ in range(ncols)]
    start[0][:filler] = want[0][:filler]
    nres = kind.nres
    want_res = np.concatenate([fr(u.results) for u in defs] + [np.tile(SENTINEL, (1, 1))])
    d_cols = [ctx.to_device(c) for c in start]
    d_vals = ctx.to_device(fr(vals))
    d_res = ctx.to_device(np.tile(SENTINEL, (nunits * nres + 1, 1)))
    try:
        kind.fill(ctx, d_cols, usable, bps, d_vals, len(vals), d_res, nunits * nres, units)
        ctx.sync()
        what = "breaks (%s, %s, %d columns)" % (name, case, ncols)
        _compare(ctx, d_cols, want, what)
        _compare(ctx, [d_res], [want_res], what + " (results)")
    finally:
        for ptr in d_cols + [d_vals, d_res]:
            ctx.free(ptr)


# ------------------------------------------------------------------------------------------------ E: chaining
def check_chained(ctx, curve, n=88, k=3, lb=8, count=3):
    """bits = num_to_bits(s, 2); T = select_from_bits(G .. 4 G, bits), read from the first call's results; S = A + T by h2hip_ec_fill_dev, T read
    from the second call's results as Q; Z = select(S, A, bits[0]), S read from the third call's results: four calls over ONE device buffer
    with no host copy in between.  Every column and every results section equals the definition's over sentinels, and T, S, Z are table[s],
    A + T and (s odd ? S : A) in integer curve arithmetic."""
    p = CURVES[curve][0]
    sp = Spec(n, k, lb, p)
    pt, nres = 2 * (k + 1), 9 * k + 3
    m = multiples(curve, 8 + count)
    table_pts = m[:4]
    scalars = [(j + 1) % 4 for j in range(count)]
    a_pts = [m[6 + j] for j in range(count)]
    table = [v for q in table_pts for v in point(sp, *q)]
    a_vals = [point(sp, *a) for a in a_pts]
    # the buffer: [scalars][table][A_j][bits][T_j][S_j's results][Z_j]
    at_s, at_tab, at_a = 0, count, count + 4 * pt
    at_bits = at_a + count * pt
    at_t = at_bits + 2 * count
    at_s3 = at_t + count * pt
    at_z = at_s3 + count * nres
    total = at_z + count * pt
    host = np.tile(SENTINEL, (total + 1, 1))
    host[:at_bits] = fr(scalars + table + [v for a in a_vals for v in a])
    want_buf = host.copy()
    bits_k, fb_k, sel_k = Bits(2), FromBits(sp, 2), Select(sp)
    ncol = [0, 0, 0, 0]
    want = [np.zeros((0, 4), dtype=np.uint64)] * 4
    runs = [[], [], [], []]
    units = [[], [], [], []]
    rows = [2, 1, 3, 0]
    for j in range(count):
        ub, cb = unit_def(bits_k, ([scalars[j]],))
        uf, cf = unit_def(fb_k, (table, ub.results))
        ua, ca, _lk, _t = K.unit_def(sp, ADD, a_vals[j], uf.results)
        s_pt = ua.results[:pt]
        uz, cz = unit_def(sel_k, (s_pt, a_vals[j], [ub.results[0]]))
        t_int = table_pts[scalars[j]]
        s_int = aff_add(p, a_pts[j], t_int)
        assert uf.results == [v % R for v in point(sp, *t_int)] and (ua.x3, ua.y3) == s_int
        assert uz.results == [v % R for v in (point(sp, *s_int) if scalars[j] & 1 else a_vals[j])]
        for call, (u, cells, unit) in enumerate(((ub, cb, (0, rows[0], at_s + j)),
                                                 (uf, cf, (1, rows[1], at_tab, 0, at_bits + 2 * j)),
                                                 (ua, ca, (2, rows[2], at_a + j * pt, at_t + j * pt)),
                                                 (uz, cz, (3, rows[3], at_s3 + j * nres, at_a + j * pt, at_bits + 2 * j)))):
            units[call].append(unit)
            runs[call].append((rows[call], u, cells))
            rows[call] += len(cells) + 1 + j
        want_buf[at_bits + 2 * j:at_bits + 2 * j + 2] = fr(ub.results)
        want_buf[at_t + j * pt:at_t + (j + 1) * pt] = fr(uf.results)
        want_buf[at_s3 + j * nres:at_s3 + (j + 1) * nres] = fr(ua.results)
        want_buf[at_z + j * pt:at_z + (j + 1) * pt] = fr(uz.results)
    rows_n = max(rows) + 9
    want = [np.tile(SENTINEL, (rows_n, 1)) for _ in range(4)]
    for call in range(4):
        for row, u, cells in runs[call]:
            keep = own_mask(u) if call == 2 else np.ones(len(cells), dtype=bool)
            want[call][row:row + len(cells)][keep] = fr(cells)[keep]
    d_cols = [ctx.to_device(np.tile(SENTINEL, (rows_n, 1))) for _ in range(4)]
    d_buf = ctx.to_device(host)
    try:
        PL.num_to_bits_fill(ctx, d_cols, rows_n - 2, None, d_buf, total, d_buf + 32 * at_bits, 2 * count, 2, units[0])
        PL.ec_select_fill(ctx, d_cols, rows_n - 2, None, sp.params(), FROM_BITS, 2, d_buf, total, d_buf + 32 * at_t, count * pt, units[1])
        PL.ec_fill(ctx, d_cols, rows_n - 2, None, sp.params(), ADD, d_buf, total, d_buf + 32 * at_s3, count * nres, units[2])
        PL.ec_select_fill(ctx, d_cols, rows_n - 2, None, sp.params(), SELECT, 0, d_buf, total, d_buf + 32 * at_z, count * pt, units[3])
        ctx.sync()
        _compare(ctx, d_cols + [d_buf], want + [want_buf], "chained calls on %s" % curve)
    finally:
        for ptr in d_cols + [d_buf]:
            ctx.free(ptr)


# ------------------------------------------------------------------------------------------------ F: the refusals
def check_rejections(ctx):
    """one case per refusal of h2hip_ec_select_fill_dev and of h2hip_num_to_bits_fill_dev: H2HIP_ERR_INVALID, the reason in h2hip_last_error,
    the sentinel everywhere (columns and results); then count == 0 and good calls at the limits from the same context"""
    sp = Spec(88, 3, 8, SECP_P)
    k, pt, w = sp.k, 2 * (sp.k + 1), 2
    ncells = from_bits_cells(k, w)
    n_rows, usable = 2 * ncells + 60, 2 * ncells + 50
    table, pat = from_bits_pool(sp, w, "secp256k1_p")[2]
    vals = [v % R for v in table] + pat + [1]                                # the table, two bits, a selector
    nv, at_bits = len(vals), 4 * pt
    sent, sent_res = np.tile(SENTINEL, (n_rows, 1)), np.tile(SENTINEL, (4 * pt, 1))
    d_cols = [ctx.to_device(sent) for _ in range(3)]
    d_vals = ctx.to_device(fr(vals))
    d_res = ctx.to_device(sent_res)
    good = sp.params()
    ok = (0, 0, 0, 0, at_bits)
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
            for ptr in d_cols:
                assert np.array_equal(ctx.download(ptr, (n_rows, 4)), sent), "%s: a cell was written" % what
            assert np.array_equal(ctx.download(d_res, (4 * pt, 4)), sent_res), "%s: a result was written" % what

        def fill(units, cols=None, usable_rows=usable, bps=None, params=good, op=FROM_BITS, wb=w, vdev=None, vlen=nv, rdev=None, rlen=4 * pt):
            return lambda: PL.ec_select_fill(ctx, d_cols if cols is None else cols, usable_rows, bps, params, op, wb, d_vals if vdev is None else vdev, vlen,
                                             d_res if rdev is None else rdev, rlen, units)

        par = lambda n=88, k_=3, lb=8, p=SECP_P, flags=0: PL.fp_params(n, k_, lb, p, flags)
        cols = (_vp * 3)(*[_vp(int(ptr)) for ptr in d_cols])
        tab = C.cast(PL.ec_select_table([ok]), _vp)
        pp = C.cast(C.pointer(good), _vp)
        raw = lambda c, p_, v, t, cnt=1: (lambda: ctx._chk(ctx.lib.h2hip_ec_select_fill_dev(ctx.handle, c, 3, usable, None, p_, FROM_BITS, w, v, nv, _vp(int(d_res)), 4 * pt, t, cnt)))
        refused("columns NULL", "NULL argument", raw(None, pp, _vp(int(d_vals)), tab))
        refused("params NULL", "NULL argument", raw(cols, None, _vp(int(d_vals)), tab))
        refused("values NULL", "NULL argument", raw(cols, pp, None, tab))
        refused("units NULL", "NULL argument", raw(cols, pp, _vp(int(d_vals)), None))
        refused("op 2", "unknown op", fill([ok], op=2))
        refused("window_bits 0 for op 1", "window_bits outside", fill([ok], wb=0))
        refused("window_bits 9 for op 1", "window_bits outside", fill([ok], wb=9))
        refused("window_bits 1 for op 0", "window_bits must be 0", fill([ok], op=SELECT, wb=1))
        refused("num_limbs 2", "num_limbs < 3", fill([ok], params=par(n=125, k_=2, p=(1 << 250) - 1)))
        refused("flags != 0", "flags", fill([ok], params=par(flags=1)))
        refused("limb_bits 63", "limb_bits outside", fill([ok], params=par(n=63, k_=4, p=(1 << 252) - 1)))
        refused("num_limbs 5", "num_limbs outside", fill([ok], params=par(n=64, k_=5)))
        refused("p == 0", "zero", fill([ok], params=par(p=0)))
        refused("p >= 2^(n k)", "exactly num_limbs", fill([ok], params=par(p=1 << 264)))
        refused("lookup_bits 0", "lookup_bits", fill([ok], params=par(lb=0)))
        refused("column index out of range", "column index", fill([ok, (3, 0, 0, 0, at_bits)]))
        refused("a NULL column", "column index", fill([ok, (1, 0, 0, 0, at_bits)], cols=[d_cols[0], 0, d_cols[2]]))
        refused("a run that leaves the usable rows", "usable rows", fill([ok, (1, usable - ncells + 1, 0, 0, at_bits)]))
        refused("a run that leaves the last column", "last column", fill([ok, (2, usable - ncells + 1, 0, 0, at_bits)], bps=[usable - 1, usable - 1]))
        refused("a break point >= usable_rows", "break point", fill([ok], bps=[10, usable]))
        refused("a table past values_len", "outside values_len", fill([ok, (1, 0, nv - 4 * pt + 1, 0, at_bits)]))
        refused("the bits past values_len", "outside values_len", fill([ok, (1, 0, 0, 0, nv - 1)]))
        refused("the bits far past values_len", "outside values_len", fill([(1, 0, 0, 0, (1 << 64) - 2)]))
        refused("sel past values_len", "outside values_len", fill([(1, 0, 0, pt, nv)], op=SELECT, wb=0))
        refused("Q past values_len", "outside values_len", fill([(1, 0, 0, nv - pt + 1, 0)], op=SELECT, wb=0))
        refused("results_len too small", "results_len", fill([ok, (1, 0, 0, 0, at_bits)], rlen=2 * pt - 1))
        refused("count times the segments > 2^32", "2^32", raw(cols, pp, _vp(int(d_vals)), tab, cnt=(1 << 32) // from_bits_segments(k, w) + 1))
        refused("two units' cells overlap", "cells overlap", fill([ok, (0, ncells - 1, 0, 0, at_bits)]))
        refused("a break copy inside another unit", "cells overlap", fill([(1, 0, 0, 0, at_bits), (0, 20, 0, 0, at_bits)], bps=[25, usable - 1]))
        refused("the bits inside cells this call writes", "operand range", fill([(1, 0, 150, 0, 5)], vdev=d_cols[1], vlen=usable))
        refused("the results inside cells this call writes", "results overlap", fill([(1, 0, 0, 0, at_bits)], rdev=d_cols[1] + 32 * 10, rlen=pt))
        refused("the results over operands of the call", "operand range", fill([ok], rdev=d_vals, rlen=nv))
        for what, prm, op, wb in (("layout: flags", par(flags=2), FROM_BITS, 2), ("layout: op", good, 3, 0), ("layout: window", good, FROM_BITS, 0),
                                  ("layout: window of op 0", good, SELECT, 2), ("layout: k", par(n=125, k_=2, p=(1 << 250) - 1), SELECT, 0)):
            try:
                PL.ec_select_layout(prm, op, wb, ctx.lib)
            except H.H2HipError as e:
                assert e.code == ERR_INVALID, what
            else:
                raise AssertionError(what + " was accepted")
        # ---- h2hip_num_to_bits_fill_dev: the scalar is vals[nv - 1]
        nb, bcells = 5, 33
        bok = (0, 0, nv - 1)

        def bfill(units, cols=None, usable_rows=usable, bps=None, vdev=None, vlen=nv, rdev=None, rlen=4 * pt, num_bits=nb):
            return lambda: PL.num_to_bits_fill(ctx, d_cols if cols is None else cols, usable_rows, bps, d_vals if vdev is None else vdev, vlen,
                                               d_res if rdev is None else rdev, rlen, num_bits, units)

        btab = C.cast(PL.bits_unit_table([bok]), _vp)
        braw = lambda c, v, t, cnt=1, num_bits=nb: (lambda: ctx._chk(ctx.lib.h2hip_num_to_bits_fill_dev(ctx.handle, c, 3, usable, None, v, nv, _vp(int(d_res)), 4 * pt, num_bits, t, cnt)))
        refused("bits: columns NULL", "NULL argument", braw(None, _vp(int(d_vals)), btab))
        refused("bits: values NULL", "NULL argument", braw(cols, None, btab))
        refused("bits: units NULL", "NULL argument", braw(cols, _vp(int(d_vals)), None))
        refused("bits: num_bits 0", "num_bits outside", bfill([bok], num_bits=0))
        refused("bits: num_bits 255", "num_bits outside", bfill([bok], num_bits=255))
        refused("bits: count times num_bits > 2^32", "2^32", braw(cols, _vp(int(d_vals)), btab, cnt=(1 << 32) // nb + 1))
        refused("bits: column index out of range", "column index", bfill([bok, (3, 0, 0)]))
        refused("bits: a NULL column", "column index", bfill([bok, (1, 0, 0)], cols=[d_cols[0], 0, d_cols[2]]))
        refused("bits: a run that leaves the usable rows", "usable rows", bfill([bok, (1, usable - bcells + 1, 0)]))
        refused("bits: a run that leaves the last column", "last column", bfill([bok, (2, usable - bcells + 1, 0)], bps=[usable - 1, usable - 1]))
        refused("bits: a break point >= usable_rows", "break point", bfill([bok], bps=[10, usable]))
        refused("bits: the value past values_len", "outside values_len", bfill([bok, (1, 0, nv)]))
        refused("bits: results_len too small", "results_len", bfill([bok, (1, 0, 0)], rlen=2 * nb - 1))
        refused("bits: two units' cells overlap", "cells overlap", bfill([bok, (0, bcells - 1, 0)]))
        refused("bits: the value inside cells this call writes", "operand range", bfill([(1, 0, 7)], vdev=d_cols[1], vlen=usable))
        refused("bits: the results inside cells this call writes", "results overlap", bfill([(1, 0, 0)], rdev=d_cols[1] + 32 * 10, rlen=nb))
        refused("bits: the results over the value", "operand range", bfill([bok], rdev=d_vals + 32 * (nv - 3), rlen=nb))
        try:
            PL.num_to_bits_layout(0, ctx.lib)
        except H.H2HipError as e:
            assert e.code == ERR_INVALID
        else:
            raise AssertionError("num_to_bits_layout(0) was accepted")
        # count == 0 needs nothing
        ctx._chk(ctx.lib.h2hip_ec_select_fill_dev(ctx.handle, None, 0, 0, None, None, 9, 99, None, 0, None, 0, None, 0))
        ctx._chk(ctx.lib.h2hip_num_to_bits_fill_dev(ctx.handle, None, 0, 0, None, None, 0, None, 0, 0, None, 0))
        # the largest run that still fits (its last cell on row usable - 1) with a table that ends where the bits begin and bits that end one
        # before values_len; a unit that ends on its break point; a selection whose sel is the last value; a scalar that is the last value
        units = [(0, usable - ncells, 0, (1 << 64) - 1, at_bits), (1, 30, 0, 7, at_bits)]
        bps = [usable - 1, 30 + ncells - 1]
        fill(units, bps=bps, rlen=2 * pt)()
        one = [(2, 3, 0, pt, nv - 1)]
        fill(one, op=SELECT, wb=0, rdev=d_res + 32 * 2 * pt, rlen=pt)()
        bit = [(2, 3 + 16 * (k + 1), nv - 1)]
        bfill(bit, rdev=d_res + 32 * 3 * pt, rlen=nb)()
        ctx.sync()
        want = [np.tile(SENTINEL, (n_rows, 1)) for _ in range(3)]
        want_res = np.tile(SENTINEL, (4 * pt, 1))
        uf, cf = unit_def(FromBits(sp, w), (table, pat))
        for col, row, *_ in units:
            for i, c, r in place(col, row, len(cf), bps, 3)[0]:
                want[c][r] = fr([cf[i]])[0]
        want_res[:pt] = want_res[pt:2 * pt] = fr(uf.results)
        us, cs = unit_def(Select(sp), (vals[:pt], vals[pt:2 * pt], [vals[nv - 1]]))
        want[2][3:3 + len(cs)] = fr(cs)
        want_res[2 * pt:3 * pt] = fr(us.results)
        ub, cb = unit_def(Bits(nb), ([vals[nv - 1]],))
        want[2][bit[0][1]:bit[0][1] + len(cb)] = fr(cb)
        want_res[3 * pt:3 * pt + nb] = fr(ub.results)
        _compare(ctx, d_cols + [d_res], want + [want_res], "after the refusals")
    finally:
        for ptr in d_cols + [d_vals, d_res]:
            ctx.free(ptr)


def check_names_in_every_layer():
    """the two constants, the four symbols and the two structs in the header, the Rust sys crate and ctypes"""
    import os
    import re

    hdr = open(os.path.join(K.ROOT, "include", "h2hip.h")).read()
    rs = open(os.path.join(K.ROOT, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    for name, py in (("H2HIP_EC_SELECT", SELECT), ("H2HIP_EC_SELECT_FROM_BITS", FROM_BITS)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == py == int(re.search(r"pub const %s: u32 = (\d+);" % name, rs).group(1))
    lib = H.load_library()
    for fn in ("h2hip_ec_select_layout", "h2hip_ec_select_fill_dev", "h2hip_num_to_bits_layout", "h2hip_num_to_bits_fill_dev"):
        assert ("int %s(" % fn) in hdr and ("pub fn %s(" % fn) in rs and hasattr(lib, fn), fn
    for name, struct, size in (("h2hip_ec_select", PL.EcSelectStruct, 32), ("h2hip_bits_unit", PL.BitsUnitStruct, 16)):
        c_fields = re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1), flags=re.S))
        rs_fields = re.findall(r"pub (\w+):", re.search(r"pub struct %s \{(.*?)\}" % name, rs, re.S).group(1))
        assert c_fields == rs_fields == [f for f, _t in struct._fields_] and C.sizeof(struct) == size, (name, c_fields, rs_fields)


# ------------------------------------------------------------------------------------------------ G: inside a proof
def _msm_program(builder, sp, s, table_vals, a_vals, filler):
    """loads s, the four table points and A as witnesses (and `filler` plain witness cells in front of the addition), then bits = num_to_bits(s, 2); T = select_from_bits(table, bits); S = A + T
    (ec_add_unequal); Z = select(S, A, bits[0]): one window step of multi_scalar_multiply.  The scalar is the instance.
    -> [(thread offset of the unit's first cell, queue position, the Unit)] of the four units"""
    ctx = builder.main()
    chip = VR.RangeChip(sp.lb, builder.lookup_manager)
    pt = 2 * (sp.k + 1)
    st = ctx.load_witness(s)
    tab = [ctx.load_witness(v) for v in table_vals]
    at = [ctx.load_witness(v) for v in a_vals]
    queue = lambda: len(chip.lookup_manager.cells_to_lookup.get(ctx.tag(), []))
    out = []
    ub = num_to_bits(ctx, st, 2)
    out.append((ub.start, queue(), ub))
    uf = ec_select_from_bits(ctx, sp, [tab[j * pt:(j + 1) * pt] for j in range(4)], ub.out_cells)
    out.append((uf.start, queue(), uf))
    fill_at = len(ctx.advice)
    for i in range(filler):
        ctx.load_witness(7 + i)
    q = queue()
    ua = K.ec_op(ctx, chip, sp, ADD, at, uf.out_cells)
    out.append((ua.start, q, ua))
    uz = ec_select(ctx, sp, ua.out_cells, at, ub.out_cells[0])
    out.append((uz.start, queue(), uz))
    builder.assigned_instances = [[st]]
    return out, fill_at


def check_proof(ctx, kk, seed, nl, s=2):
    """G: a BaseConfig circuit built through the Context mirror (one window step on secp256k1 at (88, 3)); keygen from the mirror's selectors
    and copies; the device advice starts with the loaded witnesses only (plain filler cells in front of the addition among them, so that
    the step crosses a column break at k = 11 too); num_to_bits_fill, ec_select_fill (FROM_BITS), ec_fill_with_ranges and
    ec_select_fill (SELECT), each reading the results of those before, write every other gate cell and the whole lookup columns.  s < 4: the
    columns equal the Python-computed advice, the proof has the bytes of the oracle prover's over the host-synthesized trace, both verifiers
    accept it, check_witness finds nothing.  s = 5 does not fit two bits: the fill still equals the host trace, and check_witness reports the
    copy between s and the recomposed sum and nothing else."""
    lb = kk - 1
    sp = Spec(88, 3, lb, SECP_P)
    k, nres, pt = sp.k, 9 * sp.k + 3, 2 * (sp.k + 1)
    m = multiples("secp256k1_p", 7)
    table_vals = [v for q in m[:4] for v in point(sp, *q)]
    a_vals = point(sp, *m[6])
    n = 1 << kk
    filler = max(0, n - 1100)                          # plain witness cells in front of the addition: the step crosses a column break at k = 11 as at k = 10
    na = 12
    while True:                                        # the number of gate columns the layout fills (an empty one would have a disjoint selector)
        sh = P.Shape(kk, na, nl, 1, 1, lb)
        kb = VR.BaseCircuitBuilder(False)
        _msm_program(kb, sp, s, table_vals, a_vals, filler)
        advice_k, fixed, copies, instances, bps = kb.synthesize(sh)
        if len(bps) == na - 1:
            break
        na = len(bps) + 1
    assert na >= 2 and len(bps) >= 1
    pb = VR.BaseCircuitBuilder(True)
    pb.break_points = bps
    calls, fill_at = _msm_program(pb, sp, s, table_vals, a_vals, filler)
    advice, _, _, _, _ = pb.synthesize(sh)
    assert all(np.array_equal(a, b) for a, b in zip(advice, advice_k))
    ub, uf, ua, uz = (c[2] for c in calls)
    if s < 4:
        t_int = m[s]
        s_int = aff_add(SECP_P, m[6], t_int)
        assert (ua.x3, ua.y3) == s_int and uz.results == [v % R for v in (point(sp, *s_int) if s & 1 else a_vals)]
    total = sum(len(t.advice) for t in pb.threads)
    first = {}
    for i, c, r in place(0, 0, total, bps, na)[0]:
        first.setdefault(i, (c, r))
    nw = 1 + 5 * pt
    assert first[ua.start][0] < first[ua.end - 1][0], "a column break falls inside the addition"
    assert all(first[i] == (0, i) for i in list(range(nw)) + list(range(fill_at, fill_at + filler)))   # the witnesses: flat index i of the gate allocation
    kzg, srs_params = srs(ctx, kk, seed)
    gpk = PL.keygen(kzg, PL.BaseCircuitParams.new(kk, na, nl, 1, 1, lb), fixed, copies)
    budget = rng_budget(sh)
    # one device buffer: [gate columns][the bits][T][the addition's results][Z]
    at_bits = na * n
    at_t, at_s, at_z = at_bits + 2, at_bits + 2 + pt, at_bits + 2 + pt + nres
    host = np.zeros((at_z + pt, 4), dtype=np.uint64)
    host[:nw] = advice[0][:nw]
    host[fill_at:fill_at + filler] = advice[0][fill_at:fill_at + filler]
    d_gate = ctx.to_device(host)
    d_lookup = ctx.to_device(np.zeros((nl * n, 4), dtype=np.uint64))
    d_cols = [d_gate + 32 * n * c for c in range(na)]
    d_lks = [d_lookup + 32 * n * c for c in range(nl)]
    try:
        PL.num_to_bits_fill(ctx, d_cols, sh.usable_rows, bps, d_gate, len(host), d_gate + 32 * at_bits, 2, 2, [first[calls[0][0]] + (0,)])
        PL.ec_select_fill(ctx, d_cols, sh.usable_rows, bps, sp.params(), FROM_BITS, 2, d_gate, len(host), d_gate + 32 * at_t, pt,
                          [first[calls[1][0]] + (1, 0, at_bits)])
        PL.ec_fill_with_ranges(ctx, d_cols, sh.usable_rows, bps, d_lks, sp.params(), ADD, d_gate, len(host), d_gate + 32 * at_s, nres,
                               [first[calls[2][0]] + (1 + 4 * pt, at_t)], [calls[2][1]])
        PL.ec_select_fill(ctx, d_cols, sh.usable_rows, bps, sp.params(), SELECT, 0, d_gate, len(host), d_gate + 32 * at_z, pt,
                          [first[calls[3][0]] + (at_s, 1 + 4 * pt, at_bits)])
        ctx.sync()
        got_cols = np.concatenate([ctx.download(d_gate, (na, n, 4)), ctx.download(d_lookup, (nl, n, 4))])
        for c in range(na + nl):
            assert np.array_equal(got_cols[c], advice[c]), "advice column %d differs from the Python-computed advice" % c
        if s >= 4:
            total_f, fails = PL.check_witness(gpk, d_cols + d_lks, instances, max_failures=4096, advice_on_device=True)
            perm = lambda cell: (1 + cell[0], cell[1])                      # one constants column, then the gate advice
            s_cell, sum_cell = perm(first[0]), perm(first[ub.start + ub.sum_offset])
            assert total_f == len(fails) and fails, fails[:8]
            # the cycle is {the instance, s, the sum}: every failure is a copy with the sum's cell at one end and s or the instance (row 0 of
            # its column) at the other; s's own copy is among them
            for f in fails:
                ends = [(f.column, f.row), (f.peer_column, f.peer_row)]
                assert f.kind == "copy" and sum_cell in ends and all(e == sum_cell or e[1] == 0 for e in ends), fails[:8]
            assert any(s_cell in [(f.column, f.row), (f.peer_column, f.peer_row)] for f in fails), fails[:8]
            return
        got = PL.create_proof(gpk, d_cols + d_lks, instances, PreDrawnRng(budget, 2000 + seed), advice_on_device=True)
        asm = P.PermutationAssembly(sh)
        for l, r in copies:
            asm.copy(l, r)
        opk = P.keygen(srs_params, sh, fixed, asm, 2)
        oracle = P.create_proof(srs_params, opk, advice, [_ints(v) for v in instances], PreDrawnRng(budget, 2000 + seed), 2)
        assert got == oracle, "the proof differs from the oracle prover's over the host-synthesized trace"
        assert PL.verify_proof(gpk, instances, got), "h2hip_plonk_verify_proof rejects the proof"
        assert P.verify_proof(srs_params, vk_from_gpu(sh, gpk), [_ints(v) for v in instances], got), "the test verifier rejects the proof"
        total_f, fails = PL.check_witness(gpk, d_cols + d_lks, instances, advice_on_device=True)
        assert total_f == 0, fails
    finally:
        ctx.free(d_gate)
        ctx.free(d_lookup)
        gpk.free()
        kzg.free()
