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
import numpy as np

from halo2_lib_amd import plonk as PL
from halo2_lib_amd import virtual_region as VR
from tests import ec_fill_checks as K
from tests import fused_fill_harness as FH
from tests.ec_fill_checks import CURVES, PARAMS, aff_add, multiples, point
from tests.fp_mul_checks import MODULI, SECP_P, Spec
from tests.fused_fill_harness import SENTINEL, Bits, FromBits, Select, compare, own_mask, place
from tests.util import R, fr

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
    u.start, u.queue, u.gaps = len(ctx.advice), 0, []   # (no range checks: no lookup cells, no gaps)
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


def unit_def(kind, case):
    """one unit on a thread of its own -> (the Unit, its cells)"""
    return kind.unit_def(case)[:2]


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
                    ctx, _chip, _ = FH.thread()
                    u = kind.define(ctx, _chip, (table, pat))
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
                ctx, _chip, _ = FH.thread()
                u = kind.define(ctx, _chip, (p, q, s))
                assert not gates_hold(ctx) and u.end - u.start == 16 * (k + 1)
                if s[0] in (0, 1):
                    assert u.results == [x % R for x in (p if s[0] else q)]
                assert u.out_offsets == [8 * j + 7 for j in range(pt)]
    for nb in NUM_BITS + [5]:
        for (vals,) in bits_pool(nb):
            ctx, _chip, _ = FH.thread()
            u = Bits(nb).define(ctx, _chip, (vals,))
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


def check_select_fill(ctx, n, k, lb, modulus, count=5, pool=None):
    sp = Spec(n, k, lb, MODULI[modulus])
    FH.check_fill(ctx, Select(sp), select_pool(sp, modulus) if pool is None else pool, count)


def check_from_bits_fill(ctx, n, k, lb, modulus, w, count=5, pool=None):
    sp = Spec(n, k, lb, MODULI[modulus])
    FH.check_fill(ctx, FromBits(sp, w), from_bits_pool(sp, w, modulus) if pool is None else pool, count)


def check_bits_fill(ctx, nb, count=4, pool=None):
    pool = bits_pool(nb) if pool is None else pool
    if nb < 254:
        assert any(v[0][0] >= (1 << nb) for v in pool), "the pool holds a value that does not fit"
    FH.check_fill(ctx, Bits(nb), pool, count)


def check_no_results(ctx):
    """results_dev = NULL: the cells are written all the same"""
    sp = Spec(88, 3, 8, SECP_P)
    for kind, pool in ((Select(sp), select_pool(sp, "secp256k1_p")[:2]), (FromBits(sp, 2), from_bits_pool(sp, 2, "secp256k1_p")[:2]), (Bits(5), bits_pool(5)[:2])):
        FH.check_no_results(ctx, kind, pool, 12, 2)


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


def check_select_breaks(ctx, name, case, ncols):
    """the harness's check_breaks over units of one kind behind 50 plain cells: every break on the cell the case names (case "two": both
    breaks inside one unit, three columns)"""
    kind, pool = _break_kind(name)
    cells_at = break_cells(name)[case]
    if len(cells_at) == 2:
        assert ncols == 3
        targets = [(1, c) for c in cells_at]
    else:
        targets = [(1 + 2 * b, cells_at[0]) for b in range(ncols - 1)]
    filler = 50
    nunits = targets[-1][0] + 2
    ncells = kind.layout(ctx.lib)[0]
    bps = FH.break_points(filler, ncells, targets)
    usable = max(bps + [filler + nunits * ncells - sum(bps)]) + 20   # (the last column takes what lies behind the last break)
    FH.check_breaks(ctx, kind, [pool[(3 * j + 1) % len(pool)] for j in range(nunits)], targets, filler, usable, ncols)


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
        compare(ctx, d_cols + [d_buf], want + [want_buf], "chained calls on %s" % curve)
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
    table, pat = from_bits_pool(sp, w, "secp256k1_p")[2]
    vals = [v % R for v in table] + pat + [1]                                # the table, two bits, a selector
    at_bits = 4 * pt
    kind = FromBits(sp, w)
    with FH.RefusalBench(ctx, kind, vals, (0, at_bits), (0, at_bits), ncells, from_bits_segments(k, w), 4 * pt) as b:
        usable, nv, fill, refused, ok = b.usable, b.nv, b.fill, b.refused, b.ok
        b.refuse_nulls()
        refused("op 2", "unknown op", fill([ok], op=2))
        refused("window_bits 0 for op 1", "window_bits outside", fill([ok], w=0))
        refused("window_bits 9 for op 1", "window_bits outside", fill([ok], w=9))
        refused("window_bits 1 for op 0", "window_bits must be 0", fill([ok], op=SELECT, w=1))
        refused("num_limbs 2", "num_limbs < 3", fill([ok], params=FH.par(n=125, k_=2, p=(1 << 250) - 1)))
        b.refuse_params(only=("flags != 0", "limb_bits 63", "num_limbs 5", "p == 0", "p >= 2^(n k)", "lookup_bits 0"))
        b.refuse_placement()
        refused("a table past values_len", "outside values_len", fill([ok, (1, 0, nv - 4 * pt + 1, 0, at_bits)]))
        refused("the bits past values_len", "outside values_len", fill([ok, (1, 0, 0, 0, nv - 1)]))
        refused("the bits far past values_len", "outside values_len", fill([(1, 0, 0, 0, (1 << 64) - 2)]))
        refused("sel past values_len", "outside values_len", fill([(1, 0, 0, pt, nv)], op=SELECT, w=0))
        refused("Q past values_len", "outside values_len", fill([(1, 0, 0, nv - pt + 1, 0)], op=SELECT, w=0))
        b.refuse_results_len()
        b.refuse_count()
        b.refuse_overlaps()
        b.refuse_aliasing((150, 5))
        for what, prm, op, wb in (("layout: flags", FH.par(flags=2), FROM_BITS, 2), ("layout: op", kind.params, 3, 0), ("layout: window", kind.params, FROM_BITS, 0),
                                  ("layout: window of op 0", kind.params, SELECT, 2), ("layout: k", FH.par(n=125, k_=2, p=(1 << 250) - 1), SELECT, 0)):
            FH.layout_refused(what, lambda: PL.ec_select_layout(prm, op, wb, ctx.lib))
        # ---- h2hip_num_to_bits_fill_dev: the scalar is vals[nv - 1]
        nb, bcells = 5, 33
        bb = b.over(Bits(nb), (nv - 1,), (0,), bcells, nb, "bits: ")
        brefused, bfill, bok = bb.refused, bb.fill, bb.ok
        bb.refuse_nulls()
        brefused("num_bits 0", "num_bits outside", bfill([bok], nb=0))
        brefused("num_bits 255", "num_bits outside", bfill([bok], nb=255))
        bb.refuse_count()
        bb.refuse_placement()
        brefused("the value past values_len", "outside values_len", bfill([bok, (1, 0, nv)]))
        bb.refuse_results_len()
        bb.refuse_overlaps(break_copy=False)
        brefused("the value inside cells this call writes", "operand range", bfill([(1, 0, 7)], vdev=b.d_cols[1], vlen=usable))
        brefused("the results inside cells this call writes", "results overlap", bfill([(1, 0, 0)], rdev=b.d_cols[1] + 32 * 10, rlen=nb))
        brefused("the results over the value", "operand range", bfill([bok], rdev=b.d_vals + 32 * (nv - 3), rlen=nb))
        FH.layout_refused("num_to_bits_layout(0)", lambda: PL.num_to_bits_layout(0, ctx.lib))
        # count == 0 needs nothing
        ctx._chk(ctx.lib.h2hip_ec_select_fill_dev(ctx.handle, None, 0, 0, None, None, 9, 99, None, 0, None, 0, None, 0))
        ctx._chk(ctx.lib.h2hip_num_to_bits_fill_dev(ctx.handle, None, 0, 0, None, None, 0, None, 0, 0, None, 0))
        # the largest run that still fits (its last cell on row usable - 1) with a table that ends where the bits begin and bits that end one
        # before values_len; a unit that ends on its break point; a selection whose sel is the last value; a scalar that is the last value
        units = [(0, usable - ncells, 0, (1 << 64) - 1, at_bits), (1, 30, 0, 7, at_bits)]
        bps = [usable - 1, 30 + ncells - 1]
        fill(units, bps=bps, rlen=2 * pt)()
        one = [(2, 3, 0, pt, nv - 1)]
        fill(one, op=SELECT, w=0, rdev=b.d_res + 32 * 2 * pt, rlen=pt)()
        bit = [(2, 3 + 16 * (k + 1), nv - 1)]
        bfill(bit, rdev=b.d_res + 32 * 3 * pt, rlen=nb)()
        ctx.sync()
        want = [np.tile(SENTINEL, (b.n_rows, 1)) for _ in range(3)]
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
        compare(ctx, b.d_cols + [b.d_res], want + [want_res], "after the refusals")


def check_names_in_every_layer():
    """the two constants, the four symbols and the two structs in the header, the Rust sys crate and ctypes"""
    FH.check_names(constants=[("H2HIP_EC_SELECT", SELECT), ("H2HIP_EC_SELECT_FROM_BITS", FROM_BITS)],
                   functions=("h2hip_ec_select_layout", "h2hip_ec_select_fill_dev", "h2hip_num_to_bits_layout", "h2hip_num_to_bits_fill_dev"),
                   structs=[("h2hip_ec_select", PL.EcSelectStruct, 32), ("h2hip_bits_unit", PL.BitsUnitStruct, 16)])


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
    nres, pt = 9 * sp.k + 3, 2 * (sp.k + 1)
    m = multiples("secp256k1_p", 7)
    table_vals = [v for q in m[:4] for v in point(sp, *q)]
    a_vals = point(sp, *m[6])
    filler = max(0, (1 << kk) - 1100)                  # plain witness cells in front of the addition: the step crosses a column break at k = 11 as at k = 10
    with FH.ProofBench(ctx, kk, nl, lb, seed, lambda builder: _msm_program(builder, sp, s, table_vals, a_vals, filler)) as pb:
        (calls, fill_at), first = pb.calls, pb.first
        ub, uf, ua, uz = (c[2] for c in calls)
        if s < 4:
            t_int = m[s]
            s_int = aff_add(SECP_P, m[6], t_int)
            assert (ua.x3, ua.y3) == s_int and uz.results == [v % R for v in (point(sp, *s_int) if s & 1 else a_vals)]
        nw = 1 + 5 * pt
        assert first[ua.start][0] < first[ua.end - 1][0], "a column break falls inside the addition"
        # one device buffer: [gate columns][the bits][T][the addition's results][Z]
        at_bits = pb.buffers(2 + pt + nres + pt, [range(nw), range(fill_at, fill_at + filler)])
        at_t, at_s, at_z = at_bits + 2, at_bits + 2 + pt, at_bits + 2 + pt + nres
        d_cols, d_gate, usable, bps, nhost = pb.d_cols, pb.d_gate, pb.sh.usable_rows, pb.bps, len(pb.host)
        PL.num_to_bits_fill(ctx, d_cols, usable, bps, d_gate, nhost, d_gate + 32 * at_bits, 2, 2, [first[calls[0][0]] + (0,)])
        PL.ec_select_fill(ctx, d_cols, usable, bps, sp.params(), FROM_BITS, 2, d_gate, nhost, d_gate + 32 * at_t, pt, [first[calls[1][0]] + (1, 0, at_bits)])
        PL.ec_fill_with_ranges(ctx, d_cols, usable, bps, pb.d_lks, sp.params(), ADD, d_gate, nhost, d_gate + 32 * at_s, nres,
                               [first[calls[2][0]] + (1 + 4 * pt, at_t)], [calls[2][1]])
        PL.ec_select_fill(ctx, d_cols, usable, bps, sp.params(), SELECT, 0, d_gate, nhost, d_gate + 32 * at_z, pt, [first[calls[3][0]] + (at_s, 1 + 4 * pt, at_bits)])
        ctx.sync()
        pb.check_columns()
        if s >= 4:
            total_f, fails = pb.check_witness(max_failures=4096)
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
        pb.check_proof(host=False, oracle=True)
