"""The prefix / grand products (fr_ops.hip: three launches over tiles of 256 lanes x SCAN_J = 2048 elements), the strided batch inversion and the
pointwise kernels at the sizes at which they change behaviour (host side only; every check takes a ctx).

* Beyond 1024 tiles (more than 2^21 scanned elements in one segment) a lane of fr_prefix_prod_sums_kernel takes per = ceil(tiles / 1024) > 1 tile
  totals, the last busy lane fewer, the lanes after it none.  products_local scans sets * 2^k + 1 elements in one segment, so a k = 20 proof with
  three permutation sets (1536 tiles) and every proof from k = 21 on go that way.
* fr_batch_invert_to, out of place, copies a zero denominator (dst[i] = v); lane t owns t, t + T, ...: the zeros here sit on the first and the last
  element a lane owns, on the last element of the array and on a lane's whole run, over a workspace that holds stale non-zero values.
* grid_for caps a launch at 8 workgroups per CU (2^19 lanes on 256 CUs): at n = 2^20 + 259 every lane of a pointwise kernel takes two
  elements on 256 CUs and the first 259 lanes a third; on any device of up to 512 CUs some lanes still take more than one.

Every expected value comes from the serial C oracle (oracle.c_oracle: one loop over the elements, 0^-1 := 0), never from another entry of libh2hip,
and every comparison is equality, limb for limb, over all elements; the one closed form (num = i + 2, den = i + 1, z = i + 1) needs the oracle only to
put small integers into Montgomery form.  Where the oracle has no entry the reference is composed from CO.fr_mul / CO.fr_add over the whole array,
and Python integers are compared as well at sample_rows().  Operands are tests.util.full_range_fr patterns (edges included); unless a case plants
zeros, zero rows are replaced and the reference is asserted to hold no zero — equal zeros would prove nothing."""
import contextlib
import ctypes as C
import functools

import numpy as np

from oracle import bn254 as O
from oracle import c_oracle as CO
from tests.util import R, fr, full_range_fr

SCAN_J = 8                     # elements a lane of the tile kernel scans (fr_ops.hip)
TILE = 256 * SCAN_J            # elements per tile
SUMS_LANES = 1024              # lanes of fr_prefix_prod_sums_kernel: beyond SUMS_LANES tiles a lane takes several totals
SWEEP = 1 << 19                # lanes of a pointwise launch on 256 CUs (grid_for: 8 workgroups of 256 lanes per CU)
POINTWISE_N = (1 << 20) + 259
_vp = C.c_void_p

# (L, tiles, per) of section A1: the last length with per = 1; lane 512 takes one total, lanes 513.. none; lane 683 takes one total
LONG_LENGTHS = (TILE * 1024, TILE * 1024 + 1, 2049 * TILE + 5)
SHORT_LENGTHS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
RUN_LENGTHS = (((1 << 18) - 1, 4), (1 << 19, 8), ((1 << 21) + 5, 32))   # (n, automatic run of fr_batch_invert_to)


def raw(vals):
    """integers as the limbs themselves (no Montgomery factor)"""
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)


ONE = fr([1])
FILL = raw([0x0123456789ABCDEF | (0x2F << 240)])   # what replaces a zero row: any non-zero pattern below r


def tiles_of(length):
    return -(-length // TILE)


def per_of(length):
    return -(-tiles_of(length) // SUMS_LANES)


def _rep(scalar, rows):
    return np.ascontiguousarray(np.repeat(np.asarray(scalar, dtype=np.uint64).reshape(1, 4), rows, axis=0))


def _is_zero(a):
    return ~np.asarray(a).reshape(-1, 4).any(axis=1)


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=6)
def factors(n, seed):
    """n full-range patterns without a zero, shared (read-only) among the cases of one length"""
    a = full_range_fr(n, seed)
    a[_is_zero(a)] = FILL[0]
    return _frozen(a)


@functools.lru_cache(maxsize=4)
def operand(n, seed):
    """n full-range patterns, edge patterns (0, 1, r - 1, ...) included"""
    return _frozen(full_range_fr(n, seed))


def sample_rows(n):
    """the rows at which Python integers are compared: the first 300, the last 300, the 600 around every multiple of 2^19"""
    rows = set(range(min(300, n))) | set(range(max(0, n - 300), n))
    for m in range(SWEEP, n + 300, SWEEP):
        rows |= set(range(max(0, m - 300), min(n, m + 300)))
    return np.array(sorted(rows), dtype=np.int64)


def _ints(a, rows=None):
    a = np.asarray(a).reshape(-1, 4)
    return O.limbs_to_ints(a if rows is None else a[rows], R)


def scan_position(e):
    """(tile, lane in the tile, element in the lane) of scanned element e of a segment"""
    return e // TILE, e % TILE // SCAN_J, e % SCAN_J


def assert_scan_equal(got, want, tag, first=0):
    """row j of got / want is scanned element first + j of its segment (first = -1: row 0 is z[0], written outside the scan).  A first difference
    at element 0 of lane 0 of a tile > 0 points at the sums or the apply launch, anything else at the tile kernel."""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.nonzero((got != want).any(axis=1))[0]
    e = int(bad[0]) + first
    where = "z[0]" if e < 0 else "scanned element %d = (tile %d, lane %d, element %d)" % ((e,) + scan_position(e))
    raise AssertionError(f"{tag}: {len(bad)} of {len(want)} values differ from the oracle, the first at row {int(bad[0])}, {where}")


def assert_rows_equal(got, want, tag):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError(f"{tag}: {len(bad)} of {len(want)} rows differ from the oracle, first {bad[:8].tolist()}, "
                             f"in sweeps {sorted(set((bad // SWEEP).tolist()))[:9]} of 2^19 lanes")


def _no_zero(want, tag):
    assert not _is_zero(want).any(), f"{tag}: the reference holds a zero, so the values after it prove nothing"


def check_shapes():
    """the lengths, segment shapes and zero positions used below reach the branches they are named for (no kernel runs)"""
    def sums_lanes(length):   # (per, last busy lane, totals it takes) of fr_prefix_prod_sums_kernel
        nt, per = tiles_of(length), per_of(length)
        return per, (nt - 1) // per, nt - (nt - 1) // per * per
    assert [(tiles_of(L),) + sums_lanes(L) for L in LONG_LENGTHS] == [(1024, 1, 1023, 1), (1025, 2, 512, 1), (2050, 3, 683, 1)]
    k20 = 3 * ((1 << 20) - 6) + 1
    assert (tiles_of(k20), per_of(k20)) == (1536, 2) and (1 << 20) - 5 > SWEEP
    assert tiles_of(TILE * 1024 + 1) == 1025 and (TILE * 1024 + 1) % TILE != 0
    assert [invert_layout(n)[0] for n, _ in RUN_LENGTHS] == [r for _, r in RUN_LENGTHS]
    positions, lane = segment_zero_positions(40, 5000)
    assert len(positions) == 40 and all(5000 - TILE <= p < 5000 for p in positions)
    assert POINTWISE_N == 2 * SWEEP + 259 and POINTWISE_N > 512 * 8 * 256   # 256 CUs: two sweeps, 259 lanes a third; up to 512 CUs: more than one


# ------------------------------------------------------------------ A: scan lengths
def check_prefix_product(ctx, length, seed=11):
    a = factors(length, seed)
    want = CO.fr_grand_product(a, _rep(ONE, length))[1:]
    _no_zero(want, f"prefix product of {length}")
    assert_scan_equal(ctx.fr_prefix_product(a), want, f"fr_prefix_product({length})")


@functools.lru_cache(maxsize=2)
def grand_reference(n, seed):
    num, den = factors(n, seed), factors(n, seed + 1)
    want = CO.fr_grand_product(num, den)
    _no_zero(want, f"grand product of {n}")
    return num, den, _frozen(want)


def check_grand_product(ctx, n, seed=11):
    num, den, want = grand_reference(n, seed)
    assert_scan_equal(ctx.fr_grand_product(num, den), want, f"fr_grand_product({n})", first=-1)


def small_montgomery(lo, count):
    """lo, lo + 1, ... in Montgomery form: the integers written as limbs, times the limbs of 2^512 mod r (fe_mul divides by 2^256)"""
    v = np.zeros((count, 4), dtype=np.uint64)
    v[:, 0] = np.arange(lo, lo + count, dtype=np.uint64)
    return CO.fr_mul(v, _rep(raw([(1 << 512) % R]), count))


def check_telescoping(ctx, n):
    """num[i] = i + 2, den[i] = i + 1: z[i] = i + 1, whatever the oracle's grand product says"""
    m = small_montgomery(1, n + 1)
    spot = [0, 1, n // 2, n - 1, n]
    assert np.array_equal(m[spot], fr([i + 1 for i in spot]))   # the conversion itself, against Python integers
    assert_scan_equal(ctx.fr_grand_product(m[1:], m[:n]), m, f"telescoping grand product of {n}", first=-1)


def segment_factors(segments, seg_len, seed):
    nums = [factors(seg_len, seed + 2 * s) for s in range(segments)]
    dens = [factors(seg_len, seed + 2 * s + 1) for s in range(segments)]
    return nums, dens


def reference_products(nums, dens, chained):
    """every product from CO.fr_grand_product of its own factors; chained: times the previous product's last value"""
    out, carry = [], None
    for num, den in zip(nums, dens):
        z = CO.fr_grand_product(num, den)
        if chained and carry is not None:
            z = CO.fr_mul(z, _rep(carry, len(z)))
        carry = z[-1:].copy()
        out.append(z)
    return out


def assert_products_equal(got, want, chained, tag):
    assert len(got) == len(want)
    seg_len = len(want[0]) - 1
    for s, (g, w) in enumerate(zip(got, want)):
        # chained: ONE scan over [1, all factors], row i of set s is its element s * seg_len + i; otherwise a scan of [1, factors] per segment
        assert_scan_equal(g, w, f"{tag}, product {s} of {len(want)}", first=s * seg_len if chained else 0)


def check_grand_products(ctx, segments, seg_len, chained, seed=301):
    nums, dens = segment_factors(segments, seg_len, seed)
    want = reference_products(nums, dens, chained)
    for z in want:
        _no_zero(z, f"{segments} x {seg_len}")
    got = ctx.fr_grand_products(nums, dens, chained=chained)
    assert_products_equal(got, want, chained, f"fr_grand_products({segments} x {seg_len}, chained={chained})")


def check_empty_segments(ctx):
    empty = np.zeros((0, 4), dtype=np.uint64)
    for chained in (False, True):
        got = ctx.fr_grand_products([empty] * 3, [empty] * 3, chained=chained)
        assert len(got) == 3 and all(np.array_equal(z, ONE) for z in got), chained


def check_too_many_segments(ctx):
    """65536 segments are refused before anything is launched: the one product column handed in 65536 times keeps its contents, and the context
    goes on computing"""
    segments = 65536
    sentinel = _rep(FILL, 2)
    z, f = ctx.to_device(sentinel), ctx.to_device(factors(segments, 77))
    try:
        table = (_vp * segments)(*([_vp(z)] * segments))
        for chained in (0, 1):
            rc = ctx.lib.h2hip_fr_grand_products_dev(ctx.handle, table, _vp(f), _vp(f), segments, 1, chained)
            assert rc != 0, "65536 segments accepted"
            assert b"segments" in ctx.lib.h2hip_last_error()
        ctx.sync()
        assert np.array_equal(ctx.download(z, (2, 4)), sentinel), "a refused call wrote to the product column"
    finally:
        ctx.free(z)
        ctx.free(f)
    check_prefix_product(ctx, SHORT_LENGTHS[0])


# ------------------------------------------------------------------ B: zero factors
def invert_layout(total, run=0):
    """(elements per lane, T) of fr_batch_invert_to for `total` elements: lane t owns t, t + T, t + 2 T, ...  THIS IS THE CODE'S RULE (fr_ops.hip:
    per_lane = total >> 16 clamped to 4..32 unless fr_invert_run sets it, one lane per per_lane elements, whole workgroups of 256), restated so
    that the zeros below land on the positions the kernel treats specially; if the rule changes, so must this."""
    per = run or min(max(total >> 16, 4), 32)
    lanes = -(-total // per)
    return per, 256 * (-(-lanes // 256))


def owned(t, total, stride):
    return list(range(t, total, stride))


def segment_zero_positions(segments, seg_len, seed=5):
    """one position per segment, each in its segment's last TILE elements, such that the flat indices (over the concatenated array the inversion
    sees) cover: the first element a lane owns, the last element a lane owns, an element in between, the last element of the array, and a lane
    whose whole run is zero.  Positions come from invert_layout, i.e. from the code's own rule."""
    total = segments * seg_len
    per, stride = invert_layout(total)
    lo = max(seg_len - TILE, 0)
    allowed = lambda g: g % seg_len >= lo
    pos = {}
    # a lane with a full run, every element of it in the allowed window of a different segment
    lane = next(t for t in range(stride) if len(owned(t, total, stride)) == per and all(allowed(g) for g in owned(t, total, stride))
                and len({g // seg_len for g in owned(t, total, stride)}) == per)
    for g in owned(lane, total, stride):
        pos[g // seg_len] = g % seg_len
    g = np.random.default_rng(seed)
    for s in range(segments):
        if s not in pos:
            pos[s] = int(g.integers(lo, seg_len))
    assert segments - 1 not in {q // seg_len for q in owned(lane, total, stride)}
    pos[segments - 1] = seg_len - 1
    flat = [s * seg_len + pos[s] for s in range(segments)]
    alone = [q for q in flat if q % stride != lane]   # zeros in lanes whose other elements are not zero
    assert any(q < stride for q in alone), "no zero on the first element of a lane"
    assert any(q + stride >= total and q != total - 1 for q in alone), "no zero on the last element of a lane"
    assert any(stride <= q < total - stride for q in alone), "no zero inside a lane's run"
    assert total - 1 in flat and all(allowed(q) for q in flat)
    return [pos[s] for s in range(segments)], lane


def _assert_zero_from(want, p, tag):
    """the reference is non-zero up to the planted zero (factor p, value p + 1 of the product) and zero from there on"""
    assert not _is_zero(want[:p + 1]).any() and _is_zero(want[p + 1:]).all(), tag


def check_zero_denominators(ctx, segments=40, seg_len=5000, seed=501):
    nums, dens = segment_factors(segments, seg_len, seed)
    check_grand_products(ctx, segments, seg_len, False, seed)   # first: the inversion's destination now holds non-zero inverses of this size
    positions, _ = segment_zero_positions(segments, seg_len)
    dens = [d.copy() for d in dens]
    for d, p in zip(dens, positions):
        d[p] = 0
    want = reference_products(nums, dens, False)
    for s, (z, p) in enumerate(zip(want, positions)):
        _assert_zero_from(z, p, f"segment {s}")
    assert_products_equal(ctx.fr_grand_products(nums, dens, chained=False), want, False, f"zero denominators, {segments} x {seg_len}")


def check_zero_numerator_long(ctx, n, at, seed=11):
    """one zero numerator at factor `at` of a single grand product of n factors (the non-zero case of the same size runs first)"""
    num, den, before = grand_reference(n, seed)
    assert n - TILE <= at < n
    assert_scan_equal(ctx.fr_grand_product(num, den), before, f"fr_grand_product({n})", first=-1)
    num = num.copy()
    num[at] = 0
    want = CO.fr_grand_product(num, den)
    _assert_zero_from(want, at, f"zero numerator at {at}")
    assert np.array_equal(want[:at + 1], before[:at + 1])
    assert_scan_equal(ctx.fr_grand_product(num, den), want, f"fr_grand_product({n}), zero numerator at {at} = element {scan_position(at)}", first=-1)


def check_zero_numerator_chained(ctx, at_scan, segments=3, seg_len=6000, seed=601):
    """a zero numerator in the last set of a chain, at scanned element at_scan of [1, all factors] (the non-zero case runs first)"""
    nums, dens = segment_factors(segments, seg_len, seed)
    check_grand_products(ctx, segments, seg_len, True, seed)
    flat = at_scan - 1
    s, p = divmod(flat, seg_len)
    assert s == segments - 1 and flat >= segments * seg_len - TILE
    nums = list(nums)
    nums[s] = nums[s].copy()
    nums[s][p] = 0
    want = reference_products(nums, dens, True)
    for z in want[:-1]:
        _no_zero(z, "the sets before the last")
    _assert_zero_from(want[-1], p, "last set")
    assert_products_equal(ctx.fr_grand_products(nums, dens, chained=True), want, True, f"zero numerator at scanned element {at_scan}")


def check_invert_in_place(ctx, n, run, seed=701):
    per, stride = invert_layout(n)
    assert per == run, (n, per, run)
    a = operand(n, seed).copy()
    a[_is_zero(a)] = FILL[0]
    g = np.random.default_rng(seed)
    a[g.random(n) < 1 / 7] = 0
    first, last, whole = 5, owned(stride // 2 + 3, n, stride)[-1], owned(stride // 3 + 1, n, stride)
    assert len(whole) >= per - 1 and last + stride >= n
    a[[first, last, n - 1] + whole] = 0
    assert_rows_equal(ctx.fr_batch_invert(a), CO.fr_batch_invert(a), f"fr_batch_invert({n}), run {run}")
    zero = np.zeros((n, 4), dtype=np.uint64)
    assert not ctx.fr_batch_invert(zero).any(), "the all-zero column"


# ------------------------------------------------------------------ C: pointwise kernels, several elements per lane
def _abc(n):
    return operand(n, 801), operand(n, 802), operand(n, 803)


def _scalars():
    """three scalars: a full-range one, r - 1 and a small one"""
    return full_range_fr(1, 811, edges=False), fr([R - 1]), fr([3])


def check_binops(ctx, n=POINTWISE_N):
    a, b, c = _abc(n)
    assert_rows_equal(ctx.fr_add(a, b), CO.fr_add(a, b), "fr_add")
    assert_rows_equal(ctx.fr_sub(a, b), CO.fr_sub(a, b), "fr_sub")
    assert_rows_equal(ctx.fr_mul(a, b), CO.fr_mul(a, b), "fr_mul")
    want = CO.fr_add(CO.fr_mul(a, b), c)
    rows = sample_rows(n)
    assert _ints(want, rows) == [(x * y + z) % R for x, y, z in zip(_ints(a, rows), _ints(b, rows), _ints(c, rows))]
    assert_rows_equal(ctx.fr_mul_add(a, b, c), want, "fr_mul_add")


def check_scaled_sums(ctx, n=POINTWISE_N):
    y, x, _ = _abc(n)
    for s in _scalars():
        for c in _scalars()[:2]:
            assert_rows_equal(ctx.fr_axpby(y, s, c, x), CO.fr_lincomb(y, s, x, c), "fr_axpby")
        assert_rows_equal(ctx.fr_axpy(y, s, x), CO.fr_axpy(y, s, x), "fr_axpy")
        assert_rows_equal(ctx.fr_scale(y, s), CO.fr_scale(y, s), "fr_scale")


@contextlib.contextmanager
def _device(ctx):
    """up(host array) uploads once; everything is freed at the end of the block"""
    made = []

    def up(host):
        made.append(ctx.to_device(host))
        return made[-1]

    try:
        yield up
    finally:
        for p in made:
            ctx.free(p)


def check_linear_combination(ctx, count, n=POINTWISE_N, seed=821):
    """sum_j c_j P_j with coefficients r - 1, 0 and 1 among random ones; 16 terms: 15 in the first launch, one in a second that re-reads out[i].
    The columns are five resident arrays taken in turn (16 separate uploads would be half a GiB)."""
    pool = [operand(n, 801 + j) for j in range(5)]
    cs = full_range_fr(count, seed, edges=False)
    cs[0], cs[1], cs[4] = fr([R - 1])[0], 0, ONE[0]
    which = [(3 * j + 1) % len(pool) for j in range(count)]
    want = None
    for j in range(count):   # the reference: one CO.fr_mul and one CO.fr_add per term, over the whole array
        term = CO.fr_mul(pool[which[j]], _rep(cs[j], n))
        want = term if want is None else CO.fr_add(want, term)
    rows = sample_rows(n)
    ci, pi = _ints(cs), [_ints(p, rows) for p in pool]
    assert _ints(want, rows) == [sum(ci[j] * pi[which[j]][i] for j in range(count)) % R for i in range(len(rows))]
    with _device(ctx) as up:
        d = [up(p) for p in pool]
        out = up(_rep(FILL, n))   # stale values: the first launch must not accumulate onto them
        table = (_vp * count)(*[_vp(d[w]) for w in which])
        ctx._chk(ctx.lib.h2hip_fr_linear_combination_dev(ctx.handle, _vp(out), table, cs.ctypes.data_as(_vp), count, n))
        assert_rows_equal(ctx.download(out, (n, 4)), want, f"fr_linear_combination, {count} terms")


def check_lookup_terms(ctx, n=POINTWISE_N):
    a, s, ap = _abc(n)
    sp = operand(n, 804)
    beta, gamma, _ = _scalars()
    term = lambda x, y: CO.fr_mul(CO.fr_add(x, _rep(beta, n)), CO.fr_add(y, _rep(gamma, n)))
    want_n, want_d = term(a, s), term(ap, sp)
    rows = sample_rows(n)
    bi, gi = _ints(beta)[0], _ints(gamma)[0]
    for w, x, y in ((want_n, a, s), (want_d, ap, sp)):
        assert _ints(w, rows) == [(u + bi) * (v + gi) % R for u, v in zip(_ints(x, rows), _ints(y, rows))]
    got_n, got_d = ctx.lookup_product_terms(a, s, ap, sp, beta, gamma)
    assert_rows_equal(got_n, want_n, "lookup_product_terms: numerators")
    assert_rows_equal(got_d, want_d, "lookup_product_terms: denominators")


def check_assigned_resolve(ctx, n=POINTWISE_N):
    num = operand(n, 801)
    den = operand(n, 802).copy()
    den[::7] = 0
    den[1::5] = ONE[0]
    want = CO.fr_mul(num, CO.fr_batch_invert(den))
    rows = sample_rows(n)
    assert _ints(want, rows) == [x * O.inv_mod(d, R) % R for x, d in zip(_ints(num, rows), _ints(den, rows))]
    assert_rows_equal(ctx.assigned_resolve(num, den), want, "assigned_resolve")
