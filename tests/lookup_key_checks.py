"""The lookup permutation (lookup.hip: A', S' of halo2's lookup argument) on FULL-WIDTH keys through every sort path (host side only; takes a
ctx).  Every other kernel-level lookup test uses keys below 2^18 with at most three full-size field elements at the end: in every comparison
the bitonic network makes there, words 1..7 of both keys are zero — a key_less that skipped a word or walked the words in the wrong order, a
compare-exchange that moved part of a key, the 256-bit binary search of lk_mark_kernel and key_eq of lk_flags_kernel all sort such input
correctly.  Here every key is a 254-bit value (unless a case says otherwise), and the sizes walk the routes between the two sorters: one LDS
tile with and without padding, several tiles with global stages, the 4096-key tile, the counting sort's 2^22 threshold, the batched route, its
48-column launches and its per-column fall-back.  The reference is always oracle.bn254.permute_expression_pair (Python integers, sorted, a
Counter); A' and S' are compared for equality, element by element.  Shared by the emulated build (CPU suite, small sizes) and the GPU suite
(proof sizes).  Every check restores the knob it touched, also when it fails."""
import numpy as np

import halo2_lib_amd as H
from oracle import bn254 as O
from tests.knob_checks import knobs
from tests.util import R, edge_fr_values, fr, full_range_fr

MONT = (1 << 256) % R            # stored limbs of the canonical value v: v * MONT mod r
_RINV = pow(1 << 256, -1, R)
R_TOP = R >> 224                 # word 7 of r: a key whose word 7 is below it is below r whatever its other words are
MIN_TILE = 1024                  # lookup.hip: LK_MIN_TILE
COUNT_MAX_BINS = 1 << 22         # lookup.hip: LK_COUNT_MAX_BINS (keys below it take the counting sort)
BATCH = 48                       # lookup.hip: LK_BATCH (columns per launch)


def padded_keys(u):
    """lookup.hip's padded_keys / lookup_padded_keys: the power of two, at least one tile, that a sort of u keys pads to"""
    n = MIN_TILE
    while n < u:
        n <<= 1
    return n


def check_padded_keys_mirror(ctx):
    """the mirror above against the library (h2hip_lookup_sorted_table_bytes = 32 bytes per padded key)"""
    for u in (1, 2, 1000, 1023, 1024, 1025, 2048, 2049, 4000, 4096, 4097, 5000, 20000, (1 << 17) - 20, (1 << 19) - 6, (1 << 20) - 7):
        assert ctx.lib.h2hip_lookup_sorted_table_bytes(u) == 32 * padded_keys(u), u


def _ints(raw):
    """(n, 4) uint64 limb patterns read as integers (NOT as Montgomery residues)"""
    b = np.ascontiguousarray(raw, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def uniform_values(n, seed, edges=False):
    """n canonical values uniform over [0, r)"""
    return _ints(full_range_fr(n, seed, edges=edges))


def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


# ------------------------------------------------------------------------------------------------------------------------ 1. key families
def _distinct_count(u):
    return max(1, (2 * u) // 3)   # about half of the distinct values occur twice in a table of u rows


def keys_uniform(d, seed):
    out = sorted(set(uniform_values(d + 8, seed)))[:d]
    assert len(out) == d
    return out


def keys_one_word(d, w, decoy, seed):
    """d distinct keys below r that agree in every 32-bit word of their canonical form except word w.  decoy: while word w ascends from key to
    key, EVERY lower word descends (so a comparator that skips word w, or ranks a lower word above it, reverses them) and every higher word
    stays constant."""
    g = np.random.default_rng([seed, w, int(decoy), 0x0E])
    base = [int(x) for x in g.integers(1 << 28, 1 << 32, size=8)]
    base[7] = int(g.integers(1, R_TOP))                      # word 7 below r's: the key is below r
    top = R_TOP if w == 7 else 1 << 32
    assert d <= top // 2
    ws = sorted(int(x) for x in g.choice(top, size=d, replace=False)) if d < (1 << 16) else \
        sorted(set(int(x) for x in g.integers(0, top, size=2 * d)))[:d]
    assert len(ws) == d
    lows = sorted(set(int(x) for x in g.integers(8, 1 << 32, size=2 * d + 8)), reverse=True)[:d]
    assert len(lows) == d
    out = []
    for i, x in enumerate(ws):
        k = list(base)
        k[w] = x
        if decoy:
            for l in range(w):
                k[l] = lows[i] - l                           # strictly descending in i, in every lower word
        v = sum(k[j] << (32 * j) for j in range(8))
        assert v < R
        out.append(v)
    assert out == sorted(out) and len(set(out)) == d
    for a, b in zip(out, out[1:]):                           # only word w (and, for a decoy, the words below it) differ
        wa, wb = words(a), words(b)
        assert wa[w] < wb[w] and wa[w + 1:] == wb[w + 1:]
        assert all(x > y for x, y in zip(wa[:w], wb[:w])) if decoy else wa[:w] == wb[:w]   # decoy: every lower word runs against the order
    return out


def keys_one_word_all(d, seed):
    """the 16 groups of keys_one_word (w = 0..7, plain and decoy) in one key set: within a group only word w decides"""
    per = max(1, d // 16)
    out = set()
    for w in range(8):
        for decoy in (False, True):
            out.update(keys_one_word(per, w, decoy, seed + 1))
    out = sorted(out)
    extra = keys_uniform(max(0, d - len(out)) + 1, seed + 2)
    return sorted(set(out + extra))[:max(d, 1)] if len(out) < d else out[:d]


def keys_stored_small(d, seed):
    """canonical, not stored, order: the keys whose STORED (Montgomery) limbs are the small integers 1 + seed .. d + seed — full-width canonical
    values in pseudo-random order.  Sorting the stored form, or routing by it (the counting sort applies to small CANONICAL keys), cannot pass."""
    out = [(i + 1 + seed) * _RINV % R for i in range(d)]
    assert all(v * MONT % R == i + 1 + seed for i, v in enumerate(out[:4]))
    return out


def stored_order_differs(keys):
    return sorted(keys, key=lambda v: v * MONT % R) != sorted(keys)


def edge_keys():
    """the edge values as CANONICAL values: the ends of the range, the neighbours of 2^32 (the first key the routing calls large), a key whose
    low word is small while a high word is set, and tests.util.edge_fr_values()"""
    e = [R - 1, 0, 1, R - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 224) + 5] + edge_fr_values()
    out = []
    for v in e:
        assert 0 <= v < R
        if v not in out:
            out.append(v)
    return out


def keys_edges(d, seed):
    """d distinct keys: the edge values first (r - 1 among them from d = 1), filled up with uniform ones"""
    e = edge_keys()[:d]
    eset = set(e)
    return e + [v for v in keys_uniform(d, seed) if v not in eset][:d - len(e)]


def pair_from_keys(keys, u, seed, shape="shuffled"):
    """(inputs, table) of u rows over the distinct values `keys` (at most u of them): the table holds every key once and, to fill its u rows,
    some of them twice (a few three times); the inputs are drawn from the table with repeats, and hold the smallest and the largest key (the
    largest sorts next to the padding).  shape: the row order of both columns — shuffled, sorted, reverse, or bitonic (up, then down)."""
    g = np.random.default_rng([seed, u, 0x7AB])
    keys = list(keys)
    assert 1 <= len(keys) <= u and len(set(keys)) == len(keys)
    table = keys + [keys[int(i)] for i in g.integers(0, len(keys), size=u - len(keys))]
    inputs = [table[int(i)] for i in g.integers(0, u, size=u)]
    inputs[int(g.integers(0, u))] = max(keys)
    if u > 1:
        p = int(g.integers(0, u))
        if inputs[p] != max(keys) or inputs.count(max(keys)) > 1:
            inputs[p] = min(keys)
    return arrange(inputs, shape, g), arrange(table, shape, g)


def arrange(vals, shape, g):
    vals = list(vals)
    if shape == "shuffled":
        return [vals[int(i)] for i in g.permutation(len(vals))]
    s = sorted(vals)
    if shape == "sorted":
        return s
    if shape == "reverse":
        return s[::-1]
    if shape == "bitonic":     # ascending, then descending
        return s[0::2] + s[1::2][::-1]
    if shape == "valley":      # descending, then ascending
        return s[0::2][::-1] + s[1::2]
    raise ValueError(shape)


# -- multiplicities
def pair_one_value(u, seed):
    """one value in all u input rows against a table that holds it once: u - 1 leftovers, every row but one repeated"""
    k = keys_uniform(u, seed)
    v = k[len(k) // 2]
    return [v] * u, arrange(k, "shuffled", np.random.default_rng(seed))


def pair_permutation(u, seed):
    """the input is a permutation of a duplicate-free table: no repeated rows, no leftovers"""
    k = keys_uniform(u, seed)
    g = np.random.default_rng(seed)
    return arrange(k, "shuffled", g), arrange(k, "shuffled", g)


def pair_three_five(u, seed):
    """a table value present three times and used by five input rows, inside a uniform pair (u >= 8)"""
    assert u >= 8
    a, s = pair_from_keys(keys_uniform(_distinct_count(u - 5), seed), u - 5, seed)
    v = (1 << 224) + 5 + seed
    assert v not in s
    g = np.random.default_rng(seed)
    a, s = a + [v] * 5, s + [v] * 3 + [max(s)] * 2
    assert a.count(v) == 5 and s.count(v) == 3
    return arrange(a, "shuffled", g), arrange(s, "shuffled", g)


def run_boundaries(u):
    """the sorted positions a long run should straddle: the tile boundaries (1024-key and 4096-key tiles) and the global stages' (N/4, N/2)"""
    n = padded_keys(u)
    return sorted(b for b in {MIN_TILE, 2 * MIN_TILE, 4096, n // 4, n // 2} if 40 <= b < u - 40)


def pair_runs(u, seed):
    """long runs of equal values that straddle every boundary of run_boundaries(u) in the SORTED order of the inputs and of the table (asserted):
    equal keys on both sides of a tile's edge and of a global stage's partner distance.  Without a boundary below u: one run in the middle."""
    bounds = run_boundaries(u) or [max(1, u // 2)]
    srt = keys_uniform(u, seed)
    half = min(37, max(1, u // 4))
    for b in bounds:
        lo, hi = max(0, b - half), min(u, b + half + 4)
        srt[lo:hi] = [srt[lo]] * (hi - lo)
    keys = sorted(set(srt))
    extra = u - len(keys)
    table, done = list(keys), 0
    for i, b in enumerate(bounds):       # the table's runs: its spare rows go to the key that then lies across the boundary
        e = extra // len(bounds) if i < len(bounds) - 1 else extra - done
        j = min(len(keys) - 1, max(0, b - e // 2 - done))
        table += [keys[j]] * e
        done += e
    assert len(table) == u
    ts = sorted(table)
    for b in bounds:
        if 1 <= b < u:
            assert srt[b - 1] == srt[b], b
            if u >= 2 * MIN_TILE:
                assert ts[b - 1] == ts[b], b
    g = np.random.default_rng(seed)
    return arrange(srt, "shuffled", g), arrange(table, "shuffled", g)


FAMILIES = ("uniform", "one_word_all", "stored_small", "edges", "one_value", "permutation", "three_five", "runs", "sorted", "reverse", "bitonic",
            "valley")
ONE_WORD = tuple(("one_word", w, decoy) for w in range(8) for decoy in (False, True))


def make_pair(family, u, seed):
    """(inputs, table) as canonical values, u rows each"""
    d = _distinct_count(u)
    if isinstance(family, tuple):
        _, w, decoy = family
        return pair_from_keys(keys_one_word(d, w, decoy, seed), u, seed)
    if family == "uniform":
        return pair_from_keys(keys_uniform(d, seed), u, seed)
    if family == "one_word_all":
        return pair_from_keys(keys_one_word_all(d, seed), u, seed)
    if family == "stored_small":
        keys = keys_stored_small(d, seed)
        assert d < 8 or stored_order_differs(keys)      # sorting the stored limbs gives another order than the canonical one
        return pair_from_keys(keys, u, seed)
    if family == "edges":
        return pair_from_keys(keys_edges(min(d, u), seed)[:u], u, seed)
    if family == "one_value":
        return pair_one_value(u, seed)
    if family == "permutation":
        return pair_permutation(u, seed)
    if family == "three_five":
        return pair_three_five(u, seed) if u >= 8 else pair_from_keys(keys_uniform(d, seed), u, seed)
    if family == "runs":
        return pair_runs(u, seed)
    if family in ("sorted", "reverse", "bitonic", "valley"):
        return pair_from_keys(keys_uniform(d, seed), u, seed, shape=family)
    raise ValueError(family)


# ------------------------------------------------------------------------------------------------------------------ running and comparing
_TAIL = 7   # rows beyond `usable`: other values, which must be ignored


def _column(limbs, seed):
    return np.concatenate([limbs, full_range_fr(_TAIL, seed)])


class _Limbs:
    """stored (Montgomery) limbs of columns over a common set of values: every distinct value is converted once"""

    def __init__(self, *cols):
        vals = sorted(set().union(*cols))
        self.index = {v: i for i, v in enumerate(vals)}
        self.limbs = fr(vals)

    def __call__(self, col):
        return np.ascontiguousarray(self.limbs[np.fromiter((self.index[v] for v in col), dtype=np.int64, count=len(col))])


class Case:
    """one (inputs, table) pair with its reference, as device-ready limbs"""

    def __init__(self, vals, table, tag):
        assert len(vals) == len(table)
        self.u, self.tag = len(vals), tag
        want_a, want_s = O.permute_expression_pair(vals, table)
        to_limbs = _Limbs(vals, table)       # (the reference's outputs hold no other value)
        self.want_a, self.want_s = to_limbs(want_a), to_limbs(want_s)
        self.a, self.s = _column(to_limbs(vals), 1), _column(to_limbs(table), 2)

    def check(self, got, how):
        got_a, got_s = got
        for name, g, w in (("A'", got_a, self.want_a), ("S'", got_s, self.want_s)):
            g = np.asarray(g).reshape(-1, 4)
            assert g.shape == w.shape, (self.tag, how, name, g.shape)
            if not np.array_equal(g, w):
                bad = np.nonzero((g != w).any(axis=1))[0]
                raise AssertionError(f"{self.tag} {how}: {name} differs from permute_expression_pair in {len(bad)} of {self.u} rows, first {bad[:8].tolist()}")

    def run(self, ctx, modes=(False, True)):
        for presort in modes:
            self.check(ctx.lookup_permute(self.a, self.s, self.u, presort_table=presort), "presorted" if presort else "plain")


def check_families(ctx, sizes, families=FAMILIES + ONE_WORD, tile_bits=(None,), seed=0):
    """every family at every size through lookup_permute and the presorted route, under every value of lookup_big_tile_bits given (None: as it
    stands).  Returns the number of (family, size) cases."""
    cases = 0
    for u in sizes:
        for fi, fam in enumerate(families):
            vals, table = make_pair(fam, u, seed + 31 * fi + u % 29)
            case = Case(vals, table, (fam, u))
            for bits in tile_bits:
                if bits is None:
                    case.run(ctx)
                else:
                    with knobs(ctx, lookup_big_tile_bits=bits):
                        case.run(ctx)
            cases += 1
    return cases


def check_edges_next_to_padding(ctx, u):
    """r - 1 as the largest key of both columns with padding behind it: it must sort below the all-ones padding keys"""
    assert padded_keys(u) != u
    vals, table = make_pair("edges", u, 3)
    assert max(vals) == R - 1 == max(table) and 0 in vals
    Case(vals, table, ("edges", u)).run(ctx)


def check_families_batch(ctx, u, families, seed=0):
    """lookup_permute_batch: one input column per family against ONE table that holds every family's keys (u rows in all)"""
    per = max(1, _distinct_count(u) // len(families))
    cols_keys = []
    for fi, fam in enumerate(families):
        if isinstance(fam, tuple):
            k = keys_one_word(per, fam[1], fam[2], seed + fi)
        elif fam == "stored_small":
            k = keys_stored_small(per, seed + fi)
        elif fam == "edges":
            k = edge_keys()[:per]
        elif fam == "one_word_all":
            k = keys_one_word_all(per, seed + fi)
        else:
            k = keys_uniform(per, seed + fi)
        cols_keys.append(k)
    allkeys = sorted(set(v for k in cols_keys for v in k))
    assert len(allkeys) <= u
    g = np.random.default_rng([seed, u, 0xBA7])
    table = allkeys + [allkeys[int(i)] for i in g.integers(0, len(allkeys), size=u - len(allkeys))]
    table = arrange(table, "shuffled", g)
    inputs = []
    for fam, k in zip(families, cols_keys):
        col = [k[int(i)] for i in g.integers(0, len(k), size=u)]
        if fam in ("sorted", "reverse", "bitonic", "valley"):
            col = arrange(col, fam, g)
        elif fam == "one_value":
            col = [k[0]] * u
        inputs.append(col)
    _run_batch(ctx, inputs, table, ("batch", u))
    return len(inputs)


def _run_batch(ctx, inputs, table, tag):
    u = len(table)
    to_limbs = _Limbs(table, *inputs)
    got = ctx.lookup_permute_batch([_column(to_limbs(c), 3 + j) for j, c in enumerate(inputs)], _column(to_limbs(table), 2), u)
    assert len(got) == len(inputs)
    for j, c in enumerate(inputs):
        wa, ws = O.permute_expression_pair(c, table)
        assert np.array_equal(got[j][0], to_limbs(wa)), tag + (j, "A'")
        assert np.array_equal(got[j][1], to_limbs(ws)), tag + (j, "S'")


# --------------------------------------------------------------------------------------------------------------------- 3. routing thresholds
# the largest key of a column decides its sorter (lookup.hip: sort_columns_keys reads max over the keys of (key < 2^32 ? key : 0xFFFFFFFF) and
# compares it with LK_COUNT_MAX_BINS = 2^22):
THRESHOLD_KEYS = (
    ((1 << 22) - 2, "counting"),   # bins = 2^22 - 1
    ((1 << 22) - 1, "counting"),   # the last counting-sort value: bins = 2^22, the largest histogram
    (1 << 22, "bitonic"),          # the first key that is not below LK_COUNT_MAX_BINS
    ((1 << 32) - 1, "bitonic"),    # the largest one-word key: reported as 0xFFFFFFFF, which is also the marker of a large key
    (1 << 32, "bitonic"),          # word 0 is ZERO, word 1 set: reported as 0xFFFFFFFF because a high word is set
    ((1 << 224) + 5, "bitonic"),   # word 0 small (5), word 7 set
)


def expected_sorter(largest_key):
    """sort_columns_keys for one column whose largest key is given"""
    small_max = largest_key if largest_key < (1 << 32) else 0xFFFFFFFF
    return "counting" if small_max < COUNT_MAX_BINS else "bitonic"


def batched_route(count, largest_key):
    """sort_columns_keys' predicate: True = one histogram per column in one launch; False = column by column"""
    small_max = largest_key if largest_key < (1 << 32) else 0xFFFFFFFF
    bins = small_max + 1
    return small_max < COUNT_MAX_BINS and count * (bins + 2) * 8 <= (1 << 30)


def check_thresholds(ctx, u, keys=THRESHOLD_KEYS, seed=0):
    """one column of small keys (below 2^12) whose largest key is set to each threshold value, in the table alone (the inputs stay small: the
    two columns of one call take different sorters) and in both"""
    g = np.random.default_rng([seed, u, 0x22])
    small = min(u, 1 << 12)
    for big, sorter in keys:
        assert expected_sorter(big) == sorter and big < R
        table = [int(i) % small for i in range(u)]
        table[int(g.integers(0, u))] = big
        assert big in table and sum(v >= small for v in table) == 1
        base = [table[int(i)] for i in g.integers(0, u, size=u)]
        base = [v if v != big else 0 for v in base]
        for in_input in (False, True):
            vals = list(base)
            if in_input:
                vals[int(g.integers(0, u))] = big
                if u > 3:
                    vals[int(g.integers(0, u))] = big      # (twice, usually: a repeated row takes a leftover)
            assert expected_sorter(max(vals)) == (sorter if in_input else "counting")
            Case(vals, table, ("threshold", big, in_input, u)).run(ctx)
    return 2 * len(keys)


def check_batch_mixed_sorters(ctx, u, seed=0):
    """one batch whose columns' largest keys are small, 2^22 - 2, 2^22 - 1, 2^22 and full-width: one large column sends the whole batch column by
    column, where each column takes its own sorter (both sorters in one call); then the same without the large columns (batched counting sort
    with 2^22 bins)"""
    g = np.random.default_rng([seed, u, 0x33])
    wide = keys_uniform(max(1, u // 8), seed + 5)
    special = [(1 << 22) - 2, (1 << 22) - 1, 1 << 22, (1 << 32) - 1, 1 << 32, (1 << 224) + 5]
    small = max(1, min(u - len(wide) - len(special), 1 << 10))
    table = arrange(list(range(small)) + special + wide + [0] * (u - small - len(special) - len(wide)), "shuffled", g)
    assert len(table) == u

    def column(largest, extra=()):
        col = [int(v) for v in g.integers(0, small, size=u)]
        for v in (largest,) + tuple(extra):
            col[int(g.integers(0, u))] = v
        col[0] = largest
        return col

    cols = [column(small - 1), column((1 << 22) - 1), column(max(wide), wide[: len(wide) // 2]), column((1 << 22) - 2), column(1 << 22),
            column(small - 1), column((1 << 224) + 5, [1 << 32, (1 << 32) - 1])]
    sorters = [expected_sorter(max(c)) for c in cols]
    assert sorters == ["counting", "counting", "bitonic", "counting", "bitonic", "counting", "bitonic"]
    assert not batched_route(len(cols), max(max(c) for c in cols))
    _run_batch(ctx, cols, table, ("mixed", u))
    counting = [c for c, s in zip(cols, sorters) if s == "counting"]
    assert batched_route(len(counting), max(max(c) for c in counting))
    _run_batch(ctx, counting, table, ("mixed, counting only", u))


def check_batch_many_columns(ctx, u, counts=(BATCH + 1, 2 * BATCH + 1), bits=6, seed=0):
    """more columns of small keys than one launch takes (48): a full launch and a ragged last one.  Every column is different."""
    g = np.random.default_rng([seed, u, 0x44])
    m = min(u, 1 << bits)
    table = list(range(m)) + [0] * (u - m)
    for count in counts:
        assert count % BATCH and count > BATCH
        cols = []
        for j in range(count):
            col = [int(v) for v in g.integers(0, 1 + (j % m), size=u)]   # column j: keys 0 .. j mod m
            cols.append(col)
        _run_batch(ctx, cols, table, ("columns", count, u))


def fallback_counts():
    """(the largest column count that still takes the batched counting sort, the smallest that does not) when one key is 2^22 - 1: derived
    from sort_columns_keys' predicate"""
    big = COUNT_MAX_BINS - 1
    over = next(c for c in range(1, BATCH + 1) if not batched_route(c, big))
    assert batched_route(over - 1, big) and over - 1 >= 1
    return over - 1, over


def check_batch_histogram_limit(ctx, u, count, seed=0):
    """`count` columns against a table that holds 2^22 - 1 once; column j uses that key iff j is even, so the largest key of the BATCH is 2^22 - 1
    and the histograms (one of 2^22 bins per column when batched) decide the route"""
    g = np.random.default_rng([seed, u, count])
    big = COUNT_MAX_BINS - 1
    small = min(u - 1, 50)
    table = arrange(list(range(small)) + [big] + [0] * (u - small - 1), "shuffled", g)
    cols = []
    for j in range(count):
        col = [int(v) for v in g.integers(0, small, size=u)]
        if j % 2 == 0:
            col[j % u] = big
        cols.append(col)
    _run_batch(ctx, cols, table, ("histogram limit", count, u))


def check_missing_value(ctx, u, seed=0):
    """a full-width input value that differs from a table value in ONE middle word (3, 4 or 5; the lowest bit, or the highest) is missing from
    the table: the call must fail with that error — alone, and as the last column of a batch whose other columns are fine"""
    vals, table = make_pair("uniform", u, seed + 9)
    tset = set(table)
    Case(vals, table, ("missing: control", u)).run(ctx)
    for word, bit in ((3, 0), (4, 31), (5, 0), (3, 31)):
        bad = list(vals)
        victim = sorted(tset)[len(tset) // 2]
        bad_v = victim ^ (1 << (32 * word + bit))
        assert bad_v < R and bad_v not in tset and [i for i in range(8) if words(bad_v)[i] != words(victim)[i]] == [word]
        bad[u // 2] = bad_v
        for presort in (False, True):
            _expect_missing(lambda: ctx.lookup_permute(_column(fr(bad), 1), _column(fr(table), 2), u, presort_table=presort), (word, bit, presort))
        _expect_missing(lambda: ctx.lookup_permute_batch([_column(fr(vals), 1), _column(fr(vals[::-1]), 3), _column(fr(bad), 4)], _column(fr(table), 2), u),
                        (word, bit, "batch"))
    Case(vals, table, ("missing: the context still works", u)).run(ctx)


def _expect_missing(call, tag):
    try:
        call()
    except H.H2HipError as e:
        assert "missing from the table" in str(e), (tag, str(e))
    else:
        raise AssertionError(f"{tag}: a value that is not in the table went unnoticed")
