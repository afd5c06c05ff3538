"""The device steps that exist only for the sharded prover (prover_ops.hip: f(X) -> f(sX), coset gather / interleave / combine, the permutation
factors of a row range) against their DEFINITIONS (host side only; takes a ctx).  Every expected value is Python big-int arithmetic
(oracle.bn254) or, at the sizes where that would take seconds, the C oracle's field operations (oracle.c_oracle.fr_mul / fr_add) — never another
entry of libh2hip; every comparison is equality, limb for limb.  The sizes walk the kernels' boundaries: the four-coefficient lane tail and the
1024-coefficient workgroup of coset_scale_kernel, its 32-column launch groups, the 256-lane workgroups of the gather / interleave / combine
kernels, all four instances of coset_combine_kernel, and the switch of perm_product_terms_run to four rows per lane at 2^16 rows.  Values come
from the whole of [0, r) with the edge limb patterns planted (tests/util.py: full_range_fr); scale factors, beta and gamma are full-width.
Output buffers start out filled with a stale pattern and end in guard rows that must survive; inputs must come back unchanged.  Shared by the
emulated build (CPU suite) and the GPU suite (the same plus one longer size each).  Every check restores the knob it touched."""
import contextlib

import numpy as np

import halo2_lib_amd as H
from halo2_lib_amd import h2hip as HH
from oracle import bn254 as O
from oracle import c_oracle as CO
from tests.knob_checks import knobs
from tests.util import R, _raw_limbs, fr, full_range_fr

STALE = 0xA5A5A5A5A5A5A5A5      # every word of an output buffer before the call
GUARD_WORD = 0x5EA15EA15EA15EA1   # every word of the rows behind a buffer's end
POISON = 0xDEADBEEFDEADBEEF     # every word of a slot of the gathered buffer that no coset owns
GUARD = 3
COSET_BATCH = 32                # prover_ops.hip: columns per launch of coset_scale_kernel
LONG_ROWS = 1 << 16             # prover_ops.hip: perm_product_terms_run takes four rows per lane from here


def ints(limbs):
    """the canonical values of stored (Montgomery) limbs"""
    return O.limbs_to_ints(np.asarray(limbs).reshape(-1, 4), R)


def _words(rows, word):
    return np.full((rows, 4), word, dtype=np.uint64)


def _rep(scalar_limbs, rows):
    return np.ascontiguousarray(np.repeat(np.asarray(scalar_limbs, dtype=np.uint64).reshape(1, 4), rows, axis=0))


class _Buf:
    """a device buffer: `host` (or `rows` stale rows) followed by GUARD guard rows"""

    def __init__(self, ctx, host=None, rows=None):
        body = _words(rows, STALE) if host is None else np.ascontiguousarray(host, dtype=np.uint64).reshape(-1, 4)
        self.ctx, self.rows = ctx, len(body)
        self.host = np.concatenate([body, _words(GUARD, GUARD_WORD)])
        self.ptr = ctx.to_device(self.host)

    def read(self):
        got = self.ctx.download(self.ptr, self.host.shape)
        assert np.array_equal(got[self.rows:], self.host[self.rows:]), "rows behind the end of a buffer were written"
        return got[:self.rows]

    def assert_unchanged(self, tag):
        assert np.array_equal(self.read(), self.host[:self.rows]), (tag, "a buffer that the call only reads, or was not given, changed")


@contextlib.contextmanager
def _device(ctx):
    """buf(host) / buf(rows=...) allocate; everything is freed at the end of the block"""
    made = []

    def buf(host=None, rows=None):
        made.append(_Buf(ctx, host, rows))
        return made[-1]

    try:
        yield buf
    finally:
        for b in made:
            ctx.free(b.ptr)


def _assert_rows_equal(got, want, tag):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError(f"{tag}: {len(bad)} of {len(want)} elements differ from the definition, first {bad[:8].tolist()}")


def full_width_values(count, seed):
    """canonical values uniform over [0, r) (two thirds of them above 2^252)"""
    return ints(full_range_fr(count, seed, edges=False))


def stored_as(pattern):
    """the canonical value whose STORED limbs are the integer `pattern`"""
    return ints(_raw_limbs([pattern]))[0]


# ------------------------------------------------------------------------------------------------------------- 1. f(X) -> f(sX)
# (n, columns): the lane tail (n = 1 .. 5: one lane with 1 .. 4 coefficients, a second lane with one), the workgroup of 1024 coefficients (1023,
# 1024, 1025: a second block of one lane), two blocks and a third (2047, 2049); 32 / 33 / 70 columns: one full launch group, one more column,
# two groups and a ragged third
SCALE_CASES = ((1, 1), (2, 3), (3, 33), (4, 32), (5, 70), (1023, 3), (1024, 1), (1025, 4), (2047, 3), (2049, 4))
SCALE_CASES_LONG = (((1 << 16) + 3, 3),)


def scale_factors():
    """(name, canonical value): 1, r - 1, the shift zeta * omega_e^c of coset 3 of a 2^12-point extended domain and its inverse, and two values
    whose stored limbs are edge patterns (r - 1 and 2^253 + 1: every limb of the multiplier's operand at its extreme)"""
    s_c = O.ZETA * pow(O.omega_for(12), 3, R) % R
    out = [("one", 1), ("minus one", R - 1), ("coset shift", s_c), ("inverse coset shift", O.inv_mod(s_c, R)), ("stored r - 1", stored_as(R - 1)),
           ("stored 2^253 + 1", stored_as((1 << 253) + 1))]
    assert all(0 < v < R for _, v in out) and np.array_equal(fr([out[4][1]]), _raw_limbs([R - 1]))
    return out


def scale_columns(n, count, seed):
    """count columns from the whole of [0, r) with the edge patterns planted; from two columns on one is all zero, from three on one is all r - 1
    (the value), from four on one is all r - 1 as a STORED pattern"""
    cols = [full_range_fr(n, seed + j) for j in range(count)]
    if count >= 2:
        cols[1] = np.zeros((n, 4), dtype=np.uint64)
    if count >= 3:
        cols[2] = _rep(fr([R - 1]), n)
    if count >= 4:
        cols[3] = _rep(_raw_limbs([R - 1]), n)
    return cols


def powers(s, n):
    """[s^t mod r, t < n] by repeated multiplication"""
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * s % R
    return out


def check_coset_scale(ctx, cases=SCALE_CASES, factors=None, seed=0):
    """out[col][t] = in[col][t] * s^t, out of place and in place, for every scale factor; one more column than the call is given must stay as it
    is.  Returns the number of calls."""
    calls = 0
    for n, count in cases:
        cols = scale_columns(n, count + 1, seed + 100 * n)
        for name, s in (factors or scale_factors()):
            pw = powers(s, n)
            pw_limbs = fr(pw)
            want = [CO.fr_mul(c, pw_limbs) for c in cols[:count]]
            if n * count <= 4096:      # the definition in big-int arithmetic alone
                for c, w in zip(cols[:count], want):
                    assert ints(w) == [v * p % R for v, p in zip(ints(c), pw)]
            for in_place in (False, True):
                tag = ("coset scale", n, count, name, "in place" if in_place else "out of place")
                with _device(ctx) as buf:
                    ins = [buf(c) for c in cols]
                    outs = ins[:count] if in_place else [buf(rows=n) for _ in range(count)]
                    ctx.fr_coset_scale_batch_dev([b.ptr for b in outs], [b.ptr for b in ins[:count]], n, fr([s]))
                    for j in range(count):
                        _assert_rows_equal(outs[j].read(), want[j], tag + (j,))
                    for b in ins[count:] if in_place else ins:
                        b.assert_unchanged(tag)
                calls += 1
    return calls


# --------------------------------------------------------------------------------------------------------- 2. gather and interleave
SMALL_NS = (1, 255, 256, 257)   # one lane; a workgroup less one lane, a whole one, and a second block of one lane


def prover_slots(ncosets, world):
    """plonk_prove.hip's table: coset c belongs to rank c % world and is that rank's (c / world)-th; every rank sends max_cosets slots.  Returns
    (slots, number of slots of the gathered buffer)"""
    max_cosets = (ncosets + world - 1) // world
    return [(c % world) * max_cosets + c // world for c in range(ncosets)], world * max_cosets


def _scrambled(g, count):
    """a permutation of range(count) that is not the identity (count > 1)"""
    while True:
        p = [int(x) for x in g.permutation(count)]
        if count == 1 or p != list(range(count)):
            return p


def gather_lists(log_c, g, repeat_counts=range(1, 17)):
    """every coset once in scrambled order; proper subsets of 1, C / 2 and C - 1 cosets; lists of 1 .. 16 indices with repeats"""
    nc = 1 << log_c
    out = [_scrambled(g, nc)]
    for count in sorted({1, nc // 2, nc - 1} - {0, nc}):
        out.append([int(x) for x in g.choice(nc, size=count, replace=False)])
    for count in repeat_counts:
        rep = [int(x) for x in g.integers(0, nc, size=count)]
        if count >= 2:
            rep[-1] = rep[0]
        out.append(rep)
    return out


def check_coset_gather(ctx, shapes, seed=0):
    """out[m * n + j] = in[(j << log_c) + cosets[m]] by numpy indexing; shapes: (log_cosets, n).  Returns the number of calls."""
    calls = 0
    for log_c, n in shapes:
        g = np.random.default_rng([seed, log_c, n, 0x6A])
        full = full_range_fr(n << log_c, seed + 7 * n + log_c)
        with _device(ctx) as buf:
            d_full = buf(full)
            counts = set()
            long = n > 4096      # a long size moves count * n elements per list: the repeats at 2 and 16 indices only
            for cosets in gather_lists(log_c, g, (2, 16) if long else range(1, 17)):
                out = buf(rows=len(cosets) * n)
                ctx.fr_coset_gather_dev(out.ptr, d_full.ptr, cosets, log_c, n)
                want = np.concatenate([full[c::1 << log_c] for c in cosets])
                _assert_rows_equal(out.read(), want, ("coset gather", log_c, n, cosets))
                counts.add(len(cosets))
                calls += 1
            assert long or counts >= set(range(1, 17))
            d_full.assert_unchanged(("coset gather", log_c, n))
    return calls


def slot_tables(log_c, g):
    """(name, slots, slots of the buffer): identity and a scrambled permutation over a packed buffer, the prover's table for world 1 .. 4"""
    nc = 1 << log_c
    out = [("identity", list(range(nc)), nc), ("scrambled", _scrambled(g, nc), nc)]
    for world in (1, 2, 3, 4):
        slots, total = prover_slots(nc, world)
        assert sorted(set(slots)) == sorted(slots) and max(slots) < total
        out.append((f"world {world}", slots, total))
    return out


def gathered_buffer(parts, slots, total, n):
    """the all-gathered buffer: coset c's n elements at slot slots[c], every slot that no coset owns poisoned"""
    b = _words(total * n, POISON)
    for c, p in enumerate(parts):
        b[slots[c] * n:(slots[c] + 1) * n] = p
    return b


def _no_poison(got, tag):
    assert not (got == np.uint64(POISON)).all(axis=1).any(), (tag, "an element of an unused slot reached the output")


def check_coset_interleave(ctx, shapes, seed=0):
    """out[(j << log_c) + c] = in[slots[c] * n + j] by numpy indexing.  Returns the number of calls."""
    calls, unused = 0, 0
    for log_c, n in shapes:
        nc = 1 << log_c
        g = np.random.default_rng([seed, log_c, n, 0x17])
        parts = [full_range_fr(n, seed + 50 * c + n) for c in range(nc)]
        for name, slots, total in slot_tables(log_c, g):
            tag = ("coset interleave", log_c, n, name)
            src = gathered_buffer(parts, slots, total, n)
            want = np.empty((n << log_c, 4), dtype=np.uint64)
            for c in range(nc):
                want[c::nc] = src[slots[c] * n:(slots[c] + 1) * n]
            unused += total - nc
            with _device(ctx) as buf:
                d_in, d_out = buf(src), buf(rows=n << log_c)
                ctx.fr_coset_interleave_dev(d_out.ptr, d_in.ptr, slots, log_c, n)
                got = d_out.read()
                _assert_rows_equal(got, want, tag)
                _no_poison(got, tag)
                d_in.assert_unchanged(tag)
            calls += 1
    assert unused > 0 or all(log_c == 0 for log_c, _ in shapes)
    return calls


def check_gather_interleave_round_trip(ctx, shapes, seed=0):
    """interleave(gather(x)) = x when coset cosets[m] is read back from slot m"""
    for log_c, n in shapes:
        nc = 1 << log_c
        cosets = _scrambled(np.random.default_rng([seed, log_c, n, 0x27]), nc)
        slots = [cosets.index(c) for c in range(nc)]
        x = full_range_fr(n << log_c, seed + 3 * n + log_c)
        with _device(ctx) as buf:
            d_x, d_g, d_back = buf(x), buf(rows=n << log_c), buf(rows=n << log_c)
            ctx.fr_coset_gather_dev(d_g.ptr, d_x.ptr, cosets, log_c, n)
            ctx.fr_coset_interleave_dev(d_back.ptr, d_g.ptr, slots, log_c, n)
            _assert_rows_equal(d_back.read(), x, ("gather / interleave round trip", log_c, n))


# --------------------------------------------------------------------------------------------------------------------- 3. combine
def coset_transforms_bigint(h, n, log_c, rho, zn):
    """P_c[t] = sum_q h[q n + t] * zn^q * rho^(c q) for every coset c: what the per-coset inverse transforms of the polynomial with the
    coefficients h (canonical values) hold when zn = zeta^n and rho = omega_e^n.  No transform is involved."""
    nc = 1 << log_c
    out = []
    for c in range(nc):
        xq = powers(zn * pow(rho, c, R) % R, nc)
        out.append([sum(h[q * n + t] * xq[q] for q in range(nc)) % R for t in range(n)])
    return out


def coset_transforms_oracle(h_limbs, n, log_c, rho, zn):
    """the same on stored limbs with the C oracle's fr_mul / fr_add (Horner's rule over q), for the sizes where the big-int form takes seconds"""
    nc = 1 << log_c
    out = []
    for c in range(nc):
        x = _rep(fr([zn * pow(rho, c, R) % R]), n)
        p = np.ascontiguousarray(h_limbs[(nc - 1) * n:nc * n])
        for q in range(nc - 2, -1, -1):
            p = CO.fr_add(CO.fr_mul(p, x), h_limbs[q * n:(q + 1) * n])
        out.append(p)
    return out


def combine_slot_tables(log_c):
    nc = 1 << log_c
    out = [("identity", list(range(nc)), nc), ("reversed", list(range(nc))[::-1], nc)]
    for world in (2, 3):
        slots, total = prover_slots(nc, world)
        out.append((f"world {world}", slots, total))
    return out


def _combine_case(ctx, h_limbs, n, log_c, zn, table, tag, oracle_form=False):
    name, slots, total = table
    rho = O.omega_for(log_c)      # a primitive C-th root of unity ...
    assert pow(rho, 1 << log_c, R) == 1 and pow(rho, 1 << (log_c - 1), R) == R - 1
    if n & (n - 1) == 0:          # ... and omega_e^n where the size-n domain exists
        assert rho == pow(O.omega_for(log_c + n.bit_length() - 1), n, R)
    assert zn % R != 0
    parts = coset_transforms_oracle(h_limbs, n, log_c, rho, zn) if oracle_form else [fr(p) for p in coset_transforms_bigint(ints(h_limbs), n, log_c, rho, zn)]
    src = gathered_buffer(parts, slots, total, n)
    with _device(ctx) as buf:
        d_in, d_out = buf(src), buf(rows=n << log_c)
        ctx.fr_coset_combine_dev(d_out.ptr, d_in.ptr, slots, log_c, n, fr([O.inv_mod(rho, R)]), fr([O.inv_mod(zn, R)]))
        got = d_out.read()
        _assert_rows_equal(got, h_limbs, tag + (name,))
        _no_poison(got, tag + (name,))
        d_in.assert_unchanged(tag + (name,))


def combine_zns(n, seed):
    """1, r - 1, zeta^n, a full-width value and one whose stored limbs are an edge pattern"""
    return [1, R - 1, pow(O.ZETA, n, R), full_width_values(1, seed)[0], stored_as(R - 2)]


def check_coset_combine(ctx, shapes, seed=0):
    """h -> its per-coset transforms P_c in big-int arithmetic -> h2hip_fr_coset_combine_dev must give h back: every slot table at every shape with
    the values of zn in rotation.  Returns the number of calls."""
    calls = 0
    for log_c, n in shapes:
        h = full_range_fr(n << log_c, seed + 11 * n + log_c)
        zns = combine_zns(n, seed + n)
        for ti, table in enumerate(combine_slot_tables(log_c)):
            zn = zns[(ti + log_c + n) % len(zns)]
            _combine_case(ctx, h, n, log_c, zn, table, ("coset combine", log_c, n, zn))
            calls += 1
    return calls


def check_coset_combine_special(ctx, n, seed=0):
    """zn = 1 and r - 1 with h identically zero, every coefficient r - 1 (as a value and as a stored pattern) and uniform, for all four instances"""
    calls = 0
    for log_c in (1, 2, 3, 4):
        rows = n << log_c
        hs = (("zero", np.zeros((rows, 4), dtype=np.uint64)), ("all r - 1", _rep(fr([R - 1]), rows)), ("all stored r - 1", _rep(_raw_limbs([R - 1]), rows)),
              ("uniform", full_range_fr(rows, seed + log_c)))
        tables = combine_slot_tables(log_c)
        for zi, zn in enumerate((1, R - 1)):
            for hi, (hname, h) in enumerate(hs):
                _combine_case(ctx, h, n, log_c, zn, tables[(zi + hi) % len(tables)], ("coset combine", log_c, n, zn, hname))
                calls += 1
    return calls


def check_coset_combine_reference_forms(n=5, log_c=2, seed=3):
    """the two forms of the reference agree (the oracle form is the one a long size uses)"""
    h = full_range_fr(n << log_c, seed)
    rho, zn = O.omega_for(log_c), full_width_values(1, seed)[0]
    a = coset_transforms_bigint(ints(h), n, log_c, rho, zn)
    b = coset_transforms_oracle(h, n, log_c, rho, zn)
    assert [ints(p) for p in b] == a


def check_coset_combine_long(ctx, log_c, n, seed=0):
    """one long size under the prover's table for world 3 (unused slots poisoned), the reference through the C oracle's field operations"""
    h = full_range_fr(n << log_c, seed + n)
    slots, total = prover_slots(1 << log_c, 3)
    assert total > 1 << log_c
    _combine_case(ctx, h, n, log_c, full_width_values(1, seed + 1)[0], ("world 3", slots, total), ("coset combine, long", log_c, n), oracle_form=True)


# ------------------------------------------------------------------------------------------- 4. permutation factors by row range
def perm_factors_bigint(cols, sigmas, chunk_len, row0, rows, beta, gamma, omega):
    """(nums, dens), one (rows, 4) limb array per set: num[i] = prod_j (col_j[i] + beta delta^j omega^i + gamma), den[i] = prod_j (col_j[i] +
    beta sigma_j[i] + gamma) over the columns j of the set (j: the column's index in the whole argument), for i in [row0, row0 + rows) — computed
    for those rows alone.  cols / sigmas: canonical values"""
    nums, dens = [], []
    w0 = pow(omega, row0, R)
    for c0 in range(0, len(cols), chunk_len):
        nu, de = [1] * rows, [1] * rows
        for j in range(c0, min(c0 + chunk_len, len(cols))):
            x = beta * pow(O.DELTA, j, R) % R * w0 % R
            col, sig = cols[j], sigmas[j]
            for i in range(rows):
                v = col[row0 + i]
                nu[i] = nu[i] * (v + x + gamma) % R
                de[i] = de[i] * (v + beta * sig[row0 + i] + gamma) % R
                x = x * omega % R
        nums.append(fr(nu))
        dens.append(fr(de))
    return nums, dens


def perm_factors_oracle(cols, sigmas, chunk_len, row0, rows, beta, gamma, omega):
    """the same on stored limbs with the C oracle's fr_mul / fr_add; the powers omega^i by repeated big-int multiplication"""
    w0 = pow(omega, row0, R)
    wp = fr([w0 * p % R for p in powers(omega, rows)])
    g, b = _rep(fr([gamma]), rows), _rep(fr([beta]), rows)
    nums, dens = [], []
    for c0 in range(0, len(cols), chunk_len):
        nu = de = None
        for j in range(c0, min(c0 + chunk_len, len(cols))):
            v, s = np.ascontiguousarray(cols[j][row0:row0 + rows]), np.ascontiguousarray(sigmas[j][row0:row0 + rows])
            a = CO.fr_add(CO.fr_add(v, CO.fr_mul(_rep(fr([beta * pow(O.DELTA, j, R) % R]), rows), wp)), g)
            d = CO.fr_add(CO.fr_add(v, CO.fr_mul(b, s)), g)
            nu, de = (a, d) if nu is None else (CO.fr_mul(nu, a), CO.fr_mul(de, d))
        nums.append(nu)
        dens.append(de)
    return nums, dens


def row_ranges(n):
    """one row at both ends and next to the start, the whole column, its upper half, and 255 / 256 / 257 rows (a workgroup less one lane, a whole
    one, a second block of one lane) from an odd start"""
    return [(0, 1), (1, 1), (n - 1, 1), (0, n), (n // 2, n // 2), (n // 3, 255), (n // 3, 256), (n // 3, 257)]


def three_way_split(n):
    a, b = n // 5 + 1, n // 5 + n // 2 + 4
    assert 0 < a < b < n and len({a, b - a, n - b}) == 3
    return [(0, a), (a, b - a), (b, n - b)]


def beta_gamma_pairs(seed):
    """full-width canonical values; r - 1 in either place; values whose stored limbs are edge patterns"""
    u = full_width_values(4, seed)
    return [(u[0], u[1]), (R - 1, u[2]), (u[3], R - 1), (stored_as((1 << 253) + 1), stored_as(R - 2))]


def _perm_rows(ctx, cols, sigmas, chunk_len, row0, rows, beta, gamma, omega):
    return ctx.permutation_product_terms_sets(cols, sigmas, chunk_len, fr([beta]), fr([gamma]), fr([O.DELTA]), fr([omega]), row0=row0, rows=rows)


def _assert_sets_equal(got, want, tag):
    (gn, gd), (wn, wd) = got, want
    assert len(gn) == len(wn) == len(gd) == len(wd), tag
    for s in range(len(wn)):
        _assert_rows_equal(gn[s], wn[s], tag + ("num", s))
        _assert_rows_equal(gd[s], wd[s], tag + ("den", s))


def check_perm_row_ranges(ctx, k, ncols=5, chunk_len=2, seed=0):
    """h2hip_permutation_product_terms_rows_dev over five columns in sets of two (a ragged last set) of 2^k rows: every range of row_ranges and an
    uneven three-way split whose pieces concatenate to the whole column, for every (beta, gamma) pair, on unsaturated limbs (quotient_29 = 1) and
    in saturated arithmetic.  Returns the number of calls."""
    n = 1 << k
    omega = O.omega_for(k)
    cols, sigmas = [full_range_fr(n, seed + 10 + j) for j in range(ncols)], [full_range_fr(n, seed + 20 + j) for j in range(ncols)]
    ci, si = [ints(c) for c in cols], [ints(c) for c in sigmas]
    assert ncols % chunk_len, "a ragged last set"
    calls = 0
    for pi, (beta, gamma) in enumerate(beta_gamma_pairs(seed + 30)):
        want = {rng: perm_factors_bigint(ci, si, chunk_len, rng[0], rng[1], beta, gamma, omega) for rng in row_ranges(n) + three_way_split(n)}
        if pi == 0:    # the oracle form (what the long ranges use) against the big-int form
            rng = (n // 3, 257)
            wo = perm_factors_oracle(cols, sigmas, chunk_len, rng[0], rng[1], beta, gamma, omega)
            _assert_sets_equal(wo, want[rng], ("reference forms",))
        for q29 in (1, 0):
            with knobs(ctx, quotient_29=q29):
                for rng in row_ranges(n):
                    _assert_sets_equal(_perm_rows(ctx, cols, sigmas, chunk_len, rng[0], rng[1], beta, gamma, omega), want[rng], ("perm rows", q29, pi, rng))
                    calls += 1
                pieces = [_perm_rows(ctx, cols, sigmas, chunk_len, r0, rn, beta, gamma, omega) for r0, rn in three_way_split(n)]
                for (r0, rn), p in zip(three_way_split(n), pieces):
                    _assert_sets_equal(p, want[(r0, rn)], ("perm rows, split", q29, pi, (r0, rn)))
                joined = tuple([np.concatenate([p[side][s] for p in pieces]) for s in range(len(pieces[0][0]))] for side in (0, 1))
                _assert_sets_equal(joined, want[(0, n)], ("perm rows, split joined", q29, pi))
                calls += 3
    return calls


LONG_K = 17
LONG_RANGES = (((1 << 16) - 7, (1 << 16) + 5), ((1 << 16) - 3, (1 << 16) - 1))   # four rows per lane from an odd start; the last size with one


def check_perm_rows_long(ctx, k=LONG_K, ranges=LONG_RANGES, ncols=5, chunk_len=2, seed=0):
    """a row range of 2^16 + 5 rows (the four-rows-per-lane launch, its xstep and the rounded-up power table under quotient_29 = 1) and one of
    2^16 - 1 rows (the last size of the one-row launch), from rows 2^16 - 7 and 2^16 - 3 of 2^17-row columns; the reference through the C oracle's field
    operations on those rows alone"""
    n = 1 << k
    omega = O.omega_for(k)
    cols, sigmas = [full_range_fr(n, seed + 40 + j) for j in range(ncols)], [full_range_fr(n, seed + 50 + j) for j in range(ncols)]
    beta, gamma = full_width_values(1, seed + 60)[0], R - 1
    assert any(rn >= LONG_ROWS and r0 for r0, rn in ranges) and any(rn == LONG_ROWS - 1 for _, rn in ranges)
    for r0, rn in ranges:
        assert r0 + rn <= n
        want = perm_factors_oracle(cols, sigmas, chunk_len, r0, rn, beta, gamma, omega)
        for q29 in (1, 0):
            with knobs(ctx, quotient_29=q29):
                _assert_sets_equal(_perm_rows(ctx, cols, sigmas, chunk_len, r0, rn, beta, gamma, omega), want, ("perm rows, long", q29, (r0, rn)))


# -------------------------------------------------------------------------------------------------------------- 5. argument errors
def _expect_error(call, tag):
    try:
        call()
    except H.H2HipError:
        return
    raise AssertionError(f"{tag}: accepted")


def check_argument_errors(ctx):
    """every rejection is followed by a small valid call that is checked against its definition: the context stays usable.  Buffers are as large as
    the rejected call would need, and none of them may change."""
    n = 4
    with _device(ctx) as buf:
        big_in, big_out = buf(full_range_fr(32 * n, 1)), buf(rows=32 * n)

        def untouched(tag):
            big_in.assert_unchanged(tag)
            big_out.assert_unchanged(tag)

        # gather: an index >= 2^log_cosets, 17 indices, log_cosets = 5
        for tag, cosets, log_c in (("gather: coset index 4 of 4", [0, 4], 2), ("gather: coset index 1 of 1", [1], 0), ("gather: count = 17", [0] * 17, 4),
                                   ("gather: log_cosets = 5", [0, 1], 5)):
            _expect_error(lambda: ctx.fr_coset_gather_dev(big_out.ptr, big_in.ptr, cosets, log_c, n), tag)
            untouched(tag)
        check_coset_gather(ctx, [(2, 5)])
        # interleave: log_cosets = 5
        _expect_error(lambda: ctx.fr_coset_interleave_dev(big_out.ptr, big_in.ptr, list(range(32)), 5, n), "interleave: log_cosets = 5")
        untouched("interleave: log_cosets = 5")
        check_coset_interleave(ctx, [(2, 5)])
        # combine: log_cosets = 5 and 0, out == in
        one = fr([1])
        for tag, out, log_c in (("combine: log_cosets = 5", big_out, 5), ("combine: log_cosets = 0", big_out, 0), ("combine: out == in", big_in, 2)):
            _expect_error(lambda: ctx.fr_coset_combine_dev(out.ptr, big_in.ptr, list(range(32)), log_c, n, one, one), tag)
            untouched(tag)
        check_coset_combine(ctx, [(2, 5)])
        # scale: a NULL column, as input or output, in the first launch group and in the second — no column of the call may have been scaled
        cols = [buf(full_range_fr(n, 10 + j)) for j in range(COSET_BATCH + 2)]
        outs = [buf(rows=n) for _ in cols]
        s = fr([O.ZETA])
        for tag, count, null_at, null_in in (("scale: NULL input", 1, 0, True), ("scale: NULL output", 3, 1, False),
                                             ("scale: NULL input in the second group", COSET_BATCH + 2, COSET_BATCH + 1, True),
                                             ("scale: NULL output in the second group", COSET_BATCH + 2, COSET_BATCH, False)):
            ip, op = [b.ptr for b in cols[:count]], [b.ptr for b in outs[:count]]
            (ip if null_in else op)[null_at] = None
            _expect_error(lambda: ctx.fr_coset_scale_batch_dev(op, ip, n, s), tag)
            for b in cols + outs:
                b.assert_unchanged(tag)
        check_coset_scale(ctx, [(5, 3)], factors=scale_factors()[2:3])
        # row-range factors: chunk_len 0 and 9
        pc, ps = [buf(full_range_fr(n, 50 + j)) for j in range(9)], [buf(full_range_fr(n, 60 + j)) for j in range(9)]
        tab = lambda bs: (HH._vp * len(bs))(*[HH._vp(b.ptr) for b in bs])
        consts = [fr([v]) for v in (5, 7, O.DELTA, O.omega_for(2))]
        for chunk_len in (0, 9):
            tag = f"row-range factors: chunk_len = {chunk_len}"
            _expect_error(lambda: ctx._chk(ctx.lib.h2hip_permutation_product_terms_rows_dev(ctx.handle, big_out.ptr, big_in.ptr, tab(pc), tab(ps), 9, chunk_len,
                                                                                          1, 2, *[HH._ptr(c) for c in consts])), tag)
            untouched(tag)
        cols_h, sig_h = [b.host[:n] for b in pc[:3]], [b.host[:n] for b in ps[:3]]
        got = _perm_rows(ctx, cols_h, sig_h, 2, 1, 2, 5, 7, O.omega_for(2))
        _assert_sets_equal(got, perm_factors_bigint([ints(c) for c in cols_h], [ints(c) for c in sig_h], 2, 1, 2, 5, 7, O.omega_for(2)), ("row-range factors",))
