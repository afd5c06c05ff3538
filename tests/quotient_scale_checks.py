"""The kernels that build h(X) (quotient.hip: gate, lookup and permutation identities, divide_by_vanishing_poly; ntt.hip: extended_to_coeff) at the
extended-domain sizes at which they change behaviour (host side only; every check takes a ctx).  From 2^19 extended points on a lane of the
permutation kernels takes 2, 4 and 8 points and carries w_ext^i forward with xstep = w_ext^(grid * 256); the gate / lookup / divide kernels sweep
the domain more than once beyond 8 workgroups per CU (2^19 points on 256 CUs); divide_by_vanishing_poly switches from kernel arguments to a table
of inverses at 2^(ext_k - k) = 16; extended_to_coeff puts a different scale on the coefficients at i mod 3 = 0, 1, 2, which only shows on data
whose coefficients from n up are not zero.  Every expected value comes from the C oracle (oracle.c_oracle) — never from another entry of
libh2hip — and every comparison is equality, limb for limb, over all 2^ext_k points.  Columns are uploaded once per shape and the entries are
called on device pointers: only the accumulator travels again per call.  Every check restores quotient_29."""
import contextlib
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from halo2_lib_amd import h2hip as HH
from oracle import bn254 as O
from oracle import c_oracle as CO
from tests.util import R, edge_fr_values, fr, rand_fr

T = 16                       # oracle threads
SWEEP = 1 << 19              # points one sweep of the gate / lookup kernels covers: 8 workgroups of 256 lanes on each of 256 CUs
LAST_ROTATION = -7
PERM_COLUMNS, CHUNK_LEN = 5, 2   # 3 sets, the last one ragged: FIRST, LAST, CHAIN and PRODUCT jobs all occur
_vp = C.c_void_p
# (terms, uses z_prev, first column index, last rotation) of the one-job calls, as in test_emu_kernels._quotient_identity_checks
SET_JOBS = ((HH.PERM_FIRST | HH.PERM_PRODUCT, False, 0, 0),
            (HH.PERM_LAST | HH.PERM_CHAIN | HH.PERM_PRODUCT, True, 3, LAST_ROTATION),
            (HH.PERM_FIRST | HH.PERM_LAST | HH.PERM_PRODUCT, False, 0, 0),
            (HH.PERM_PRODUCT, False, 3, 0))


def points_per_lane(ek):
    """extended points one lane of the permutation kernels takes (quotient.hip: perm_grid)"""
    return min(max((1 << ek) >> 18, 1), 8)


def sharded_shift():
    """a coset shift that is not ZETA, as the sharded prover passes one"""
    return 5 * O.ZETA % R


def _ptr(a):
    return a.ctypes.data_as(_vp)


def _table(ptrs):
    return (_vp * len(ptrs))(*[_vp(p) for p in ptrs])


def _rep(scalar, rows):
    return np.ascontiguousarray(np.repeat(np.asarray(scalar, dtype=np.uint64).reshape(1, 4), rows, axis=0))


def _mul(a, b):
    """CO.fr_mul over T threads (the same fe_mul per element): a product of two 2^21-row columns takes 0.08 s on one"""
    return CO.fr_mul_mt(a, b, threads=T)


def _assert_equal(got, want, tag, stride=None):
    """stride: the points one pass of the kernel's grid covers (point i is pass i // stride of lane i % stride)"""
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        where = "" if stride is None else f", in passes {sorted(set((bad // stride).tolist()))[:9]} of {stride} lanes"
        raise AssertionError(f"{tag}: {len(bad)} of {len(want)} points differ from the oracle, first {bad[:8].tolist()}{where}")


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


@contextlib.contextmanager
def _restoring_form(ctx):
    """quotient_29 is 1 again after the block"""
    try:
        yield
    finally:
        ctx.set_param("quotient_29", 1)


def random_columns(ne, seed0, count):
    """count rand_fr columns with the seeds seed0 + 2 j (rand_fr uses seed and seed + 1), drawn side by side: numpy draws without the
    interpreter lock, and at 2^21 rows a column takes a third of a second"""
    with ThreadPoolExecutor(T) as pool:
        return list(pool.map(lambda j: rand_fr(ne, seed0 + 2 * j), range(count)))


def edge_columns(ne, count):
    """count columns of the edge limb patterns of tests/util.edge_fr_values as STORED limbs, in the cyclic arrangement of
    test_emu_kernels._quotient_identity_checks(edge_patterns=True): row i of the column with seed s holds pattern (i (2 s + 1) + s) mod 25"""
    rinv = O.inv_mod(pow(2, 256, R), R)
    pat = fr([e * rinv % R for e in edge_fr_values()])
    i = np.arange(ne, dtype=np.int64)
    return [np.ascontiguousarray(pat[(i * (2 * seed + 1) + seed) % len(pat)]) for seed in range(1, count + 1)]


def _challenges(seed):
    c = rand_fr(3, seed)
    return c[0:1], c[1:2], c[2:3]   # beta, gamma, y


def _active(l_last, l_blind):
    return CO.fr_sub(_rep(fr([1]), len(l_last)), CO.fr_add(l_last, l_blind))


def _domain(k, ek, shift):
    """(ext_omega, zeta) as limbs: ZETA and the extended domain's generator, or the sharded prover's form (ext_k == k, a shift that is not ZETA,
    the generator of the 2^k domain)"""
    return fr([O.omega_for(ek)]), fr([O.ZETA if shift is None else shift])


# ------------------------------------------------------------------------------------------------ 1. the permutation argument, batched entry
def check_permutation_sets(ctx, k, ek, forms=(1, 0), shift=None, edge=False, expect_per_lane=None):
    """h2hip_quotient_permutation_sets_dev (5 columns in sets of 2, last_rotation -7) against CO.quotient_permutation"""
    ne, step = 1 << ek, 1 << (ek - k)
    per_lane = points_per_lane(ek)
    assert expect_per_lane is None or per_lane == expect_per_lane, f"2^{ek} points no longer give a lane {expect_per_lane} points: {per_lane}"
    sets = (PERM_COLUMNS + CHUNK_LEN - 1) // CHUNK_LEN
    c = edge_columns(ne, 4 + sets + 2 * PERM_COLUMNS) if edge else random_columns(ne, 100 * ek + k, 4 + sets + 2 * PERM_COLUMNS)
    (acc0, l0, l_last, l_blind), zs, cols, sigmas = c[:4], c[4:4 + sets], c[4 + sets:4 + sets + PERM_COLUMNS], c[4 + sets + PERM_COLUMNS:]
    beta, gamma, y = _challenges(7 + ek)
    ext_omega, zeta = _domain(k, ek, shift)
    delta = fr([O.DELTA])
    want = CO.quotient_permutation(acc0.copy(), zs, cols, sigmas, CHUNK_LEN, l0, l_last, _active(l_last, l_blind), step, LAST_ROTATION, beta, gamma,
                                   y, delta, zeta, ext_omega, threads=T)
    with _device(ctx) as up, _restoring_form(ctx):
        d_acc, d_l = up(acc0), [up(v) for v in (l0, l_last, l_blind)]
        pz, pc, ps = _table([up(v) for v in zs]), _table([up(v) for v in cols]), _table([up(v) for v in sigmas])
        for form in forms:
            ctx.set_param("quotient_29", form)
            ctx.upload(d_acc, acc0)
            ctx._chk(ctx.lib.h2hip_quotient_permutation_sets_dev(
                ctx.handle, _vp(d_acc), pz, sets, pc, ps, PERM_COLUMNS, CHUNK_LEN, _vp(d_l[0]), _vp(d_l[1]), _vp(d_l[2]), ek, k, LAST_ROTATION,
                _ptr(beta), _ptr(gamma), _ptr(delta), _ptr(zeta), _ptr(ext_omega), _ptr(y)))
            _assert_equal(ctx.download(d_acc, acc0.shape), want, f"permutation sets ({k}, {ek}) quotient_29={form} edge={edge}", ne // per_lane)


# ------------------------------------------------------------------------------------------------ 2. the permutation argument, one job
class SetReference:
    """O.quotient_permutation_set_terms restated on whole columns: the C oracle's field operations, X_i = zeta w^i from CO.fr_geom, rotations by
    np.roll.  Every term is computed once and shared by the masks that use it."""

    def __init__(self, z, z_prev, cols, sigmas, l0, l_last, l_blind, step, beta, gamma, delta, zeta, ext_omega, y):
        self.ne, self.step = len(z), step
        self.z, self.z_prev, self.cols, self.sigmas, self.l0, self.l_last, self.l_blind = z, z_prev, cols, sigmas, l0, l_last, l_blind
        rep = lambda s: _rep(s, self.ne)
        self.one, self.beta, self.gamma, self.y = rep(fr([1])), rep(beta), rep(gamma), rep(y)
        self.beta_i, self.delta_i = O.limbs_to_ints(beta, R)[0], O.limbs_to_ints(delta, R)[0]
        self.zeta, self.ext_omega = zeta, ext_omega
        self.memo = {}

    def _term(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def _left(self):
        v = np.roll(self.z, -self.step, axis=0)
        for p, sg in zip(self.cols, self.sigmas):
            v = _mul(v, CO.fr_add(CO.fr_add(p, _mul(self.beta, sg)), self.gamma))
        return v

    def _product(self, j0):
        x = self._term("x", lambda: CO.fr_geom(self.zeta, self.ext_omega, self.ne, threads=T))
        right, bd = self.z, self.beta_i * pow(self.delta_i, j0, R) % R
        for p in self.cols:
            right = _mul(right, CO.fr_add(CO.fr_add(p, _mul(_rep(fr([bd]), self.ne), x)), self.gamma))
            bd = bd * self.delta_i % R
        active = CO.fr_sub(self.one, CO.fr_add(self.l_last, self.l_blind))
        return _mul(active, CO.fr_sub(self._term("left", self._left), right))

    def fold(self, acc, terms, j0, rot):
        z, f = self.z, lambda v, t: CO.fr_add(_mul(v, self.y), t)
        v = acc
        if terms & HH.PERM_FIRST:
            v = f(v, self._term("first", lambda: _mul(self.l0, CO.fr_sub(self.one, z))))
        if terms & HH.PERM_LAST:
            v = f(v, self._term("last", lambda: _mul(self.l_last, CO.fr_sub(_mul(z, z), z))))
        if terms & HH.PERM_CHAIN:
            v = f(v, self._term(("chain", rot), lambda: _mul(self.l0, CO.fr_sub(z, np.roll(self.z_prev, -rot * self.step, axis=0)))))
        if terms & HH.PERM_PRODUCT:
            v = f(v, self._term(("product", j0), lambda: self._product(j0)))
        return v


def check_permutation_set_jobs(ctx, k, ek, forms=(1, 0), expect_per_lane=None):
    """h2hip_quotient_permutation_set_dev (3 columns; the dedicated kernel under quotient_29 = 1, the batch kernel with one job under 0) for
    every mask of SET_JOBS against SetReference"""
    ne, step = 1 << ek, 1 << (ek - k)
    per_lane = points_per_lane(ek)
    assert expect_per_lane is None or per_lane == expect_per_lane, f"2^{ek} points no longer give a lane {expect_per_lane} points: {per_lane}"
    c = random_columns(ne, 300 * ek + k, 12)
    (acc0, z, z_prev, l0, l_last, l_blind), cols, sigmas = c[:6], c[6:9], c[9:]
    beta, gamma, y = _challenges(11 + ek)
    ext_omega, zeta = _domain(k, ek, None)
    delta = fr([O.DELTA])
    ref = SetReference(z, z_prev, cols, sigmas, l0, l_last, l_blind, step, beta, gamma, delta, zeta, ext_omega, y)
    want = [ref.fold(acc0, terms, j0, rot) for terms, _, j0, rot in SET_JOBS]
    del ref
    with _device(ctx) as up, _restoring_form(ctx):
        d_acc, d_z, d_zp, d_l = up(acc0), up(z), up(z_prev), [up(v) for v in (l0, l_last, l_blind)]
        pc, ps = _table([up(v) for v in cols]), _table([up(v) for v in sigmas])
        for form in forms:
            ctx.set_param("quotient_29", form)
            for (terms, chained, j0, rot), w in zip(SET_JOBS, want):
                ctx.upload(d_acc, acc0)
                ctx._chk(ctx.lib.h2hip_quotient_permutation_set_dev(
                    ctx.handle, _vp(d_acc), _vp(d_z), _vp(d_zp) if chained else None, pc, ps, 3, j0, _vp(d_l[0]), _vp(d_l[1]), _vp(d_l[2]), ek, k,
                    terms, rot, _ptr(beta), _ptr(gamma), _ptr(delta), _ptr(zeta), _ptr(ext_omega), _ptr(y)))
                _assert_equal(ctx.download(d_acc, acc0.shape), w, f"permutation set ({k}, {ek}) quotient_29={form} terms={terms}", ne // per_lane)


def check_set_reference_against_bigint(k=4, ek=6):
    """SetReference against O.quotient_permutation_set_terms (Python big-int arithmetic) for every mask of SET_JOBS"""
    ne, step = 1 << ek, 1 << (ek - k)
    c = random_columns(ne, 50, 12)
    (acc0, z, z_prev, l0, l_last, l_blind), cols, sigmas = c[:6], c[6:9], c[9:]
    beta, gamma, y = _challenges(3)
    ext_omega, zeta = _domain(k, ek, None)
    ref = SetReference(z, z_prev, cols, sigmas, l0, l_last, l_blind, step, beta, gamma, fr([O.DELTA]), zeta, ext_omega, y)
    to_i = lambda a: O.limbs_to_ints(a, R)
    (bi,), (gi,), (yi,) = to_i(beta), to_i(gamma), to_i(y)
    for terms, chained, j0, rot in SET_JOBS:
        want = O.quotient_permutation_set_terms(to_i(acc0), to_i(z), to_i(z_prev) if chained else None, [to_i(c) for c in cols],
                                                [to_i(c) for c in sigmas], j0, to_i(l0), to_i(l_last), to_i(l_blind), step, terms, rot % (1 << k),
                                                bi, gi, O.DELTA, O.ZETA, O.omega_for(ek), yi)
        assert to_i(ref.fold(acc0, terms, j0, rot)) == want, terms


# ------------------------------------------------------------------------------------------------ 3. gate columns and lookups, batched entries
def check_gate_batch(ctx, k, ek, forms=(1, 0), columns=3):
    """h2hip_quotient_flex_gate_batch_dev against CO.quotient_gate folded column by column"""
    ne, step = 1 << ek, 1 << (ek - k)
    c = random_columns(ne, 500 * ek + k, 1 + 2 * columns)
    acc0, qs, advs = c[0], c[1:1 + columns], c[1 + columns:]
    y = _challenges(13 + ek)[2]
    want = acc0.copy()
    for q, a in zip(qs, advs):
        CO.quotient_gate(want, q, a, y, step, threads=T)
    with _device(ctx) as up, _restoring_form(ctx):
        d_acc = up(acc0)
        pq, pa = _table([up(v) for v in qs]), _table([up(v) for v in advs])
        for form in forms:
            ctx.set_param("quotient_29", form)
            ctx.upload(d_acc, acc0)
            ctx._chk(ctx.lib.h2hip_quotient_flex_gate_batch_dev(ctx.handle, _vp(d_acc), pq, pa, columns, ek, k, _ptr(y)))
            _assert_equal(ctx.download(d_acc, acc0.shape), want, f"gate batch ({k}, {ek}) quotient_29={form}", SWEEP)


def check_lookups(ctx, k, ek, forms=(1, 0), lookups=2):
    """h2hip_quotient_lookups_dev against CO.quotient_lookup folded in order"""
    ne, step = 1 << ek, 1 << (ek - k)
    c = random_columns(ne, 700 * ek + k, 4 + 5 * lookups)
    acc0, l0, l_last, l_blind = c[:4]
    five = [c[4 + lookups * t:4 + lookups * (t + 1)] for t in range(5)]   # z, a, s, a', s'
    beta, gamma, y = _challenges(17 + ek)
    want, active = acc0.copy(), _active(l_last, l_blind)
    for j in range(lookups):
        CO.quotient_lookup(want, *[five[t][j] for t in range(5)], l0, l_last, active, step, beta, gamma, y, threads=T)
    with _device(ctx) as up, _restoring_form(ctx):
        d_acc, d_l = up(acc0), [up(v) for v in (l0, l_last, l_blind)]
        tabs = [_table([up(v) for v in five[t]]) for t in range(5)]
        for form in forms:
            ctx.set_param("quotient_29", form)
            ctx.upload(d_acc, acc0)
            ctx._chk(ctx.lib.h2hip_quotient_lookups_dev(ctx.handle, _vp(d_acc), *tabs, lookups, _vp(d_l[0]), _vp(d_l[1]), _vp(d_l[2]), ek, k,
                                                        _ptr(beta), _ptr(gamma), _ptr(y)))
            _assert_equal(ctx.download(d_acc, acc0.shape), want, f"lookups ({k}, {ek}) quotient_29={form}", SWEEP)


# ------------------------------------------------------------------------------------------------ 4. divide_by_vanishing_poly
def check_divide(ctx, k, ek, shift=None):
    """h2hip_divide_by_vanishing_poly_dev against CO.divide_by_vanishing: 2^(ext_k - k) <= 8 inverses travel as kernel arguments, more come out
    of a table on the device"""
    a = rand_fr(1 << ek, 900 * ek + k)
    ext_omega, zeta = _domain(k, ek, shift)
    want = CO.divide_by_vanishing(a.copy(), ek, k, ext_omega, zeta, threads=T)
    with _device(ctx) as up:
        d = up(a)
        ctx._chk(ctx.lib.h2hip_divide_by_vanishing_poly_dev(ctx.handle, _vp(d), ek, k, _ptr(ext_omega), _ptr(zeta)))
        _assert_equal(ctx.download(d, a.shape), want, f"divide_by_vanishing_poly ({k}, {ek})", SWEEP)


def check_divide_refuses_long_tables(ctx, ek=17):
    """ext_k - k = 17 is H2HIP_ERR_INVALID with the entry's message, the data stays as it was, and a correct call on the same context succeeds"""
    a = rand_fr(1 << ek, 33)
    ext_omega, zeta = _domain(0, ek, None)
    with _device(ctx) as up:
        d = up(a)
        rc = ctx.lib.h2hip_divide_by_vanishing_poly_dev(ctx.handle, _vp(d), ek, 0, _ptr(ext_omega), _ptr(zeta))
        assert rc == -1, rc   # H2HIP_ERR_INVALID
        msg = ctx.lib.h2hip_last_error().decode()
        assert msg == "h2hip_divide_by_vanishing_poly_dev: invalid argument: need k <= ext_k <= 28 and ext_k - k <= 16", msg
        assert np.array_equal(ctx.download(d, a.shape), a)
        ctx._chk(ctx.lib.h2hip_divide_by_vanishing_poly_dev(ctx.handle, _vp(d), ek, 1, _ptr(ext_omega), _ptr(zeta)))
        _assert_equal(ctx.download(d, a.shape), CO.divide_by_vanishing(a.copy(), ek, 1, ext_omega, zeta, threads=T), "divide after a refused call")


# ------------------------------------------------------------------------------------------------ 5. extended_to_coeff on full-degree data
def _inverse_domain(ek):
    return fr([O.inv_mod(O.omega_for(ek), R)]), fr([O.inv_mod(1 << ek, R)]), fr([O.ZETA * O.ZETA % R])   # w_ext^-1, 2^-ext_k, ZETA^-1


def check_extended_to_coeff_full_degree(ctx, ek):
    """h2hip_extended_to_coeff_dev on random evaluations (coefficients up to degree 2^ext_k - 1, as h(X)'s reach past n) against
    CO.extended_to_coeff, all 2^ext_k outputs"""
    a = rand_fr(1 << ek, 1100 + ek)
    ext_omega, zeta = _domain(ek, ek, None)
    want = CO.extended_to_coeff(a, ek, ext_omega, zeta, threads=T)
    with _device(ctx) as up:
        d = up(a)
        ctx.extended_to_coeff_dev(d, ek, *_inverse_domain(ek))
        _assert_equal(ctx.download(d, a.shape), want, f"extended_to_coeff 2^{ek}")


def check_coeff_to_extended_in_place(ctx, ek):
    """h2hip_coeff_to_extended_dev with k == ext_k and coeffs_dev == out_dev (the one aliasing the entry allows) against CO.coeff_to_extended"""
    a = rand_fr(1 << ek, 1300 + ek)
    ext_omega, zeta = _domain(ek, ek, None)
    want = CO.coeff_to_extended(a, ek, ek, ext_omega, zeta, threads=T)
    with _device(ctx) as up:
        d = up(a)
        ctx.coeff_to_extended_dev(d, ek, d, ek, ext_omega, zeta)
        _assert_equal(ctx.download(d, a.shape), want, f"coeff_to_extended in place 2^{ek}")


# ------------------------------------------------------------------------------------------------ 6. the chain as the prover queues it
def check_chain(ctx, k, ek):
    """gate batch -> permutation sets -> lookups -> divide -> extended_to_coeff on ONE device accumulator with no host round trip in between
    (one gate column, 3 permutation columns in sets of 2, one lookup) against the same chain of oracle calls: the hand-over between the kernels
    (the workspace of the divide, the power table the permutation kernels share with the transform, the stream order)"""
    ne, step = 1 << ek, 1 << (ek - k)
    ncols, sets = 3, 2
    c = random_columns(ne, 1500 * ek + k, 19)
    (acc0, l0, l_last, l_blind, q, adv), zs, cols, sigmas, five = c[:6], c[6:8], c[8:11], c[11:14], c[14:]
    beta, gamma, y = _challenges(19 + ek)
    ext_omega, zeta = _domain(k, ek, None)
    delta = fr([O.DELTA])
    want, active = acc0.copy(), _active(l_last, l_blind)
    CO.quotient_gate(want, q, adv, y, step, threads=T)
    CO.quotient_permutation(want, zs, cols, sigmas, CHUNK_LEN, l0, l_last, active, step, LAST_ROTATION, beta, gamma, y, delta, zeta, ext_omega, threads=T)
    CO.quotient_lookup(want, *five, l0, l_last, active, step, beta, gamma, y, threads=T)
    CO.divide_by_vanishing(want, ek, k, ext_omega, zeta, threads=T)
    want = CO.extended_to_coeff(want, ek, ext_omega, zeta, threads=T)
    with _device(ctx) as up:
        d_acc, d_l = up(acc0), [_vp(up(v)) for v in (l0, l_last, l_blind)]
        one = lambda v: _table([up(v)])
        ctx._chk(ctx.lib.h2hip_quotient_flex_gate_batch_dev(ctx.handle, _vp(d_acc), one(q), one(adv), 1, ek, k, _ptr(y)))
        ctx._chk(ctx.lib.h2hip_quotient_permutation_sets_dev(
            ctx.handle, _vp(d_acc), _table([up(v) for v in zs]), sets, _table([up(v) for v in cols]), _table([up(v) for v in sigmas]), ncols, CHUNK_LEN,
            *d_l, ek, k, LAST_ROTATION, _ptr(beta), _ptr(gamma), _ptr(delta), _ptr(zeta), _ptr(ext_omega), _ptr(y)))
        ctx._chk(ctx.lib.h2hip_quotient_lookups_dev(ctx.handle, _vp(d_acc), *[one(v) for v in five], 1, *d_l, ek, k, _ptr(beta), _ptr(gamma), _ptr(y)))
        ctx._chk(ctx.lib.h2hip_divide_by_vanishing_poly_dev(ctx.handle, _vp(d_acc), ek, k, _ptr(ext_omega), _ptr(zeta)))
        ctx.extended_to_coeff_dev(d_acc, ek, *_inverse_domain(ek))
        _assert_equal(ctx.download(d_acc, acc0.shape), want, f"chain ({k}, {ek})")
