"""Differential checks of the tuning knobs (include/h2hip.h, h2hip_set_param): every knob selects a kernel path, a launch geometry or a
schedule and claims "same results" — proof-byte equality only checks that claim at the knob's default.  Each check here sets knob values
from the knob's legal domain, runs the operation the knob steers and compares it bit for bit with the C oracle (or, at GPU sizes, with the
known-dlog closed form of CO.known_dlog_bases).  Shared by the emulated build (CPU suite, small sizes) and the GPU suite (real sizes).
Every check restores the knobs it touched, also when it fails."""
import contextlib
import itertools

import numpy as np

import halo2_lib_amd as H
from halo2_lib_amd.h2hip import BASES_PLAIN, BASES_PRECOMPUTE
from oracle import bn254 as O
from oracle import c_oracle as CO
from tests.util import R, domain_consts, fr, full_range_fr, jac_to_affine_ints, rand_fr


@contextlib.contextmanager
def knobs(ctx, **vals):
    """set knobs for the duration of the block; the previous values come back in any case"""
    old = {n: ctx.get_param(n) for n in vals}
    try:
        for n, v in vals.items():
            ctx.set_param(n, v)
        yield
    finally:
        for n, v in old.items():
            ctx.set_param(n, v)


def pairwise(params):
    """a deterministic list of rows (dicts) in which every pair of values of every two parameters occurs at least once (greedy covering)"""
    names = list(params)
    todo = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in params[a] for vb in params[b]}
    rows = []
    while todo:
        a, va, b, vb = min(todo, key=lambda t: (names.index(t[0]), names.index(t[2]), params[t[0]].index(t[1]), params[t[2]].index(t[3])))
        row = {a: va, b: vb}
        for n in names:
            if n in row:
                continue
            gain = lambda v: sum(((m, row[m], n, v) if names.index(m) < names.index(n) else (n, v, m, row[m])) in todo for m in row)
            row[n] = max(params[n], key=gain)   # (ties: the first value)
        rows.append(row)
        todo -= {(m, row[m], n, row[n]) for m, n in itertools.combinations(names, 2)}
    return rows


# ---------------------------------------------------------------------------------------------------------------------------- MSM columns
def scalar_column(kind, n, seed):
    if kind == "uniform":
        return rand_fr(n, seed)
    if kind == "equal":   # one bucket per window: every chunk puts all its entries into the same bucket
        return np.ascontiguousarray(np.repeat(full_range_fr(1, seed, edges=False), n, axis=0))
    if kind == "one":
        return np.ascontiguousarray(np.repeat(fr([1]), n, axis=0))
    if kind == "zero_one":
        return np.ascontiguousarray(fr([0, 1])[np.random.default_rng(seed).integers(0, 2, size=n)])
    if kind == "zero":
        return np.zeros((n, 4), dtype=np.uint64)
    if kind == "full_range":
        return full_range_fr(n, seed)
    raise ValueError(kind)


K0, D = 987654321, 31   # bases i * G with dlog K0 + i * D


def dlog_bases(n):
    return CO.known_dlog_bases(n, fr([K0]), fr([D]))


def closed_form(s):
    """sum_i s_i * (K0 + i * D) * G as an affine point (None = identity): independent of any MSM implementation"""
    si = O.limbs_to_ints(s, R)
    a = sum(si) % R
    b = sum(i * v for i, v in enumerate(si)) % R
    total = (K0 * a + D * b) % R
    return O.g1_mul(O.G1_GEN, total) if total else None


def _affine(got):
    return O.limbs_to_points(got)[0] if got.any() else None


def expected_msm(s, bases, threads, exact):
    """the oracle's affine limbs (exact=True: the C oracle's best_multiexp) or the closed form's point"""
    return CO.best_multiexp(s, bases, threads=threads) if exact else closed_form(s)


def same_point(got, want):
    if isinstance(want, np.ndarray):
        return np.array_equal(got, want)
    return _affine(got) == want


def as_point(want):
    """an expected_msm result as an affine point (None = identity)"""
    return _affine(want) if isinstance(want, np.ndarray) else want


# ------------------------------------------------------------------------------------------------------------------ 1. MSM sort geometry
SORT_KNOBS = {
    "msm_hist_split": [1, 2, 4, 8, 16, 32, 64],
    "msm_scatter_split": [1, 2, 4, 8, 16, 32, 64],
    "msm_hist_packed": [0, 1],
    "msm_scatter_full_lds": [0, 1],
    "msm_sort_threads": [256, 512, 1024],
    "msm_sort_groups": [1, 2, 31, 33, 1024],
}
KINDS = ["uniform", "equal", "zero_one", "full_range"]


def check_msm_sort_geometry(ctx, n, windows, threads, exact=True):
    """the counting sort's launch geometry: histogram / scatter sub-ranges (clamped to B at small windows), packed and plain counters, the
    scatter's LDS declaration, workgroup sizes and chunk counts — pairwise over the knobs, the window sizes and the scalar columns"""
    bases = dlog_bases(n)
    b = ctx.bases_upload(bases)
    cols = {k: scalar_column(k, n, 40 + i) for i, k in enumerate(KINDS)}
    want = {k: expected_msm(s, bases, threads, exact) for k, s in cols.items()}
    rows = pairwise(dict(SORT_KNOBS, msm_window_bits=list(windows), kind=KINDS))
    try:
        for row in rows:
            kind = row.pop("kind")
            with knobs(ctx, **row):
                got = ctx.msm(b, cols[kind], H.POINT_AFFINE)
            assert same_point(got, want[kind]), (kind, row)
    finally:
        b.free()
    return len(rows)


def check_packed_counter_boundary(ctx, sizes, threads):
    """(GPU sizes) chunks that each put exactly 65535 entries into ONE bucket — the most a packed 16-bit counter holds (chunk_cap) — and one
    entry more in a last chunk: all-equal and all-one columns, packed and plain histogram, plain and precomputed bases"""
    for n in sizes:
        bases = dlog_bases(n)
        sum_k = (K0 * n + D * (n * (n - 1) // 2)) % R   # sum of the bases' dlogs
        for flags in (BASES_PLAIN, BASES_PRECOMPUTE):
            b = ctx.bases_upload(bases, flags)
            try:
                for kind in ("equal", "one"):
                    s = scalar_column(kind, n, 7)
                    v = O.limbs_to_ints(s[:1], R)[0]
                    want = O.g1_mul(O.G1_GEN, v * sum_k % R)
                    for packed in (1, 0):
                        with knobs(ctx, msm_hist_packed=packed):
                            got = ctx.msm(b, s, H.POINT_AFFINE)
                        assert _affine(got) == want, (n, flags, kind, packed)
            finally:
                b.free()


# ---------------------------------------------------------------------------------------------------------- 2. accumulation and reduction
def check_msm_chunk_lone(ctx, n, threads, exact=True, values=(-1, 0, 1, 2, 7, 4096)):
    bases = dlog_bases(n)
    s = scalar_column("uniform", n, 11)
    want = expected_msm(s, bases, threads, exact)
    b = ctx.bases_upload(bases)
    try:
        for v in values:
            with knobs(ctx, msm_chunk_lone=v):
                assert same_point(ctx.msm(b, s, H.POINT_AFFINE), want), v
    finally:
        b.free()


def check_msm_quad_seg_max(ctx, n, window_bits, threads, exact=True):
    """the bucket reduction's quad-lane / one-lane switch on both sides of the shape's segment count (plain bases: ceil(255 / c) windows of
    2^(c-1) / msm_seg segments each)"""
    bases = dlog_bases(n)
    s = scalar_column("full_range", n, 12)
    want = expected_msm(s, bases, threads, exact)
    B = 1 << (window_bits - 1)
    nseg = -(-255 // window_bits) * (B // min(ctx.get_param("msm_seg"), B))
    b = ctx.bases_upload(bases)
    try:
        with knobs(ctx, msm_window_bits=window_bits, msm_quad_tails=1):
            for v in (0, nseg - 1, nseg, 32768):
                with knobs(ctx, msm_quad_seg_max=v):
                    assert same_point(ctx.msm(b, s, H.POINT_AFFINE), want), (v, nseg)
    finally:
        b.free()
    return nseg


def check_msm_table_split(ctx, n, k, threads, exact=True):
    """msm_table_split is read when a base set is made: uploaded (plain and precomputed), generated by params_kzg_setup, or converted by
    g1_to_lagrange — each made under both values, then used"""
    bases = dlog_bases(n)
    s = scalar_column("uniform", n, 13)
    want = expected_msm(s, bases, threads, exact)
    sk = rand_fr(1 << k, 14)
    toxic = fr([0x1D0C0FFEE + k])
    out = {}
    for split in (0, 1):
        with knobs(ctx, msm_table_split=split):
            for flags in (BASES_PLAIN, BASES_PRECOMPUTE):
                b = ctx.bases_upload(bases, flags)
                try:
                    assert same_point(ctx.msm(b, s, H.POINT_AFFINE), want), (split, flags)
                finally:
                    b.free()
                g, gl = ctx.params_kzg_setup(k, toxic, flags)
                lg = ctx.g1_to_lagrange(g, k, flags)
                try:
                    out[(split, flags)] = (ctx.msm(g, sk), ctx.msm(gl, sk), ctx.msm(lg, sk), ctx.bases_download(g), ctx.bases_download(gl))
                finally:
                    for x in (g, gl, lg):
                        x.free()
    ref = out[(1, BASES_PLAIN)]
    g_pts, gl_pts = ref[3], ref[4]
    assert np.array_equal(ref[1], ref[2])   # g1_to_lagrange(g) == the setup's own Lagrange set
    assert np.array_equal(ref[0], CO.best_multiexp(sk, g_pts, threads=threads))
    assert np.array_equal(ref[1], CO.best_multiexp(sk, gl_pts, threads=threads))
    for key, v in out.items():
        assert all(np.array_equal(x, y) for x, y in zip(v, ref)), key


# ------------------------------------------------------------------------------------------------------------------------ 3. batch driver
BATCH_KNOBS = {"msm_lanes": [1, 2, 3, 4], "msm_stagger_sorts": [-1, 0, 1], "clean_on_lane": [0, 1], "ncols": [1, 3, 5, 9],
               "precompute": [0, 1], "msm_fuse_cols": [0, 1]}


def check_msm_batch_driver(ctx, n, threads, exact=True):
    """msm_batch_dev / msm_multi_dev over 1, 3, 5 and 9 columns (an all-zero column among them; counts that are not multiples of the lane count)
    with every lane count, sort stagger and bucket clean-up stream; precomputed bases with fused (auto) and per-column (msm_fuse_cols = 1) lanes.
    Every column of every call is checked."""
    bases = dlog_bases(n)
    pool = [scalar_column(k, n, 60 + i) for i, k in enumerate(["uniform", "zero", "zero_one", "full_range", "equal", "uniform"])]
    want = [expected_msm(s, bases, threads, exact) for s in pool]
    dev = [ctx.to_device(s) for s in pool]
    bs = {f: ctx.bases_upload(bases, f) for f in (BASES_PLAIN, BASES_PRECOMPUTE)}
    rows = pairwise(BATCH_KNOBS)
    try:
        for i, row in enumerate(rows):
            row = dict(row)
            ncols, pre = row.pop("ncols"), row.pop("precompute")
            b = bs[BASES_PRECOMPUTE if pre else BASES_PLAIN]
            idx = [(i + j) % len(pool) for j in range(ncols)]
            if 1 not in idx:
                idx[-1] = 1   # the all-zero column
            with knobs(ctx, **row):
                if i % 2:
                    got = ctx.msm_multi_dev([b] * ncols, [dev[j] for j in idx], n, H.POINT_JACOBIAN)
                else:
                    got = ctx.msm_batch_dev(b, [dev[j] for j in idx], n, H.POINT_JACOBIAN)
            for c, j in enumerate(idx):
                assert jac_to_affine_ints(got[c]) == as_point(want[j]), (row, ncols, pre, c, j)
    finally:
        for d in dev:
            ctx.free(d)
        for x in bs.values():
            x.free()
    return len(rows)


# -------------------------------------------------------------------------------------------------------------------------------- 4. NTT
def check_ntt_knobs(ctx, log_n, ext, threads):
    """ntt_full_table x ntt_min_col_bits x ntt_tile_bits (pairwise) on the forward transform, the inverse with divisor, the coset extension
    and its inverse, and the batched column transforms — at log_n <= 23, where the first pass reads the full omega^e table"""
    a = full_range_fr(1 << log_n, 70 + log_n)
    w, winv, div = domain_consts(log_n)
    want_f = CO.best_fft(a, log_n, w, threads=threads)
    ek = log_n + ext
    we, weinv, ediv = domain_consts(ek)
    z, zinv = fr([O.ZETA]), fr([O.ZETA * O.ZETA % R])
    want_ext = CO.coeff_to_extended(a, log_n, ek, we, z, threads=threads)
    cols = [full_range_fr(1 << log_n, 80 + j) for j in range(3)]
    want_cols = [CO.ifft(c, log_n, w, threads=threads) for c in cols]
    for mc in range(6):
        for ti, tb in enumerate((4, 6, 10)):
            ft = (mc + ti) % 2
            with knobs(ctx, ntt_full_table=ft, ntt_min_col_bits=mc, ntt_tile_bits=tb):
                got = ctx.best_fft(a, w, log_n)
                assert np.array_equal(got, want_f), (ft, mc, tb)
                assert np.array_equal(ctx.ifft(got, winv, log_n, div), a), (ft, mc, tb)
                e = ctx.coeff_to_extended(a, log_n, ek, we, z)
                assert np.array_equal(e, want_ext), (ft, mc, tb)
                back = ctx.extended_to_coeff(e, ek, weinv, ediv, zinv)
                assert np.array_equal(back[: 1 << log_n], a) and not back[1 << log_n:].any(), (ft, mc, tb)
                ds = [ctx.to_device(c) for c in cols]
                try:
                    ctx.ifft_batch_dev(ds, winv, log_n, div)
                    for d, wc in zip(ds, want_cols):
                        assert np.array_equal(ctx.download(d, wc.shape), wc), (ft, mc, tb)
                finally:
                    for d in ds:
                        ctx.free(d)


# ----------------------------------------------------------------------------------------------------------------------- 5. kate division
def check_kate_knobs(ctx, threads=4):
    """kate_coeffs_per_lane (0 = by length, 1, 2, 4, 8) on the multi-point, accumulating and sets variants, at n = 256 J - 1, 256 J, 256 J + 1
    for every J and at 1, 2 and 8 points, each with kate_29 at 0 and 1"""
    sizes = [256 * j + d for j in (1, 2, 4, 8) for d in (-1, 0, 1)]
    polys = {n: [full_range_fr(n, 900 + n), full_range_fr(n, 901 + n)] for n in sizes}
    pts = {m: full_range_fr(m, 910 + m) for m in (1, 2, 8)}
    ws = {m: full_range_fr(m, 920 + m) for m in (1, 2, 8)}

    def lincomb(c, m, acc=None):
        out = acc
        for j in range(m):
            q = CO.fr_kate_division(c, pts[m][j:j + 1])
            t = CO.fr_mul(q, np.repeat(ws[m][j:j + 1], len(q), axis=0))
            out = t if out is None else CO.fr_add(out, t)
        return out

    want = {}
    for n in sizes:
        for m in (1, 2, 8):
            want[(n, m, 0)] = lincomb(polys[n][0], m)
            want[(n, m, 1)] = lincomb(polys[n][1], m)
    calls = 0
    for J in (0, 1, 2, 4, 8):
        for i, n in enumerate(sizes):
            for k29 in (0, 1):
                m = (1, 2, 8)[(i + k29 + J) % 3]
                c0, c1 = polys[n]
                with knobs(ctx, kate_coeffs_per_lane=J, kate_29=k29):
                    assert np.array_equal(ctx.fr_kate_division_multi(c0, pts[m], ws[m]), want[(n, m, 0)]), (J, n, m, k29)
                    acc = full_range_fr(n - 1, 930 + n)
                    assert np.array_equal(ctx.fr_kate_division_multi_acc(acc, c0, pts[m], ws[m]), CO.fr_add(acc, want[(n, m, 0)])), (J, n, m, k29)
                    m2 = (1, 2, 8)[(i + k29 + J + 1) % 3]
                    got = ctx.fr_kate_division_sets([c0, c1], [pts[m], pts[m2]], [ws[m], ws[m2]])
                    assert np.array_equal(got, CO.fr_add(want[(n, m, 0)], want[(n, m2, 1)])), (J, n, m, m2, k29)
                calls += 3
    return calls


# --------------------------------------------------------------------------------------------------------------------- 6. batch inversion
def check_invert_run(ctx, ns):
    """fr_invert_run (elements per lane) with n not a multiple of the run, zeros scattered in, and an all-zero column: the in-place API and
    the out-of-place inversion inside the grand products"""
    for run in (0, 1, 2, 3, 1023, 1024):
        with knobs(ctx, fr_invert_run=run):
            for n in ns:
                a = full_range_fr(n, 1000 + n + run)
                a[np.random.default_rng(run + n).integers(0, n, size=max(1, n // 7))] = 0
                assert np.array_equal(ctx.fr_batch_invert(a), CO.fr_batch_invert(a)), (run, n)
                z = np.zeros((n, 4), dtype=np.uint64)
                assert np.array_equal(ctx.fr_batch_invert(z), z), (run, n)
                num, den = full_range_fr(n, 1001 + n), full_range_fr(n, 1002 + n)
                den[~den.any(axis=1)] = fr([5])[0]   # the grand product divides: no zero denominators
                want = CO.fr_grand_product(num, den)
                assert np.array_equal(ctx.fr_grand_product(num, den), want), (run, n)
                num2, den2 = full_range_fr(n, 1003 + n), full_range_fr(n, 1004 + n)
                den2[~den2.any(axis=1)] = fr([7])[0]
                want2 = CO.fr_grand_product(num2, den2)
                got = ctx.fr_grand_products([num, num2], [den, den2], chained=False)
                assert np.array_equal(got[0], want) and np.array_equal(got[1], want2), (run, n)
                got = ctx.fr_grand_products([num, num2], [den, den2], chained=True)
                chained2 = CO.fr_mul(np.repeat(want[-1:], n + 1, axis=0), want2)
                assert np.array_equal(got[0], want) and np.array_equal(got[1], chained2), (run, n)
