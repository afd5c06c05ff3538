"""Curve arithmetic on DEGENERATE base sets through every MSM path (host side only; takes a ctx).  Every other base set of the suite
(CO.known_dlog_bases, a KZG setup) holds distinct points, none the identity, none the negative of another, so the three exceptional cases
of a curve addition — P + P (must fall through to a doubling), P + (-P) (must give the identity), identity + P — essentially never occur
above a handful of points.  Here every base is k_i * P for a small k_i in {-M .. M} (k = 0: the identity) and a fixed non-generator P:
collisions in every bucket, every run, every merge level, every table window.  Every case is held against TWO independent references,
both by exact equality: the C oracle's best_multiexp (bit for bit) and the closed form (sum_i s_i * k_i mod r) * P from Python integers
and O.g1_mul, itself checked against O.g1_mul_complete — it depends on no MSM implementation.  Shared by the emulated build (CPU suite,
small sizes) and the GPU suite (real sizes).  Every check restores the knobs it touched, also when it fails."""
import numpy as np

import halo2_lib_amd as H
from halo2_lib_amd.h2hip import BASES_PLAIN, BASES_PRECOMPUTE
from oracle import bn254 as O
from oracle import c_oracle as CO
from tests.knob_checks import knobs
from tests.util import Q, R, _raw_limbs, circuit_like_fr, domain_consts, edge_fr_values, fr, full_range_fr, jac_to_affine_ints, rand_fr

P0 = O.g1_mul(O.G1_GEN, 0xDEADBEEF)   # the fixed non-generator point all bases are small multiples of
MMAX = 6
_RINV = pow(1 << 256, -1, R)


def _signed_multiples(mul, neg, base, M):
    """[-M * base, ..., -base, identity, base, ..., M * base]"""
    pos = [mul(base, k) for k in range(1, M + 1)]
    return [neg(p) for p in reversed(pos)] + [None] + pos


_G1_POINTS = _signed_multiples(O.g1_mul, O.g1_neg, P0, MMAX)
_G1_LIMBS = O.points_to_limbs(_G1_POINTS)   # row k + MMAX = k * P0; row MMAX (k = 0) is all-zero, as points_to_limbs([None]) is


def limbs_of_dlogs(k):
    k = np.asarray(k, dtype=np.int64)
    assert len(k) == 0 or (k.min() >= -MMAX and k.max() <= MMAX)
    return np.ascontiguousarray(_G1_LIMBS[k + MMAX])


def small_dlog_bases(n, M, seed, identity_share=0.1):
    """(limbs of k_i * P0, k_i): k_i uniform over {-M .. M}, and a further `identity_share` of the positions set to the identity"""
    assert 1 <= M <= MMAX
    g = np.random.default_rng([seed, M, 0xDE6E])
    k = g.integers(-M, M + 1, size=n)
    k[g.random(n) < identity_share] = 0
    return limbs_of_dlogs(k), k


FIXED_SETS = ("identity", "first", "last", "equal", "alternating")


def fixed_dlogs(kind, n):
    k = np.zeros(n, dtype=np.int64)
    if kind == "first" and n:
        k[0] = 3
    elif kind == "last" and n:
        k[-1] = 3
    elif kind == "equal":
        k[:] = 2
    elif kind == "alternating":
        k[0::2], k[1::2] = 1, -1
    elif kind != "identity":
        assert kind in ("first", "last"), kind
    return k


SCALAR_KINDS = ("rand", "circuit", "full_range", "few", "cancel", "cancel_late")


def make_case(n, base_kind, scalar_kind, seed):
    """(bases limbs, dlogs k, scalars) — base_kind: 1 / 6 (small_dlog_bases with that M) or a name from FIXED_SETS.  The cancelling kinds pair
    every entry with a partner that holds the same scalar on the OPPOSITE base (the partner's dlog is overwritten): next to it ("cancel":
    every run sums to the identity inside a lane or across two) or n/2 entries away ("cancel_late": the partial sums are non-trivial and cancel
    only in the merge or in the bucket reduction).  An unpaired last entry gets the scalar 0."""
    k = fixed_dlogs(base_kind, n) if isinstance(base_kind, str) else small_dlog_bases(n, base_kind, seed)[1]
    if scalar_kind == "rand":
        s = rand_fr(n, seed)
    elif scalar_kind == "circuit":
        s = circuit_like_fr(n, seed)
    elif scalar_kind == "full_range":
        s = full_range_fr(n, seed)
    elif scalar_kind == "few":   # 2..5 distinct values: a window has a handful of buckets, each a run of ~n/5 entries over many lanes, waves, merge levels
        vals = full_range_fr(2 + seed % 4, seed + 1, edges=False)
        s = np.ascontiguousarray(vals[np.random.default_rng(seed).integers(0, len(vals), size=n)])
    elif scalar_kind in ("cancel", "cancel_late"):
        h = n // 2
        half = full_range_fr(h, seed, edges=False) if seed % 2 else rand_fr(h, seed)
        if seed % 3 == 0 and h:   # every third case: few distinct values, so the cancelling runs are long
            half = np.ascontiguousarray(half[np.random.default_rng(seed).integers(0, min(h, 5), size=h)])
        s = np.zeros((n, 4), dtype=np.uint64)
        k = k.copy()
        if scalar_kind == "cancel":
            s[0:2 * h:2], s[1:2 * h:2] = half, half
            k[1:2 * h:2] = -k[0:2 * h:2]
        else:
            s[:h], s[h:2 * h] = half, half
            k[h:2 * h] = -k[:h]
    else:
        raise ValueError(scalar_kind)
    return limbs_of_dlogs(k), k, np.ascontiguousarray(s)


def dlog_sum(s, k):
    """sum_i s_i * k_i mod r from the raw limbs (Python integers; vectorised per dlog value, 32 bits at a time)"""
    s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
    k = np.asarray(k, dtype=np.int64)
    assert len(s) == len(k) < (1 << 31)
    total = 0
    for kv in np.unique(k):
        if kv == 0:
            continue
        rows = s[k == kv]
        lo, hi = (rows & np.uint64(0xFFFFFFFF)).sum(axis=0), (rows >> np.uint64(32)).sum(axis=0)
        total += int(kv) * sum((int(lo[j]) + (int(hi[j]) << 32)) << (64 * j) for j in range(4))
    return total * _RINV % R   # the limbs are Montgomery residues


class Expected:
    """both references of one case: the C oracle's affine limbs and the closed form's point; they must agree with each other too"""

    def __init__(self, bases, k, s, threads, base=P0, count=None):
        n = len(s) if count is None else count
        self.limbs = CO.best_multiexp(s[:n], bases[:n], threads=threads)
        total = dlog_sum(s[:n], k[:n])
        self.point = O.g1_mul(base, total) if total else None
        assert self.point == O.g1_mul_complete(base, total)          # two independent G1 implementations
        assert O.limbs_to_points(self.limbs) == [self.point]         # the oracle's MSM and the closed form
        self.is_identity = total == 0

    def check(self, got, tag, point_format=H.POINT_AFFINE):
        if point_format == H.POINT_AFFINE:
            assert np.array_equal(np.asarray(got).reshape(1, 8), self.limbs), tag
            assert O.limbs_to_points(got) == [self.point], tag
        else:
            assert jac_to_affine_ints(np.asarray(got)) == self.point, tag


# ------------------------------------------------------------------------------------------------------------------------ 1. single MSMs
def check_msm_paths(ctx, sizes, threads, seed=0, thin=1):
    """ctx.msm (affine and Jacobian) and ctx.msm_dev over plain and precomputed bases, each made under msm_table_split 0 and 1 (table building
    over identity, duplicate and negated bases), for the base sets x scalar kinds at every size.  thin = 1: every case under all four
    (split, flags) combinations at every size.  thin = t > 1 (the emulated build, where a call costs a fixed ~0.1 s): at a size only every t-th
    case, under ONE combination; the offsets rotate with the size, so that over the sizes every case and every combination comes up.  A case that
    is run is always held against both references.  Returns the number of cases run."""
    cases = 0
    todo = [(M, sk) for M in (1, 6) for sk in SCALAR_KINDS]
    todo += [(bk, sk) for bk in FIXED_SETS for sk in (("rand", "few", "cancel") if bk == "alternating" else ("rand", "few"))]
    combos = [(split, flags) for split in (0, 1) for flags in (BASES_PLAIN, BASES_PRECOMPUTE)]
    for ni, n in enumerate(sizes):
        for ci, (bk, sk) in enumerate(todo):
            if (ci + ni) % thin:
                continue
            bases, k, s = make_case(n, bk, sk, seed + 97 * ni + ci)
            exp = Expected(bases, k, s, threads)
            if sk.startswith("cancel") or bk == "identity":
                assert exp.is_identity, (n, bk, sk)
            ds = ctx.to_device(s)
            try:
                for split, flags in (combos if thin == 1 else [combos[((ci + ni) // thin) % 4]]):
                    tag = (n, bk, sk, split, flags)
                    with knobs(ctx, msm_table_split=split):
                        b = ctx.bases_upload(bases, flags)
                    try:
                        exp.check(ctx.msm(b, s, H.POINT_AFFINE), tag)
                        if (split + flags + ci) % 2:   # the other entry points on half of the combinations each
                            exp.check(ctx.msm(b, s, H.POINT_JACOBIAN), tag, H.POINT_JACOBIAN)
                            exp.check(ctx.msm_dev(b, ds, n, H.POINT_AFFINE), tag)
                        else:
                            exp.check(ctx.msm_dev(b, ds, n, H.POINT_JACOBIAN), tag, H.POINT_JACOBIAN)
                    finally:
                        b.free()
            finally:
                ctx.free(ds)
            cases += 1
    return cases


def check_msm_large(ctx, n, threads, combos, seed=0):
    """(GPU sizes) the given (base kind, scalar kind) pairs at one large n, plain and precomputed bases, msm and msm_dev"""
    for ci, (bk, sk) in enumerate(combos):
        bases, k, s = make_case(n, bk, sk, seed + ci)
        exp = Expected(bases, k, s, threads)
        ds = ctx.to_device(s)
        try:
            for flags in (BASES_PLAIN, BASES_PRECOMPUTE):
                b = ctx.bases_upload(bases, flags)
                try:
                    exp.check(ctx.msm(b, s, H.POINT_AFFINE), (n, bk, sk, flags))
                    exp.check(ctx.msm_dev(b, ds, n, H.POINT_JACOBIAN), (n, bk, sk, flags), H.POINT_JACOBIAN)
                finally:
                    b.free()
        finally:
            ctx.free(ds)
    return len(combos)


def check_prefix_of_bases(ctx, n, threads):
    """fewer scalars than bases: the MSM over a prefix of a degenerate set (plain and precomputed), incl. n = 0"""
    bases, k, s = make_case(n, 6, "few", 5)
    for flags in (BASES_PLAIN, BASES_PRECOMPUTE):
        b = ctx.bases_upload(bases, flags)
        try:
            for m in (0, 1, n // 3, n - 1):
                Expected(bases, k, s, threads, count=m).check(ctx.msm(b, s[:m], H.POINT_AFFINE), (n, m, flags))
        finally:
            b.free()


# ------------------------------------------------------------------------------------------------------------------------- 2. batch paths
FUSE_DEFER = ((0, 1), (1, 1), (1, 0), (3, 1), (3, 0))


def check_msm_batch(ctx, n, threads, base_kind=6, seed=0):
    """msm_batch (host columns) and msm_batch_dev under every (msm_fuse_cols, msm_defer_reduce) setting, columns of DIFFERENT kinds in one call:
    a cancelling column next to a uniform one, then a column of zeros, then long runs, then a late-cancelling one — a stale or unzeroed
    deferred bucket buffer shows in the column behind it.  The cancelling columns need opposite partners in the SHARED base set: the set holds
    the opposite of entry i both next to it and h = 2 * (n // 4) entries away; every other column is an ordinary column over it."""
    h = (n // 4) * 2
    k = small_dlog_bases(n, base_kind, seed + 1)[1]
    k[1:h:2] = -k[0:h:2]        # opposite neighbours ...
    k[h:2 * h] = -k[:h]         # ... and the opposite of entry i again at i + h
    bases = limbs_of_dlogs(k)
    c_cancel, late = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    v = full_range_fr(h, seed + 2, edges=False)
    c_cancel[0:2 * h:2], c_cancel[1:2 * h:2] = v, v             # cancels between neighbours
    late[:h], late[h:2 * h] = v[::-1], v[::-1]                  # cancels between entries h apart
    few = full_range_fr(3, seed + 4, edges=False)[np.random.default_rng(seed).integers(0, 3, size=n)]
    cols = [c_cancel, rand_fr(n, seed + 3), np.zeros((n, 4), dtype=np.uint64), np.ascontiguousarray(few), late, circuit_like_fr(n, seed + 6)]
    exps = [Expected(bases, k, c, threads) for c in cols]
    assert exps[0].is_identity and exps[2].is_identity and exps[4].is_identity
    dptrs = [ctx.to_device(c) for c in cols]
    bs = {f: ctx.bases_upload(bases, f) for f in (BASES_PLAIN, BASES_PRECOMPUTE)}
    try:
        for fuse, defer in FUSE_DEFER:
            for flags, b in bs.items():
                tag = (n, fuse, defer, flags)
                with knobs(ctx, msm_fuse_cols=fuse, msm_defer_reduce=defer):
                    got = ctx.msm_batch_dev(b, dptrs, n, H.POINT_AFFINE)
                    goth = ctx.msm_batch(b, cols[:3], H.POINT_JACOBIAN)   # host columns: cancelling, uniform, zeros
                for j, e in enumerate(exps):
                    e.check(got[j:j + 1], tag + (j,))
                for j, e in enumerate(exps[:3]):
                    e.check(goth[j], tag + (j, "host"), H.POINT_JACOBIAN)
    finally:
        for d in dptrs:
            ctx.free(d)
        for b in bs.values():
            b.free()
    return len(FUSE_DEFER) * 2


def check_msm_multi(ctx, n, threads, seed=0):
    """msm_multi_dev over two DIFFERENT degenerate base sets in one call (M = 1 with cancelling neighbours, M = 6), per-column and fused"""
    bases_a, ka, cancel_a = make_case(n, 1, "cancel", seed + 11)
    bases_b, kb, late_b = make_case(n, 6, "cancel_late", seed + 12)
    cols = [cancel_a, late_b, rand_fr(n, seed + 13), np.zeros((n, 4), dtype=np.uint64), make_case(n, 1, "few", seed + 14)[2]]
    want_a = [Expected(bases_a, ka, c, threads) for c in cols]
    want_b = [Expected(bases_b, kb, c, threads) for c in cols]
    assert want_a[0].is_identity and want_b[1].is_identity
    dptrs = [ctx.to_device(c) for c in cols]
    with knobs(ctx, msm_window_bits=6):   # (the sets of one call must share their table layout)
        ba, bb = ctx.bases_upload(bases_a, BASES_PRECOMPUTE), ctx.bases_upload(bases_b, BASES_PRECOMPUTE)
    pa, pb = ctx.bases_upload(bases_a), ctx.bases_upload(bases_b)
    try:
        for (sa, sb) in ((ba, bb), (pa, pb)):
            sets = [sa, sb, sb, sa, sb, sa, sa]
            ptrs = [dptrs[j % 5] for j in range(len(sets))]
            for fuse, defer in (FUSE_DEFER if sa is ba else FUSE_DEFER[:3]):
                with knobs(ctx, msm_fuse_cols=fuse, msm_defer_reduce=defer):
                    got = ctx.msm_multi_dev(sets, ptrs, n, H.POINT_AFFINE)
                for j, st in enumerate(sets):
                    (want_a if st is sa else want_b)[j % 5].check(got[j:j + 1], (n, fuse, defer, j, sa is ba))
    finally:
        for d in dptrs:
            ctx.free(d)
        for b in (ba, bb, pa, pb):
            b.free()


def check_dense_then_cancelling(ctx, n, threads, seed=0):
    """two consecutive MSMs on one context over one base set: a dense one, then a cancelling one, which must be the identity — bucket
    storage that is not zeroed again shows.  Single MSMs, then the batch paths with the dense column in an earlier CALL."""
    bases, k, cancel = make_case(n, 6, "cancel", seed + 21)
    late = np.zeros((n, 4), dtype=np.uint64)
    h = n // 2
    late[0:2 * h:2] = late[1:2 * h:2] = full_range_fr(1, seed + 22, edges=False)   # one scalar everywhere: ONE bucket per window, cancelling across all lanes
    dense = rand_fr(n, seed + 23)
    e_dense, e_cancel, e_late = (Expected(bases, k, c, threads) for c in (dense, cancel, late))
    assert e_cancel.is_identity and e_late.is_identity and not e_dense.is_identity
    dd, dc, dl = (ctx.to_device(c) for c in (dense, cancel, late))
    try:
        for flags in (BASES_PLAIN, BASES_PRECOMPUTE):
            b = ctx.bases_upload(bases, flags)
            try:
                for quad in (1, 0):
                    with knobs(ctx, msm_quad_tails=quad):
                        e_dense.check(ctx.msm(b, dense), (n, flags, quad, "dense"))
                        e_cancel.check(ctx.msm(b, cancel), (n, flags, quad, "cancel after dense"))
                        e_dense.check(ctx.msm_dev(b, dd, n, H.POINT_AFFINE), (n, flags, quad, "dense"))
                        e_late.check(ctx.msm_dev(b, dl, n, H.POINT_AFFINE), (n, flags, quad, "one-bucket cancel after dense"))
                for fuse, defer in FUSE_DEFER:
                    with knobs(ctx, msm_fuse_cols=fuse, msm_defer_reduce=defer):
                        got = ctx.msm_batch_dev(b, [dd, dd, dd], n, H.POINT_AFFINE)
                        got2 = ctx.msm_batch_dev(b, [dc, dl, dc], n, H.POINT_AFFINE)
                    for j in range(3):
                        e_dense.check(got[j:j + 1], (n, flags, fuse, defer, j))
                        (e_late if j == 1 else e_cancel).check(got2[j:j + 1], (n, flags, fuse, defer, j, "after dense"))
            finally:
                b.free()
    finally:
        for d in (dd, dc, dl):
            ctx.free(d)


# ------------------------------------------------------------------------------------------------------------------------------ 3. knobs
def _knob_cases(n, seed):
    out = []
    for i, (bk, sk) in enumerate(((6, "few"), (6, "cancel"), (1, "cancel_late"), (1, "rand"), ("equal", "few"), ("alternating", "cancel"), (6, "full_range"))):
        out.append(((bk, sk),) + make_case(n, bk, sk, seed + 31 + i))
    return out


def check_msm_knobs(ctx, n, threads, windows=(4, 7, 12), exact_cases=None, seed=0):
    """the knobs that change which kernel finishes the job, over degenerate cases (plain and precomputed bases): the window size; entries per
    lane small enough that one run spans several lanes and several waves (msm_chunk_lone for a lone MSM, msm_chunk for the batch lanes);
    the reduction's segment length; serial tails and quad tails (quad29.cuh: a second implementation with its own exceptional branches) on
    both sides of msm_quad_seg_max; histogram sub-ranges and sort chunk counts.  Only values from the knobs' legal domains."""
    cases = _knob_cases(n, seed)[:exact_cases]
    settings = [dict(msm_window_bits=c) for c in windows]
    settings += [dict(msm_chunk_lone=v) for v in (1, 2, 7, 4096)]
    settings += [dict(msm_chunk=v) for v in (2, 3, 4096)]
    settings += [dict(msm_seg=v, msm_window_bits=8) for v in (1, 2, 64, 1024)]
    settings += [dict(msm_quad_tails=0), dict(msm_quad_tails=0, msm_window_bits=5), dict(msm_quad_tails=1, msm_quad_seg_max=0),
                 dict(msm_quad_tails=1, msm_quad_seg_max=(1 << 31) - 1), dict(msm_quad_tails=1, msm_quad_seg_max=(1 << 31) - 1, msm_window_bits=5),
                 dict(msm_quad_tails=1, msm_quad_seg_max=(1 << 31) - 1, msm_seg=1, msm_window_bits=9)]
    settings += [dict(msm_hist_split=v) for v in (1, 2, 64)]
    settings += [dict(msm_sort_groups=v) for v in (1, 2, 33, 1024)]
    settings += [dict(msm_chunk_lone=1, msm_window_bits=4, msm_quad_tails=0), dict(msm_chunk=2, msm_window_bits=max(windows), msm_sort_groups=2)]
    runs = 0
    for (bk, sk), bases, k, s in cases:
        exp = Expected(bases, k, s, threads)
        ds = ctx.to_device(s)
        bs = {}
        try:
            for flags in (BASES_PLAIN, BASES_PRECOMPUTE):
                bs[flags] = ctx.bases_upload(bases, flags)
            for i, kv in enumerate(settings):
                # a precomputed table is laid out for the window it was made under: other windows go to the plain set, and so does every other
                # second setting
                flags = BASES_PLAIN if ("msm_window_bits" in kv or i % 2) else BASES_PRECOMPUTE
                with knobs(ctx, **kv):
                    exp.check(ctx.msm(bs[flags], s), (n, bk, sk, kv, flags))
                    if "msm_chunk" in kv:   # the batch lanes read msm_chunk
                        got = ctx.msm_batch_dev(bs[flags], [ds, ds], n, H.POINT_AFFINE)
                        exp.check(got[0:1], (n, bk, sk, kv, flags, "batch 0"))
                        exp.check(got[1:2], (n, bk, sk, kv, flags, "batch 1"))
                runs += 1
            for c in windows:   # precomputed tables made UNDER each window, used with the tails both ways
                with knobs(ctx, msm_window_bits=c):
                    b = ctx.bases_upload(bases, BASES_PRECOMPUTE)
                    try:
                        for quad in (1, 0):
                            with knobs(ctx, msm_quad_tails=quad, msm_chunk_lone=2):
                                exp.check(ctx.msm(b, s), (n, bk, sk, c, quad, "table"))
                            runs += 1
                    finally:
                        b.free()
        finally:
            ctx.free(ds)
            for b in bs.values():
                b.free()
    return runs


# --------------------------------------------------------------------------------------------------------------------------------- 4. G2
def _g2():
    from oracle import pairing as PR

    return PR


_G2_CACHE = {}


def _g2_table():
    if not _G2_CACHE:
        PR = _g2()
        q0 = PR.g2_mul(PR.G2_GEN, 0xDEADBEEF)
        pts = _signed_multiples(PR.g2_mul, PR.g2_neg, q0, MMAX)
        vals = []
        for p in pts:
            vals += [0, 0, 0, 0] if p is None else [p[0][0], p[0][1], p[1][0], p[1][1]]
        _G2_CACHE["q0"] = q0
        _G2_CACHE["limbs"] = O.ints_to_limbs(vals, Q).reshape(-1, 16)
    return _G2_CACHE["q0"], _G2_CACHE["limbs"]


def check_msm_g2(ctx, sizes, seed=0):
    """ctx.msm_g2 over small multiples of a fixed G2 point: all identity, all equal, alternating +-Q, random dlogs from {-1, 0, 1} and {-6 .. 6},
    with uniform, few, pairwise cancelling and late cancelling scalars.  Reference: ONE scalar multiplication (sum_i s_i * k_i) * Q with
    oracle/pairing.py's affine G2 arithmetic — the cost does not grow with n, so the sizes are bounded by the kernels' time, not the reference's."""
    PR = _g2()
    q0, table = _g2_table()
    cases = 0
    for ni, n in enumerate(sizes):
        todo = [("identity", "rand"), ("equal", "rand"), ("equal", "few"), ("alternating", "rand"), ("alternating", "cancel"), (1, "few"),
                (1, "cancel"), (6, "rand"), (6, "few"), (6, "cancel"), (6, "cancel_late"), ("first", "rand"), ("last", "full_range")]
        for ci, (bk, sk) in enumerate(todo):
            _, k, s = make_case(n, bk, sk, seed + 41 * ni + ci)
            total = dlog_sum(s, k)
            want = PR.g2_mul(q0, total) if total else None
            if sk.startswith("cancel") or bk == "identity":
                assert want is None
            got = ctx.msm_g2(np.ascontiguousarray(table[k + MMAX]), s)
            v = O.limbs_to_ints(got.reshape(-1, 4), Q)
            assert (None if not any(v) else ((v[0], v[1]), (v[2], v[3]))) == want, (n, bk, sk)
            cases += 1
    return cases


# -------------------------------------------------------------------------------------------------------------------- 5. g1_to_lagrange
LAGRANGE_KINDS = ("equal", "one_hot", "alternating", "omega_powers", "small", "s_powers")


def lagrange_dlogs(kind, k, seed=0):
    n = 1 << k
    if kind == "equal":          # one point followed by identities; every butterfly hits P + P and P - P
        return [5] * n
    if kind == "one_hot":
        return [1] + [0] * (n - 1)
    if kind == "alternating":
        return [1 if i % 2 == 0 else R - 1 for i in range(n)]
    if kind == "omega_powers":   # a_i = omega^i: one-hot result, every other output cancels to the identity in the last stage
        w = O.omega_for(k)
        return [pow(w, i, R) for i in range(n)]
    if kind == "small":
        return [int(v) % R for v in np.random.default_rng([seed, k]).integers(-6, 7, size=n)]
    if kind == "s_powers":       # the well-formed SRS shape: the control
        sv = 0x1D0C0FFEE + k
        return [pow(sv, i, R) for i in range(n)]
    raise ValueError(kind)


def check_g1_to_lagrange(ctx, ks, threads, kinds=LAGRANGE_KINDS):
    """the EC FFT behind g1_to_lagrange on degenerate SRS-shaped input g_i = a_i * P0: every output point against (iNTT(a))_j * P0 (scalar
    inverse transform: the C oracle's, with domain_consts(k)'s omega and 2^-k; point multiplication: O.g1_mul), for both flags; then the
    returned set in an MSM against the oracle and the closed form."""
    mul_cache = {0: None}

    def mul(v):
        if v not in mul_cache:
            mul_cache[v] = O.g1_mul(P0, v)
        return mul_cache[v]

    for k in ks:
        n = 1 << k
        w, _, div = domain_consts(k)
        for kind in kinds:
            a = lagrange_dlogs(kind, k)
            b = O.limbs_to_ints(CO.ifft(fr(a), k, w, threads=threads), R)
            if kind == "equal":
                assert b == [5] + [0] * (n - 1)
            if kind == "one_hot":
                assert len(set(b)) == 1 and b[0] == O.limbs_to_ints(div, R)[0]
            if kind == "omega_powers" and k >= 1:
                assert b == [0, 1] + [0] * (n - 2)
            g_limbs = O.points_to_limbs([mul(v) for v in a])
            want = O.points_to_limbs([mul(v) for v in b])
            s = full_range_fr(n, 50 + k)
            total = sum(x * y for x, y in zip(O.limbs_to_ints(s, R), b)) % R
            want_pt = O.g1_mul(P0, total) if total else None
            assert want_pt == O.g1_mul_complete(P0, total)
            for flags in (BASES_PLAIN, BASES_PRECOMPUTE):
                g = ctx.bases_upload(g_limbs, flags)
                lg = None
                try:
                    lg = ctx.g1_to_lagrange(g, k, flags)
                    got = ctx.bases_download(lg)
                    assert np.array_equal(got, want), (k, kind, flags, [j for j in range(n) if not np.array_equal(got[j], want[j])][:8])
                    res = ctx.msm(lg, s, H.POINT_AFFINE)
                    assert np.array_equal(res, CO.best_multiexp(s, got, threads=threads)), (k, kind, flags)
                    assert O.limbs_to_points(res) == [want_pt], (k, kind, flags)
                finally:
                    g.free()
                    if lg is not None:
                        lg.free()


# ------------------------------------------------------------------------------------------------------- 6. point sums, fixed-base products
def _jacobian_limbs(ks, seed):
    """k_i * P0 as Jacobian (X, Y, Z) = (x z^2, y z^3, z) with a random z per point (every fourth: z = 1); the identity as Z = 0 with
    X, Y alternately zero and non-zero"""
    g = np.random.default_rng(seed)
    vals = []
    for i, kk in enumerate(ks):
        p = _G1_POINTS[kk + MMAX]
        if p is None:
            vals += [0, 0, 0] if i % 2 else [P0[0], P0[1], 0]
            continue
        z = 1 if i % 4 == 0 else int(g.integers(2, 1 << 62)) ** 4 % Q
        vals += [p[0] * z * z % Q, p[1] * z * z * z % Q, z]
    return O.ints_to_limbs(vals, Q).reshape(-1, 12)


def check_g1_sum_jacobian(ctx):
    """g1_sum_jacobian_dev (64 lanes, lane l sums entries l, l + 64, ...; then a tree over the lanes) in both point formats: identities at the
    ends and in the middle, equal and opposite neighbours at the strides the kernel adds over (1, 32, 64), lists that sum to the identity,
    n = 0 and n = 1"""
    rng = np.random.default_rng(7)
    lists = [[], [3], [0], [0, 2, 0, 0, -5, 0], [2, 2], [2, -2], [4, 4, 4, 4, -4, -4, -4, -4], [1] * 64, [1] * 65 + [-1] * 65, [1, -1] * 70,
             [3] * 128, [3] * 64 + [-3] * 64, [0] * 63 + [6], [6] + [0] * 200, [2] * 32 + [-2] * 32, [0] * 130]
    lists += [[int(v) for v in rng.integers(-6, 7, size=m)] for m in (5, 63, 64, 65, 129, 700)]
    sym = [int(v) for v in rng.integers(-6, 7, size=150)]
    lists += [sym + [-v for v in sym], sym + [-v for v in reversed(sym)]]
    for li, ks in enumerate(lists):
        want = O.g1_mul(P0, sum(ks) % R) if sum(ks) % R else None
        assert want == O.g1_mul_complete(P0, sum(ks) % R)
        pts = _jacobian_limbs(ks, li)
        d = ctx.to_device(pts) if len(ks) else 0
        try:
            assert O.limbs_to_points(ctx.g1_sum_jacobian_dev(d, len(ks), H.POINT_AFFINE)) == [want], (li, ks[:8])
            assert jac_to_affine_ints(ctx.g1_sum_jacobian_dev(d, len(ks), H.POINT_JACOBIAN)) == want, (li, ks[:8])
        finally:
            if d:
                ctx.free(d)
    return len(lists)


def check_g1_fixed_base_mul(ctx, threads=4):
    """g1_fixed_base_mul on the scalars 0, 1, r - 1, 2^252 (as field elements), every edge limb pattern, and a batch in which every scalar is
    0 — against the C oracle's fixed-base products bit for bit and O.g1_mul per scalar"""
    base = O.points_to_limbs([P0])
    batches = [np.concatenate([fr([0, 1, R - 1, 1 << 252, 2, R - 2, (R - 1) // 2, (R + 1) // 2]), _raw_limbs(edge_fr_values()), full_range_fr(40, 3)]),
               np.zeros((70, 4), dtype=np.uint64), fr([0]), fr([R - 1])]
    for bi, s in enumerate(batches):
        got = ctx.g1_fixed_base_mul(base, s)
        assert np.array_equal(got, CO.g1_fixed_base_batch(base, s, threads=threads)), bi
        assert O.limbs_to_points(got) == [O.g1_mul(P0, v) if v else None for v in O.limbs_to_ints(s, R)], bi
    assert not ctx.g1_fixed_base_mul(base, batches[1]).any()
    return len(batches)
