"""Every pass plan of `ntt_run_batch` (halo2-lib_amd/csrc/ntt.hip) and every branch of the tile kernel's first pass, run as stand-alone transforms:
the driver picks, per pass, between `ntt_pass_kernel` and `ntt_tile_kernel<KIND, MUL>`, and the tile kernel's first pass between the general
butterflies and the `quarter` short cut in its even-m form (the first radix-4 round is a copy of x0 over LDS rows that were never filled) and its
odd-m form (a radix-2 copy, then the `zeros == 2` round).  Which of them runs depends on log_n, in_len, the knobs and on whether a direct twiddle
table exists; `plan` restates that decision, `check_cases_reach_their_branches` ties the case lists below to it, and the checks compare each case
bit for bit with the C oracle on inputs uniform over [0, r) with the edge patterns planted (tests.util.full_range_fr, turned so that
position 0 is not zero: `column`).

Shared by the emulated build (tests/test_ntt_plans.py) and the GPU (tests/test_ntt_plans_gpu.py).  GPU only: the 2^19 and 2^22 extensions, the
transforms above 2^17 and the `ntt_min_col_bits = 5` plan at 2^22 — the one plan here whose middle pass has more than 2^16 twiddles, hence no direct
table, and runs the generic kernel on the unreduced scratch a tile pass left.  The emulator takes longer for a 2^22 case than the slowest case of
tests/test_product_scans.py, the bound for an emulated case; the generic kernel behind a tile pass is reached on the emulator by the 2^11 and 2^12
knob plans (there with a direct table)."""
import functools

import numpy as np

from oracle import bn254 as O
from oracle import c_oracle as CO
from tests.knob_checks import knobs
from tests.util import R, domain_consts, fr, full_range_fr

NTT_BATCH = 32   # columns per launch group (ntt.hip)


# --------------------------------------------------------------------------------------------------------------------------------- the plan
def plan(log_n, in_len=None, in_scale=False, out_scale=False, tile_bits=10, min_col_bits=2, full_table=1, tile_kernel=1):
    """What `ntt_run_batch` launches for one column of 2^log_n elements, pass by pass: a list of dicts with m, cb, log_s, `direct` (a direct
    twiddle table exists, by the rule of get_direct_table: never for the last pass, which has no inter-pass twiddles), `kernel` ("tile" or
    "generic") and, for the tile kernel, `kind`, `mul`, `quarter` and `m_odd`.  It produces no expected value.  It assumes a free direct-table slot
    (a twiddle set has four; the plans used here need at most three per set, and at most four together with the default plan of the same size)."""
    N = 1 << log_n
    if in_len is None:
        in_len = N
    lt = tile_bits
    if log_n <= lt:
        ms = [log_n]
    else:
        mcb = min_col_bits if min_col_bits < lt else lt - 1
        maxm = lt - mcb
        P = (log_n + maxm - 1) // maxm
        ms = [log_n // P + (1 if i < log_n % P else 0) for i in range(P)]
    P = len(ms)
    passes, log_s = [], 0
    for i, m in enumerate(ms):
        first, last = i == 0, i == P - 1
        cb = min(lt - m, log_n - m)
        if i > 0:
            cb = min(cb, log_s)
        direct = False
        if not last:
            bits = log_n - log_s
            direct = not ((log_s != 0 and bits > 16) or (log_s == 0 and (bits > 23 or not full_table)))
        p = dict(m=m, cb=cb, log_s=log_s, direct=direct, first=first, last=last, in_len=in_len if first else N, n=N)
        if tile_kernel and P >= 2 and lt == 10 and m + cb == 10 and m >= 2 and (last or direct):
            p.update(kernel="tile", kind=0 if first else (2 if last else 1), mul=bool(in_scale) if first else bool(last and out_scale),
                     quarter=first and in_len <= (N >> 2) and log_n >= 2, m_odd=bool(m & 1))
        else:
            p.update(kernel="generic", in_mul=bool(first and in_scale), out_mul=bool(last and out_scale))
        passes.append(p)
        log_s += m
    assert log_s == log_n
    return passes


def classes_of(passes):
    """the branch classes (strings) that one transform's passes reach"""
    out = set()
    for i, p in enumerate(passes):
        if p["kernel"] == "tile":
            if p["kind"] == 0:
                if p["quarter"]:
                    out.add("first tile pass: quarter, %s m" % ("odd" if p["m_odd"] else "even"))
                elif 2 * p["in_len"] == p["n"]:
                    out.add("first tile pass: in_len = N/2")
                elif p["in_len"] == p["n"]:
                    out.add("first tile pass: in_len = N, %s" % ("MUL" if p["mul"] else "no MUL"))
            elif p["kind"] == 1:
                out.add("tile pass KIND 1")
            else:
                out.add("tile pass KIND 2, %s" % ("MUL" if p["mul"] else "no MUL"))
                out.add("tile pass KIND 2, m = %d" % p["m"])
        else:
            if len(passes) == 1 and p["in_len"] < p["n"] and p["in_len"]:
                out.add("generic only pass, factor %d" % (p["n"] // p["in_len"]))
            if 0 < i < len(passes) - 1 and passes[i - 1]["kernel"] == "tile":
                out.add("generic middle pass behind a tile pass")
                if not p["direct"]:
                    out.add("generic middle pass behind a tile pass, no direct table")
    return out


def launch_groups(ncols):
    return [min(NTT_BATCH, ncols - c0) for c0 in range(0, ncols, NTT_BATCH)]


# -------------------------------------------------------------------------------------------------------------------------------- the cases
TRANSFORMS_GPU = (12, 13, 15, 17, 18, 21, 23)
TRANSFORMS_EMU = (12, 13, 15, 17)

EXTENSIONS_GPU = (
    # even m in the first pass, `quarter` (factors 4, 8, 16)
    (10, 12), (9, 12), (8, 12), (14, 16), (13, 16), (12, 16), (15, 17),
    # ... at the benchmark's shape
    (20, 22), (19, 22),
    # odd m, factors 8 and 16
    (10, 13), (9, 13), (16, 19),
    # half the rows zero (`quarter` off): even m, odd m, three passes
    (11, 12), (12, 13), (16, 17),
    # out of place with k = ext_k: the scaling, no padding
    (12, 12), (13, 13),
    # a single pass: the generic kernel with in_len < N
    (3, 4), (2, 5), (0, 4), (6, 10), (9, 10),
)
EXTENSIONS_EMU = tuple(c for c in EXTENSIONS_GPU if c[1] < 19)

BATCH_COLUMNS = 33        # a launch group of 32 columns and one of 1
BATCH_EXTENSION = (10, 12)
BATCH_IFFT = 12

# (knobs, log_n of the forward and inverse transform, (k, ext_k) of the extension)
KNOB_PLANS_EMU = (
    (dict(ntt_min_col_bits=5), 11, (9, 11)),    # passes 4, 4, 3: tile, generic, tile with m = 3 (the "only round" exit)
    (dict(ntt_min_col_bits=5), 12, (10, 12)),   # passes 4, 4, 4: tile, generic, tile with m = 4
)
KNOB_PLANS_GPU = KNOB_PLANS_EMU + (
    (dict(ntt_min_col_bits=5, ntt_full_table=1), 22, (20, 22)),   # passes 5, 5, 4, 4, 4: tile, generic (2^17 twiddles: no table), tile, tile, tile
    (dict(ntt_min_col_bits=5, ntt_full_table=0), 22, (20, 22)),   # ... and the first pass generic too
)


def knob_id(case):
    kn, log_n, _ = case
    return "-".join(["2^%d" % log_n] + ["%s=%d" % (n[4:], v) for n, v in sorted(kn.items())])


def _plan_kwargs(kn):
    names = dict(ntt_min_col_bits="min_col_bits", ntt_full_table="full_table", ntt_tile_bits="tile_bits", ntt_tile_kernel="tile_kernel")
    return {names[n]: v for n, v in kn.items()}


def case_plans(transforms, extensions, knob_plans):
    """the plan of every transform the checks below run for these case lists"""
    out = []
    for log_n in transforms:
        out += [plan(log_n), plan(log_n, out_scale=True)]
    for k, ek in extensions + (BATCH_EXTENSION,):
        out += [plan(ek, in_len=1 << k, in_scale=True), plan(ek, out_scale=True)]
    out.append(plan(BATCH_IFFT, out_scale=True))
    for kn, log_n, (k, ek) in knob_plans:
        kw = _plan_kwargs(kn)
        out += [plan(log_n, **kw), plan(log_n, out_scale=True, **kw), plan(ek, in_len=1 << k, in_scale=True, **kw), plan(ek, out_scale=True, **kw)]
    return out


CLASSES_BOTH = frozenset(
    ["first tile pass: quarter, even m", "first tile pass: quarter, odd m", "first tile pass: in_len = N/2", "first tile pass: in_len = N, MUL",
     "first tile pass: in_len = N, no MUL", "tile pass KIND 1", "tile pass KIND 2, MUL", "tile pass KIND 2, no MUL"]
    + ["tile pass KIND 2, m = %d" % m for m in (3, 4, 5, 6, 7, 8)]
    + ["generic only pass, factor %d" % f for f in (2, 8, 16)]
    + ["generic middle pass behind a tile pass"])
CLASSES_GPU = CLASSES_BOTH | {"generic middle pass behind a tile pass, no direct table"}


def check_cases_reach_their_branches():
    """The case lists reach every class of pass the driver can launch (no kernel runs): once for the GPU lists, once for the emulated lists with
    the classes those claim.  `plan` is a restatement of ntt_run_batch's planning and of get_direct_table's rule that is checked against the driver
    only by reading: whoever changes the plan in ntt.hip changes `plan` with it, and this test then says which cases to revisit."""
    for name, (transforms, extensions, knob_plans), want in (("gpu", (TRANSFORMS_GPU, EXTENSIONS_GPU, KNOB_PLANS_GPU), CLASSES_GPU),
                                                            ("emulated", (TRANSFORMS_EMU, EXTENSIONS_EMU, KNOB_PLANS_EMU), CLASSES_BOTH)):
        got = set()
        for p in case_plans(transforms, extensions, knob_plans):
            got |= classes_of(p)
        assert not want - got, (name, sorted(want - got))
    assert launch_groups(BATCH_COLUMNS) == [32, 1]
    # the batched cases themselves: an even-m `quarter` first pass, and a two-pass inverse
    assert "first tile pass: quarter, even m" in classes_of(plan(BATCH_EXTENSION[1], in_len=1 << BATCH_EXTENSION[0], in_scale=True))
    assert "tile pass KIND 2, MUL" in classes_of(plan(BATCH_IFFT, out_scale=True))
    # the plans the comments above name
    kernels = lambda ps: [(p["kernel"], p["m"]) for p in ps]
    assert kernels(plan(11, min_col_bits=5)) == [("tile", 4), ("generic", 4), ("tile", 3)]
    assert kernels(plan(12, min_col_bits=5)) == [("tile", 4), ("generic", 4), ("tile", 4)]
    assert kernels(plan(22, min_col_bits=5)) == [("tile", 5), ("generic", 5), ("tile", 4), ("tile", 4), ("tile", 4)]
    assert [p["direct"] for p in plan(22, min_col_bits=5)] == [True, False, True, True, False]
    assert kernels(plan(22, min_col_bits=5, full_table=0))[:2] == [("generic", 5), ("generic", 5)]
    assert kernels(plan(17)) == [("tile", 6), ("tile", 6), ("tile", 5)]
    assert [p["m"] for p in plan(22, in_len=1 << 20, in_scale=True)] == [8, 7, 7]   # the benchmark's k = 20


# ------------------------------------------------------------------------------------------------------------------------------- the checks
ZETA, ZETA_INV = fr([O.ZETA]), fr([O.ZETA * O.ZETA % R])   # zeta^3 = 1


def _frozen(a):
    a.setflags(write=False)
    return a


def column(n, seed):
    """full_range_fr turned by one place.  full_range_fr plants the edge pattern 0 at position 0, and the tile kernel's first pass loads x[0] for
    every padding row (a clamped address; the zero is selected at the fill): with a zero there, a fill that forgot the selection would still be
    right.  Turned, position 0 holds what full_range_fr put last (the pattern 1, or for n = 1 another non-zero pattern)."""
    a = np.ascontiguousarray(np.roll(full_range_fr(n, seed), 1, axis=0))
    assert a[0].any()
    return a


def _mismatch(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    return "%s: %d of %d elements differ, first at %d" % (what, len(bad), len(want), bad[0] if len(bad) else -1)


def assert_same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), _mismatch(got, want, what)


def check_forward(ctx, log_n, threads):
    a = column(1 << log_n, 1100 + log_n)
    w, _, _ = domain_consts(log_n)
    assert_same(ctx.best_fft(a, w, log_n), CO.best_fft(a, log_n, w, threads=threads), "best_fft 2^%d" % log_n)


def check_inverse(ctx, log_n, threads):
    a = column(1 << log_n, 1200 + log_n)
    w, winv, div = domain_consts(log_n)
    assert_same(ctx.ifft(a, winv, log_n, div), CO.ifft(a, log_n, w, threads=threads), "ifft 2^%d" % log_n)


def _extension_and_back(ctx, a, want_ext, want_back, k, ek):
    we, weinv, ediv = domain_consts(ek)
    ext = ctx.coeff_to_extended(a, k, ek, we, ZETA)
    assert_same(ext, want_ext, "coeff_to_extended %d -> %d" % (k, ek))
    back = ctx.extended_to_coeff(ext, ek, weinv, ediv, ZETA_INV)
    assert_same(back, want_back, "extended_to_coeff %d <- %d" % (k, ek))


def extension_reference(k, ek, threads, seed):
    """(coefficients, their extension, the extension taken back) by the oracle; the last is the coefficients followed by zeros"""
    a = column(1 << k, seed)
    we, _, _ = domain_consts(ek)
    ext = CO.coeff_to_extended(a, k, ek, we, ZETA, threads=threads)
    back = CO.extended_to_coeff(ext, ek, we, ZETA, threads=threads)
    assert np.array_equal(back[: 1 << k], a) and not back[1 << k:].any(), (k, ek)
    return _frozen(a), _frozen(ext), _frozen(back)


def check_extension(ctx, k, ek, threads):
    _extension_and_back(ctx, *extension_reference(k, ek, threads, 1300 + 32 * ek + k), k, ek)


def batch_columns(n, seed):
    """BATCH_COLUMNS distinct columns, one of them (in the first launch group) all zero"""
    cols = [column(n, seed + j) for j in range(BATCH_COLUMNS)]
    cols[7] = np.zeros((n, 4), dtype=np.uint64)
    return cols


def check_extension_batch(ctx, threads):
    """every column against the oracle's extension of that column: a column taken from, or written to, another column's buffer shows"""
    k, ek = BATCH_EXTENSION
    we, _, _ = domain_consts(ek)
    cols = batch_columns(1 << k, 1400)
    ins = [ctx.to_device(c) for c in cols]
    outs = [ctx.malloc(32 << ek) for _ in cols]
    try:
        ctx.coeff_to_extended_batch_dev(ins, k, outs, ek, we, ZETA)
        for j, (c, d, o) in enumerate(zip(cols, ins, outs)):
            assert_same(ctx.download(o, (1 << ek, 4)), CO.coeff_to_extended(c, k, ek, we, ZETA, threads=threads), "batched extension, column %d" % j)
            assert_same(ctx.download(d, c.shape), c, "batched extension, input column %d" % j)
    finally:
        for d in ins + outs:
            ctx.free(d)


def check_ifft_batch(ctx, threads):
    log_n = BATCH_IFFT
    w, winv, div = domain_consts(log_n)
    cols = batch_columns(1 << log_n, 1500)
    ds = [ctx.to_device(c) for c in cols]
    try:
        ctx.ifft_batch_dev(ds, winv, log_n, div)
        for j, (c, d) in enumerate(zip(cols, ds)):
            assert_same(ctx.download(d, c.shape), CO.ifft(c, log_n, w, threads=threads), "batched ifft, column %d" % j)
    finally:
        for d in ds:
            ctx.free(d)


@functools.lru_cache(maxsize=1)
def knob_reference(log_n, k, ek, threads):
    """inputs and oracle results of one knob case; they do not depend on the knobs, so the two 2^22 cases share them"""
    a, b = column(1 << log_n, 1600 + log_n), column(1 << log_n, 1700 + log_n)
    w, _, _ = domain_consts(log_n)
    fwd = CO.best_fft(a, log_n, w, threads=threads)
    inv = CO.ifft(b, log_n, w, threads=threads)
    return (_frozen(a), _frozen(fwd), _frozen(b), _frozen(inv)) + extension_reference(k, ek, threads, 1800 + ek)


def check_knob_plan(ctx, case, threads):
    """forward, inverse with the fused divisor, one extension and its way back under the knobs of `case`; the knobs come back in any case"""
    kn, log_n, (k, ek) = case
    a, fwd, b, inv, c, ext, back = knob_reference(log_n, k, ek, threads)
    w, winv, div = domain_consts(log_n)
    with knobs(ctx, **kn):
        assert_same(ctx.best_fft(a, w, log_n), fwd, "best_fft 2^%d under %s" % (log_n, kn))
        assert_same(ctx.ifft(b, winv, log_n, div), inv, "ifft 2^%d under %s" % (log_n, kn))
        _extension_and_back(ctx, c, ext, back, k, ek)
