"""What a context carries from one call to the next ("State a context keeps between calls"): the bucket arrays that are zero-filled
after use, the bounded twiddle cache and its direct-table slots, the pinned job ring, the resident Poseidon specs, the scratch slots and the
batch lanes.  Every check opens a context of its own (`make_ctx`), runs a SEQUENCE of calls on it and compares every result with an independent
reference — the C oracle, oracle/pairing.py, oracle/poseidon.py or the plain definition in Python integers — never with another call of the
library; every knob it changes comes back.  Shared by the emulated build (tests/test_context_state.py) and the GPU (tests/test_context_state_gpu.py).

A sequence reaches a branch only while a size relation holds ("fits the capacity the last call left", "forces a regrow", "more sets than the cache
holds").  No byte count is written down here: the MSM sizes come from the planners (csrc/msm_plan.h, through tests/emu/msm_plan_selftest.cpp),
the capacity from ws_reserve's 1 MiB granule, the G2 array from g2.hip's formula, the transforms' passes from tests/ntt_plan_checks.plan, and
small models of the bookkeeping (BucketSlot, TwiddleCache, direct_slots, ring_plan) say which branch every call takes.  The checks assert those
branches, so a changed threshold fails here instead of quietly ending the coverage.

The emulated runtime executes every stream operation at once and in order: there these checks see wrong bookkeeping, on the GPU they also run the
real streams — but a race a few microseconds wide stays a matter of reading the code on both."""
import atexit
import ctypes as C
import functools
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import halo2_lib_amd as H
from halo2_lib_amd import poseidon as PS
from halo2_lib_amd.h2hip import BASES_PLAIN, BASES_PRECOMPUTE
from oracle import bn254 as O
from oracle import c_oracle as CO
from tests import poseidon_hash_oracle as PO
from tests.golden_checks import golden_steps
from tests.knob_checks import knobs, scalar_column
from tests.ntt_plan_checks import assert_same, column, plan
from tests.util import Q, R, domain_consts, fr, full_range_fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p


# ------------------------------------------------------------------------------------------------------------------------- the planners
@functools.lru_cache(maxsize=1)
def _planner_exe():
    d = tempfile.mkdtemp(prefix="h2hip_msm_plan_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "msm_plan_selftest")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-x", "c++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "tests", "emu"), "-Wno-unused-value",
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "msm_plan_selftest.cpp"), "-lpthread"])
    return exe


def planned(cases):
    """what msm_plan / msm_batch_plan decide for each case line (the format of tests/emu/msm_plan_selftest.cpp): a dict of the printed fields"""
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("".join(c + "\n" for c in cases))
    try:
        out = subprocess.run([_planner_exe(), f.name], capture_output=True, text=True, timeout=60)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    plans = []
    for case, line in zip(cases, lines):
        assert line.startswith("rc=0 ") and "=" in line[5:], (case, line)
        plans.append(dict(t.split("=", 1) for t in line.split()[1:]))
    return plans


def table_windows(c):
    return (255 + c - 1) // c   # msm_windows, msm_plan.h


def bases_token(n, window=0):
    """a base set of the case format: plain, or precomputed for `window`"""
    return "%d:%d:%d" % (table_windows(window), window, n) if window else "1:0:%d" % n


def lone_bucket_bytes(n, window=0, table_window=0):
    """MsmPlan::buckets_bytes of one lone MSM: plain bases under msm_window_bits = window, or a table built for table_window"""
    case = "msm n=%d ncols=1 lane=0 bases=%s" % (n, bases_token(n, table_window)) + ("" if table_window else " msm_window_bits=%d" % window)
    return int(planned([case])[0]["bytes"].split(",")[5])


GRANULE = 1 << 20   # ws_reserve, capi.hip


def capacity(nbytes):
    return (max(nbytes, 256) + GRANULE - 1) // GRANULE * GRANULE


def g2_partial_bytes(n):
    """msm_g2_run's `partial` array (g2.hip): 32 windows x chunks x 256 buckets of G2Jac (three Fq2 of 64 bytes)"""
    chunk = 256 if n <= 4096 else 2048
    return 192 * 32 * ((n + chunk - 1) // chunk) * 256


class BucketSlot:
    """the bookkeeping of one zero-fill-after-use bucket array (ws_reserve's capacity, clean_bytes): which branch a use of `nbytes` takes"""

    def __init__(self):
        self.cap, self.clean = 0, 0

    def use(self, nbytes):
        if nbytes > self.cap:
            branch = "regrow" if self.cap else "allocate"
            self.cap = capacity(nbytes)
        elif self.clean >= nbytes:
            branch = "prezeroed"
        else:
            branch = "fill behind a smaller pending fill" if self.clean else "fill"
        self.clean = nbytes   # buckets_clean_after_use
        return branch

    def borrow(self, nbytes):
        """another user of the slot (the G2 MSM): no fill behind it"""
        grown = nbytes > self.cap
        if grown:
            self.cap = capacity(nbytes)
        self.clean = 0
        return grown


# ------------------------------------------------------------------------------------------------------------------------------ helpers
def _bases(n, k0, d):
    return CO.known_dlog_bases(n, fr([k0]), fr([d]))


def _check_msm(got, s, bases, threads, what):
    want = CO.best_multiexp(s, bases, threads=threads)
    assert np.array_equal(got, want), what
    return want


@functools.lru_cache(maxsize=None)
def g2_case(n, seed):
    """(points (n, 16), scalars, the expected affine point): bases (k0 + i * d) * G2 by repeated affine addition, one of them the identity; the
    expected sum is ONE scalar multiplication with oracle/pairing.py's arithmetic"""
    from oracle import pairing as PR

    k0, d = 4242 + seed, 11
    step, cur, pts = PR.g2_mul(PR.G2_GEN, d), PR.g2_mul(PR.G2_GEN, k0), []
    for _ in range(n):
        pts.append(cur)
        cur = PR.g2_add(cur, step)
    if n > 3:
        pts[3] = None
    s = full_range_fr(n, 700 + seed)
    total = sum(si * (k0 + i * d) for i, (si, p) in enumerate(zip(O.limbs_to_ints(s, R), pts)) if p is not None) % R
    vals = []
    for p in pts:
        vals += [0, 0, 0, 0] if p is None else [p[0][0], p[0][1], p[1][0], p[1][1]]
    limbs = O.ints_to_limbs(vals, Q).reshape(-1, 16)
    limbs.setflags(write=False)
    s.setflags(write=False)
    return limbs, s, (PR.g2_mul(PR.G2_GEN, total) if total else None)


def check_msm_g2_once(ctx, n, seed):
    pts, s, want = g2_case(n, seed)
    v = O.limbs_to_ints(ctx.msm_g2(pts, s).reshape(-1, 4), Q)
    assert (None if not any(v) else ((v[0], v[1]), (v[2], v[3]))) == want, ("G2 MSM", n, seed)


# ------------------------------------------------------------------------------------------------------ 1. the lone MSM's bucket array
LONE_N = 700
SMALL, MID, BIG, TABLE = 5, 8, 10, 7   # msm_window_bits of the plain calls; the window the precomputed set is built for
G2_N = 150
KINDS = ("uniform", "zero_one", "zero", "full_range", "equal")   # uniform, few distinct values, all zero, ...


def check_lone_bucket_array(make_ctx, threads):
    """One context, plain known-dlog bases, the window moved by msm_window_bits; every call with fresh scalars, every affine result bit for bit
    against the oracle's MSM.
      step 1  mid, small, mid again (the same buffer, more bytes than the last fill covered: the memset that has to wait for that fill,
              zero_or_await_buckets), big (regrows the buffer), small, mid
      step 2  a G1 MSM whose capacity holds a G2 MSM's `partial` array, that G2 MSM, the same G1 window again: without g2.hip's
              clean_bytes[0] = 0 the second G1 call would trust an array the G2 kernels wrote over
      step 3  a refused call (more scalars than bases) between two good ones
      step 4  a precomputed base set (its window fixed at upload) alternating with the plain one"""
    n = LONE_N
    size = {c: lone_bucket_bytes(n, c) for c in (SMALL, MID, BIG)}
    size["table"] = lone_bucket_bytes(n, table_window=TABLE)
    assert size[SMALL] < size[MID] <= GRANULE < size[BIG], size          # mid fits one capacity granule, big does not
    assert size[SMALL] < size["table"] < size[MID], size
    slot = BucketSlot()
    bases = _bases(n, 987654321, 31)
    calls = [0]

    def scalars():
        calls[0] += 1
        return scalar_column(KINDS[calls[0] % len(KINDS)], n, 3000 + calls[0])

    with make_ctx() as ctx:
        b = ctx.bases_upload(bases)
        with knobs(ctx, msm_window_bits=TABLE):
            bt = ctx.bases_upload(bases, BASES_PRECOMPUTE)
        try:
            def plain(c, branch):
                assert slot.use(size[c]) == branch, (c, branch)
                s = scalars()
                with knobs(ctx, msm_window_bits=c):
                    _check_msm(ctx.msm(b, s, H.POINT_AFFINE), s, bases, threads, ("plain", c, branch, calls[0]))

            def table(branch):
                assert slot.use(size["table"]) == branch, branch
                s = scalars()
                _check_msm(ctx.msm(bt, s, H.POINT_AFFINE), s, bases, threads, ("table", branch, calls[0]))

            # step 1
            plain(MID, "allocate")
            plain(SMALL, "prezeroed")
            plain(MID, "fill behind a smaller pending fill")
            plain(BIG, "regrow")
            plain(SMALL, "prezeroed")
            plain(MID, "fill behind a smaller pending fill")
            # step 2
            plain(BIG, "fill behind a smaller pending fill")
            assert slot.clean >= size[BIG] and g2_partial_bytes(G2_N) <= slot.cap, (size, g2_partial_bytes(G2_N))   # the G2 array fits inside: armed, not regrown
            check_msm_g2_once(ctx, G2_N, 1)
            assert not slot.borrow(g2_partial_bytes(G2_N))
            plain(BIG, "fill")
            # step 3
            plain(MID, "prezeroed")
            with pytest.raises(H.H2HipError):
                ctx.msm(b, scalar_column("uniform", n + 1, 1), H.POINT_AFFINE)
            plain(MID, "prezeroed")   # (the refusal came before anything touched the array)
            # step 4
            table("prezeroed")
            plain(MID, "fill behind a smaller pending fill")
            table("prezeroed")
            plain(SMALL, "prezeroed")
            table("fill behind a smaller pending fill")
            plain(BIG, "fill behind a smaller pending fill")
            table("prezeroed")
        finally:
            b.free()
            bt.free()
    return calls[0]


# -------------------------------------------------------------------------------------------------- 2. the batch's shared bucket array
BATCH_N, BATCH_WINDOW = 700, 6
# (entry point, columns, msm_defer_reduce, msm_fuse_cols, msm_lanes, clean_on_lane, the shared array's branch or None where the call has none)
BATCH_CALLS = (
    ("batch_dev", 2, 1, 0, 1, 1, "allocate"),
    ("lone", 1, 1, 0, 1, 1, None),
    ("batch_dev", 4, 1, 1, 3, 0, "fill behind a smaller pending fill"),   # grows inside the capacity
    ("multi_dev", 4, 0, 3, 2, 1, None),                                    # every lane reduces its own columns
    ("batch_dev", 3, 1, 3, 2, 0, "prezeroed"),
    ("host_batch", 3, 1, 1, 1, 1, "prezeroed"),
    ("batch_dev", 9, 1, 0, 3, 1, "regrow"),
    ("lone", 1, 0, 1, 2, 0, None),
    ("batch_dev", 2, 1, 3, 1, 0, "prezeroed"),
    ("batch_dev", 4, 1, 1, 3, 1, "fill behind a smaller pending fill"),   # the profiled call
)
PROFILED_CALL = len(BATCH_CALLS) - 1


def _cancelling_column(n, k0, d, seed):
    """non-zero scalars with sum_i s_i * (k0 + i * d) = 0: the MSM over the known-dlog bases is the identity"""
    s = O.limbs_to_ints(full_range_fr(n, seed, edges=False), R)
    rest = sum(v * (k0 + i * d) for i, v in enumerate(s) if i) % R
    s[0] = (-rest) * O.inv_mod(k0, R) % R
    assert all(s) and sum(v * (k0 + i * d) for i, v in enumerate(s)) % R == 0
    return fr(s)


def check_batch_shared_bucket_array(make_ctx, threads):
    """One context, precomputed bases with a small window: msm_batch_dev over 2, 4, 3, 9 and 2 columns with a lone msm, a msm_multi_dev over two
    base sets and the host-column msm_batch in between, msm_defer_reduce / msm_fuse_cols / msm_lanes / clean_on_lane changing from call to call
    (BATCH_CALLS).  Every batch holds an all-zero column and one whose terms cancel to the identity; every column of every call against the oracle.
    The last call runs with the kernel profile switched on after the lanes have long existed: the lanes take the switch with the knobs, at the
    start of every batch (ensure_lanes), so the profile has to count one msm_digits_kernel launch per group the planner forms."""
    n, c = BATCH_N, BATCH_WINDOW
    (k0a, da), (k0b, db) = (21, 4), (99, 9)
    bases_a, bases_b = _bases(n, k0a, da), _bases(n, k0b, db)
    pool = [_cancelling_column(n, k0a, da, 61), scalar_column("zero", n, 0)] + [scalar_column(k, n, 62 + i) for i, k in enumerate(
        ("uniform", "zero_one", "full_range", "equal", "uniform", "uniform", "full_range"))]
    want = {"a": [CO.best_multiexp(s, bases_a, threads=threads) for s in pool], "b": [CO.best_multiexp(s, bases_b, threads=threads) for s in pool]}
    assert not want["a"][0].any() and not want["a"][1].any() and want["b"][0].any()   # the identity twice; over the other set the first column does not cancel
    # what the batch planner decides for every call, and what that means for the shared array
    cases = []
    for kind, count, defer, fuse, lanes, col, _ in BATCH_CALLS:
        sets = bases_token(n, c) + (";" + bases_token(n, c) if kind == "multi_dev" else "")
        cols = "1,0,1,0" if kind == "multi_dev" else "-"
        cases.append("batch n=%d count=%d sets=%s cols=%s msm_defer_reduce=%d msm_fuse_cols=%d msm_lanes=%d clean_on_lane=%d" % (n, count, sets, cols, defer, fuse, lanes, col))
    plans = planned(cases)
    slot, seen = BucketSlot(), []
    for (kind, count, *_k, branch), p in zip(BATCH_CALLS, plans):
        if kind == "lone":
            continue
        assert (p["deferred"] == "1") == (branch is not None), (kind, count, p)
        if branch is not None:
            assert slot.use(int(p["buckets_bytes"])) == branch, (kind, count, p, slot.cap)
            seen.append((count, branch))
    # allocated for 2, grown inside the capacity by 4, trusted by 3 and 3, regrown by 9, trusted by 2 (and the profiled call's 4 grow inside again)
    assert seen[:6] == [(2, "allocate"), (4, "fill behind a smaller pending fill"), (3, "prezeroed"), (3, "prezeroed"), (9, "regrow"), (2, "prezeroed")], seen
    assert len(pool) >= max(cnt for _, cnt, *_r in BATCH_CALLS)

    with make_ctx() as ctx:
        with knobs(ctx, msm_window_bits=c):
            ba, bb = ctx.bases_upload(bases_a, BASES_PRECOMPUTE), ctx.bases_upload(bases_b, BASES_PRECOMPUTE)
        bp = ctx.bases_upload(bases_a)
        dev = [ctx.to_device(s) for s in pool]
        try:
            for i, (kind, count, defer, fuse, lanes, col, _) in enumerate(BATCH_CALLS):
                idx = [0, 1] + [2 + (i + j) % (len(pool) - 2) for j in range(count - 2)] if count >= 2 else [2 + i % (len(pool) - 2)]
                if count > 2:
                    idx = idx[2:3] + idx[:2] + idx[3:]   # (the two identities not always in front)
                assert len(set(idx)) == count
                if i == PROFILED_CALL:
                    ctx.profile_reset()
                    ctx.profile_enable(True)
                with knobs(ctx, msm_defer_reduce=defer, msm_fuse_cols=fuse, msm_lanes=lanes, clean_on_lane=col):
                    if kind == "lone":
                        s = pool[idx[0]]
                        got = ctx.msm(ba if i == 1 else bp, s, H.POINT_AFFINE)
                        which = ["a"]
                    elif kind == "batch_dev":
                        got = ctx.msm_batch_dev(ba, [dev[j] for j in idx], n, H.POINT_AFFINE)
                        which = ["a"] * count
                    elif kind == "host_batch":
                        got = ctx.msm_batch(ba, [pool[j] for j in idx], H.POINT_AFFINE)
                        which = ["a"] * count
                    else:
                        which = ["b", "a", "b", "a"]   # (the cancelling column over the set it cancels over)
                        got = ctx.msm_multi_dev([ba if w == "a" else bb for w in which], [dev[j] for j in idx], n, H.POINT_AFFINE)
                for col_i, (j, w) in enumerate(zip(idx, which)):
                    assert np.array_equal(got[col_i:col_i + 1], want[w][j]), (i, kind, count, col_i, j, w)
                if i == PROFILED_CALL:
                    ctx.profile_enable(False)
                    groups = len([g for g in plans[i]["groups"].split(",") if g])
                    assert groups == count > 1 and int(plans[i]["NL"]) > 1, plans[i]   # one column per group, dealt to several lanes
                    assert ctx.profile_dump().get("msm_digits_kernel", (0, 0, 0))[1] == groups, ctx.profile_dump()
        finally:
            for d in dev:
                ctx.free(d)
            for x in (ba, bb, bp):
                x.free()
    return len(BATCH_CALLS)


# ------------------------------------------------------------------------------------------------------------------- 3. twiddle sets
TWIDDLE_SETS = 16      # get_twiddles, ntt.hip: the cache's bound, first in first out
DIRECT_SLOTS = 4       # TwiddleSet::direct
TWIDDLE_LOGS = (4, 5, 6, 7, 8)
DIRECT_LOG_N = 11
# (ntt_tile_bits, ntt_min_col_bits) of the walk over one pair's direct tables
DIRECT_WALK = ((10, 2), (6, 2), (6, 3), (4, 2), (10, 5), (6, 3), (4, 2), (10, 2))


class TwiddleCache:
    """get_twiddles' bookkeeping: the resident (log_n, omega) pairs in the order they were made"""

    def __init__(self):
        self.resident, self.made = [], {}

    def touch(self, log_n, omega):
        key = (log_n, omega)
        if key in self.resident:
            return False
        self.made[key] = self.made.get(key, 0) + 1
        if len(self.resident) >= TWIDDLE_SETS:
            self.resident.pop(0)
        self.resident.append(key)
        return True


def roots_of(log_n):
    """four primitive 2^log_n-th roots of unity: omega, omega^-1, omega^3, omega^5"""
    w = O.omega_for(log_n)
    roots = [w, O.inv_mod(w, R), pow(w, 3, R), pow(w, 5, R)]
    assert len(set(roots)) == 4 and all(pow(r, 1 << (log_n - 1), R) == R - 1 for r in roots)
    return roots


def dft(a, root, scale=1):
    """the definition: out[j] = scale * sum_i a[i] * root^(i * j)"""
    n = len(a)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * root % R
    return [scale * sum(x * pw[i * j % n] for i, x in enumerate(a)) % R for j in range(n)]


def _ints(a):
    return O.limbs_to_ints(np.ascontiguousarray(a).reshape(-1, 4), R)


def direct_slots(log_n, walk):
    """which direct tables (by log_s) the plans of `walk` ask for, in order, and which of them get one of the set's slots (get_direct_table)"""
    asked, slots = [], []
    for tb, mcb in walk:
        for p in plan(log_n, tile_bits=tb, min_col_bits=mcb):
            if p["direct"]:
                asked.append(p["log_s"])
                if p["log_s"] not in slots and len(slots) < DIRECT_SLOTS:
                    slots.append(p["log_s"])
    return asked, slots


def check_twiddle_sets(make_ctx, threads):
    """One context: best_fft at 2^4 .. 2^8 with four primitive roots each (20 sets, the cache holds 16), then the same 20 in reverse order, then as
    listed once more — the cache drops the oldest set, so the reversed pass finds the 16 youngest sets resident and re-creates four; the third pass
    re-creates every one of the 20 behind an eviction (asserted on the model of the cache).  Every transform against the definition with the same root.
    Between the passes: permutation_product_terms and a quotient permutation term, whose kernels read the power table of a pair that has been
    evicted by then (ntt_pow_table), an ifft and a coeff_to_extended on resident pairs.
    Then one pair walked through tile / column-bit plans that ask for more direct tables than a set has slots: every transform, those whose table
    found no slot among them, against the oracle."""
    cache = TwiddleCache()
    keys = [(ln, r) for ln in TWIDDLE_LOGS for r in roots_of(ln)]
    assert len(keys) == 20 > TWIDDLE_SETS
    inputs = {key: column(1 << key[0], 2000 + i) for i, key in enumerate(keys)}
    wants = {key: dft(_ints(inputs[key]), key[1]) for key in keys}

    with make_ctx() as ctx:
        def forward(key):
            cache.touch(*key)
            assert _ints(ctx.best_fft(inputs[key], fr([key[1]]), key[0])) == wants[key], ("best_fft", key[0], keys.index(key) % 4)

        for key in keys:
            forward(key)
        assert all(cache.made[key] == 1 for key in keys) and cache.resident == keys[4:]
        # the permutation factors over 2^4 rows: omega^i comes from the power table of (4, omega), evicted by now
        w4 = O.omega_for(4)
        assert (4, w4) not in cache.resident
        cache.touch(4, w4)
        cols, sigs = [full_range_fr(16, 2100 + j) for j in range(3)], [full_range_fr(16, 2110 + j) for j in range(3)]
        beta, gamma, first = 0x1234567, 0x89ABCDEF, 2
        gn, gd = ctx.permutation_product_terms(cols, sigs, first, fr([beta]), fr([gamma]), fr([O.DELTA]), fr([w4]))
        wn, wd = [1] * 16, [1] * 16
        for j, (cl, sg) in enumerate(zip(cols, sigs)):
            bd = beta * pow(O.DELTA, first + j, R) % R
            for i, (cv, sv) in enumerate(zip(_ints(cl), _ints(sg))):
                wn[i] = wn[i] * (cv + bd * pow(w4, i, R) + gamma) % R
                wd[i] = wd[i] * (cv + beta * sv + gamma) % R
        assert _ints(gn) == wn and _ints(gd) == wd
        # a permutation term of the quotient over 2^5 extended points: (5, omega) went out when (4, omega) came back
        k, ek = 3, 5
        w5 = O.omega_for(ek)
        assert (ek, w5) not in cache.resident
        cache.touch(ek, w5)
        ne, step = 1 << ek, 1 << (ek - k)
        rs = lambda seed: _ints(full_range_fr(ne, 2200 + seed))
        acc, z, zp, l0, ll, lb = [rs(i) for i in range(6)]
        pc, ps = [rs(10 + j) for j in range(3)], [rs(20 + j) for j in range(3)]
        y = 0x13579B
        for terms, prev, j0, rot in ((1 | 8, None, 0, 0), (2 | 4 | 8, zp, 3, -3)):
            got = ctx.quotient_permutation_set(fr(acc), fr(z), None if prev is None else fr(prev), [fr(v) for v in pc], [fr(v) for v in ps], j0, fr(l0), fr(ll),
                                               fr(lb), ek, k, terms, rot, fr([beta]), fr([gamma]), fr([O.DELTA]), fr([O.ZETA]), fr([w5]), fr([y]))
            want = O.quotient_permutation_set_terms(acc, z, prev, pc, ps, j0, l0, ll, lb, step, terms, rot % (1 << k), beta, gamma, O.DELTA, O.ZETA, w5, y)
            assert _ints(got) == want, terms
        # an inverse transform and a coset extension on resident pairs
        w6inv = O.inv_mod(O.omega_for(6), R)
        assert not cache.touch(6, w6inv)
        a = column(64, 2300)
        assert _ints(ctx.ifft(a, fr([w6inv]), 6, fr([O.inv_mod(64, R)]))) == dft(_ints(a), w6inv, O.inv_mod(64, R))
        w7 = O.omega_for(7)
        assert not cache.touch(7, w7)
        a = column(32, 2301)
        scaled = [v * pow(O.ZETA, i % 3, R) % R for i, v in enumerate(_ints(a))] + [0] * 96
        assert _ints(ctx.coeff_to_extended(a, 5, 7, fr([w7]), fr([O.ZETA]))) == dft(scaled, w7)
        # the reversed pass, the listed order again
        made = sum(cache.made.values())
        for key in reversed(keys):
            forward(key)
        assert sum(cache.made.values()) - made == 4
        for key in keys:
            forward(key)
        assert all(cache.made[key] >= 2 for key in keys), cache.made   # every one re-created behind an eviction
        assert len(cache.resident) == TWIDDLE_SETS

        # ---- the four direct-table slots of one pair
        log_n = DIRECT_LOG_N
        asked, slots = direct_slots(log_n, DIRECT_WALK)
        assert len(set(asked)) > DIRECT_SLOTS and len(slots) == DIRECT_SLOTS, (asked, slots)
        w, winv, div = domain_consts(log_n)
        a = column(1 << log_n, 2400)
        want_f = CO.best_fft(a, log_n, w, threads=threads)
        b = column(1 << log_n, 2401)
        want_i = CO.ifft(b, log_n, w, threads=threads)
        past = 0
        for tb, mcb in DIRECT_WALK:
            need = [p["log_s"] for p in plan(log_n, tile_bits=tb, min_col_bits=mcb) if p["direct"]]
            past += any(s not in slots for s in need)
            with knobs(ctx, ntt_tile_bits=tb, ntt_min_col_bits=mcb):
                assert_same(ctx.best_fft(a, w, log_n), want_f, "best_fft 2^%d, tile %d, column bits %d (tables %s, slots %s)" % (log_n, tb, mcb, need, slots))
        assert past >= 2   # transforms with a table past the fourth slot: the composed lookup
        # the inverse root is a pair of its own, with its own four slots: the walk backwards fills them in another order
        for tb, mcb in reversed(DIRECT_WALK):
            with knobs(ctx, ntt_tile_bits=tb, ntt_min_col_bits=mcb):
                assert_same(ctx.ifft(b, winv, log_n, div), want_i, "ifft 2^%d, tile %d, column bits %d" % (log_n, tb, mcb))
    return sum(cache.made.values())


# --------------------------------------------------------------------------------------------------------------------- 4. the job ring
JOB_RING_BYTES = 1 << 20                 # capi.hip
KATE_JOB_BYTES = (3 + 24) * 32           # KateJob, poly_eval.hip: b, w, top and a PowTable of 24 Fr
KATE_JOB29_BYTES = (4 + 9) * 36          # KateJob29: b, w, one, top and nine powers, each nine 32-bit limbs
KATE_N = 300
KATE_CALLS = 320


def ring_plan(calls):
    """(bytes staged, wraps) of `calls` multi-point divisions, m = 1 + i % 8 points and kate_29 = (i // 8) % 2: a call stages its jobs padded to a
    multiple of four, each table rounded up to 256 bytes (upload_jobs), the unsaturated table only with kate_29"""
    staged = wraps = off = 0
    for i in range(calls):
        total = (1 + i % 8 + 3) // 4 * 4
        for nbytes in [KATE_JOB_BYTES * total] + ([KATE_JOB29_BYTES * total] if (i // 8) % 2 else []):
            need = (nbytes + 255) // 256 * 256
            if off + need > JOB_RING_BYTES:
                wraps, off = wraps + 1, 0
            off += need
            staged += need
    return staged, wraps


def check_job_ring(make_ctx, threads):
    """h2hip_fr_kate_division_multi_dev back to back on 300-coefficient polynomials, m cycling through 1 .. 8, kate_29 switching every eight calls
    (half the calls each), every call into an output buffer of its own, nothing downloaded or synchronised until the end.  A cycle of sixteen
    calls stages 41,984 + 65,536 bytes of job tables, so KATE_CALLS = 320 calls stage 2,150,400 bytes, more than twice the 1 MiB ring (304
    would not do), and wrap it twice.  Then every quotient against the oracle's divisions combined with the weights."""
    staged, wraps = ring_plan(KATE_CALLS)
    assert staged > 2 * JOB_RING_BYTES and wraps >= 2, (staged, wraps)
    assert ring_plan(KATE_CALLS - 16)[0] <= 2 * JOB_RING_BYTES   # (the count is the smallest number of whole cycles that does)
    n = KATE_N
    polys = [full_range_fr(n, 4000 + j) for j in range(3)]
    pts = [full_range_fr(1 + i % 8, 4100 + i) for i in range(KATE_CALLS)]
    ws = [full_range_fr(1 + i % 8, 4500 + i) for i in range(KATE_CALLS)]
    with make_ctx() as ctx:
        old = ctx.get_param("kate_29")
        dp = [ctx.to_device(p) for p in polys]
        out = ctx.malloc(32 * (n - 1) * KATE_CALLS)
        try:
            for i in range(KATE_CALLS):
                ctx.set_param("kate_29", (i // 8) % 2)
                m = 1 + i % 8
                ctx._chk(ctx.lib.h2hip_fr_kate_division_multi_dev(ctx.handle, _vp(out + 32 * (n - 1) * i), _vp(dp[i % 3]), n, pts[i].ctypes.data_as(_vp),
                                                                  ws[i].ctypes.data_as(_vp), m))
            got = ctx.download(out, (KATE_CALLS, n - 1, 4))
        finally:
            ctx.set_param("kate_29", old)
            for d in dp + [out]:
                ctx.free(d)
    for i in range(KATE_CALLS):
        want = None
        for j in range(1 + i % 8):
            q = CO.fr_kate_division(polys[i % 3], pts[i][j:j + 1])
            t = CO.fr_mul(q, np.repeat(ws[i][j:j + 1], len(q), axis=0))
            want = t if want is None else CO.fr_add(want, t)
        assert np.array_equal(got[i], want), ("call", i, "m", 1 + i % 8, "kate_29", (i // 8) % 2)
    return wraps


# ------------------------------------------------------------------------------------------------------------------ 5. Poseidon specs
def _set_plain(ctx, sp):
    ctx.poseidon_set_spec(sp.t, sp.r_f, sp.r_p, fr([c for row in sp.constants for c in row]), fr([m for row in sp.mds for m in row]))


def _msgs(count, length, seed):
    vals = _ints(full_range_fr(count * length, seed))
    return [vals[i * length:(i + 1) * length] for i in range(count)]


def _hash_batch(ctx, sp, msgs, what):
    rows = fr([v for m in msgs for v in m]).reshape(len(msgs), len(msgs[0]), 4)
    assert _ints(ctx.poseidon_hash(rows)) == [PO.H(sp, m) for m in msgs], what


def _fill_digests(ctx, hs, sp, msgs, what):
    """hash_fix_len_array traces of `msgs` through the RESIDENT optimised spec (no select here): their digest cells against the sponge"""
    ln = len(msgs[0])
    ncells, offs = hs.trace_layout(ln, 0)
    raw = fr([v for m in msgs for v in m])
    rows = len(msgs) * ncells + 16
    d_col, d_in = ctx.to_device(np.zeros((rows, 4), dtype=np.uint64)), ctx.to_device(raw)
    try:
        units = [(0, j * ncells + 1, j * ln, 1, 0) for j in range(len(msgs))]
        PS.fill_hashes(ctx, [d_col], rows - 7, None, d_in, len(raw), ln, units)
        col = ctx.download(d_col, (rows, 4))
    finally:
        ctx.free(d_col)
        ctx.free(d_in)
    assert _ints(col[[u[1] + offs[1] for u in units]]) == [PO.H(sp, m) for m in msgs], what


def check_poseidon_specs(make_ctx):
    """One context: the t = 3 spec, hash_batch; the t = 5 spec, hash_batch and a small Merkle tree; t = 3 again with another r_p, hash_batch.  The
    optimised spec (another slot, another width) is set between two of the steps and filled through twice, once before and once after the plain
    spec changes under it; hash_batch runs right after it is set without the plain spec being set again.  Digests, roots and digest cells against
    oracle/poseidon.py's permutation under the sponge of tests/poseidon_hash_oracle.py."""
    s3, s5, s3b = PO.spec(3), PO.spec(5), PO.spec(3, 8, 56)
    assert (s3b.r_f, s3b.r_p) != (s3.r_f, s3.r_p)
    with make_ctx() as ctx:
        _set_plain(ctx, s3)
        _hash_batch(ctx, s3, _msgs(5, 2, 5000), "t = 3")
        # the optimised spec of the OTHER width: the plain spec stays what it was
        h5 = PS.PoseidonHasher.new(ctx, 5, *PO.SPECS[5])
        h5.select_optimized()
        _fill_digests(ctx, h5, s5, _msgs(3, 4, 5001), "fill through the optimised t = 5 spec")
        _hash_batch(ctx, s3, _msgs(6, 3, 5002), "t = 3 behind set_optimized_spec")
        _set_plain(ctx, s5)
        _hash_batch(ctx, s5, _msgs(4, 5, 5003), "t = 5")
        leaves = [m[0] for m in _msgs(8, 1, 5004)]
        assert _ints(ctx.poseidon_merkle_tree(fr(leaves))) == PO.merkle_tree(s5, leaves)
        # ... and the other way round: the optimised spec after two plain specs came and went
        _set_plain(ctx, s3b)
        _fill_digests(ctx, h5, s5, _msgs(2, 3, 5005), "fill behind two set_spec calls")
        _hash_batch(ctx, s3b, _msgs(5, 2, 5006), "t = 3, r_p = 56")
        _hash_batch(ctx, s3b, _msgs(3, 4, 5007), "t = 3, r_p = 56, two chunks")
        # the optimised t = 3 spec replaces the t = 5 one; the plain one is still r_p = 56
        h3 = PS.PoseidonHasher.new(ctx, 3, *PO.SPECS[3])
        h3.select_optimized()
        _fill_digests(ctx, h3, s3, _msgs(3, 2, 5008), "fill through the optimised t = 3 spec")
        _hash_batch(ctx, s3b, _msgs(2, 2, 5009), "t = 3, r_p = 56, behind the second set_optimized_spec")


# ------------------------------------------------------------------------------------------------------------------------ 6. any order
def _g2_step(ctx):
    check_msm_g2_once(ctx, 37, 2)


def _lagrange_step(ctx):
    """g1_to_lagrange at k = 3 on g_i = s^i * G: every point against (the inverse transform of the exponents, by the definition) * G"""
    k, n = 3, 8
    sv = 0x1D0C0FFEE + k
    a = [pow(sv, i, R) for i in range(n)]
    b = dft(a, O.inv_mod(O.omega_for(k), R), O.inv_mod(n, R))
    mul = lambda v: O.g1_mul(O.G1_GEN, v) if v else None
    want = O.points_to_limbs([mul(v) for v in b])
    for flags in (BASES_PLAIN, BASES_PRECOMPUTE):
        g = ctx.bases_upload(O.points_to_limbs([mul(v) for v in a]), flags)
        lg = None
        try:
            lg = ctx.g1_to_lagrange(g, k, flags)
            assert np.array_equal(ctx.bases_download(lg), want), flags
        finally:
            g.free()
            if lg is not None:
                lg.free()


def order_steps():
    return golden_steps() + [("msm_g2", _g2_step), ("g1_to_lagrange_k3", _lagrange_step)]


ORDERS = ("listed", "reversed", "shuffled")


def ordered(steps, order):
    steps = list(steps)
    if order == "reversed":
        steps.reverse()
    elif order == "shuffled":
        random.Random(20240607).shuffle(steps)
    else:
        assert order == "listed"
    return steps


def check_any_order(make_ctx, order):
    """the committed small cases (tests/golden_checks.golden_steps), a G2 MSM and g1_to_lagrange at k = 3 on ONE context in the given order: an entry
    point that leaves something in a scratch slot which another one assumes fails in one of the orders"""
    steps = ordered(order_steps(), order)
    if order == "shuffled":
        names = [n for n, _ in steps]
        assert names != [n for n, _ in order_steps()] and names != [n for n, _ in reversed(order_steps())]
    with make_ctx() as ctx:
        for name, step in steps:
            try:
                step(ctx)
            except AssertionError as e:
                raise AssertionError("step %s failed in the %s order (%s)" % (name, order, [n for n, _ in steps])) from e
    return len(steps)
