"""What the checks of the fused trace fills share (h2hip_fp_mul_fill_dev, h2hip_ec_fill_dev, h2hip_fp_cmp_fill_dev, h2hip_ec_select_fill_dev,
h2hip_num_to_bits_fill_dev): one record per kind of unit, and the checks written once over it.  tests/fp_mul_checks.py,
tests/ec_fill_checks.py, tests/ec_strict_checks.py and tests/ec_select_checks.py keep what is theirs: the definition of their unit (the
specification, never shared), the pools, the layout checks, the table of break cells, their own refusals, their chains and their proof program.

  a kind (FpMul, EcOp, Cmp, Select, FromBits, Bits) knows its name, nres (results per unit), how the operands of a case lie in values
      (unit), its definition on a thread (define -> a Unit with start / end / results / queue / gaps / out_offsets), its layout, its fill and,
      where the unit has range gaps, fill_ranges and range_tables (None for the selections and num_to_bits).  A case is a tuple of the
      unit's operands, each a list of values: (a, b), (P, Q), (P, Q, [sel]), (table, bits), ([value],)
  check_fill, check_no_results, check_breaks   the fill against the definition over sentinel-filled columns
  RefusalBench      `refused`, the sentinel columns and results, the call builders and the refusals every entry point shares
  alike_bench, check_refuse_alike   entry points given the same bad argument give the same reason
  check_names       the header, the Rust sys crate and ctypes agree
  ProofBench        a BaseConfig circuit around a program of units: key, device buffers, the proof's checks, one changed cell

Every comparison is bit-exact."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import halo2_lib_amd as H
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import virtual_region as VR
from oracle import plonk as P
from tests.dyn_lookup_util import rng_budget, srs, vk_from_gpu
from tests.poseidon_trace_checks import _compare as compare
from tests.poseidon_trace_checks import _ints as ints
from tests.poseidon_trace_checks import place
from tests.range_fill_checks import lookup_positions
from tests.rlc_checks import SENTINEL
from tests.util import PreDrawnRng, R, fr

__all__ = ["compare", "ints", "place", "lookup_positions", "SENTINEL", "operand", "thread", "own_mask", "signed", "tdiv"]
_vp = C.c_void_p
ERR_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def signed(v):
    """fe_to_bigint (halo2-base/src/utils/mod.rs:199-208)"""
    return v if v <= R // 2 else v - R


def tdiv(a, b):
    """BigInt's `/`: toward zero"""
    return abs(a) // b if a >= 0 else -(abs(a) // b)


def thread(lb=8):
    cm = VR.CopyConstraintManager()
    ctx = VR.Context(False, "fp", 0, cm)
    return ctx, VR.RangeChip(lb, VR.LookupAnyManager(False, cm)), cm


def operand(vals, tag):
    return [VR.AssignedValue(v % R, VR.ContextCell("operand", tag, i)) for i, v in enumerate(vals)]


def own_mask(u):
    own = np.ones(u.end - u.start, dtype=bool)
    for at, cells, _bits, _res in u.gaps:
        own[at:at + cells] = False
    return own


def queue_len(ctx, chip):
    return len(chip.lookup_manager.cells_to_lookup.get(ctx.tag(), []))


def first_positions(ncells, bps, ncols, col=0, row=0):
    """{cell index: its first (column, row)} of a run laid down from (col, row)"""
    first = {}
    for i, c, r in place(col, row, ncells, bps, ncols)[0]:
        first.setdefault(i, (c, r))
    return first


def flatten(cases):
    """the cases' operands one behind the other -> (the values, where each case begins)"""
    vals, at = [], []
    for case in cases:
        at.append(len(vals))
        vals += [v % R for part in case for v in part]
    return vals, at


# ------------------------------------------------------------------------------------------------ the kinds
# (a definition is imported where a kind calls it: the modules that hold the definitions import this one)
class Kind:
    """one kind of fused unit; the protocol is this class's methods and name / nres / sp / params / lb.  entry, table, head and tail say how
    the library function is called without the Python wrapper: entry(ctx, columns, num_columns, usable_rows, break_points, *head, values,
    values_len, results, results_len, *tail, table, count)"""
    sp = None
    lb = 8
    fill_ranges = range_tables = None      # (a kind without range gaps)

    def with_(self, **changes):
        """the same kind called with other arguments (params, op, w, nb): for the refusals"""
        other = copy.copy(self)
        for name, value in changes.items():
            setattr(other, name, value)
        return other

    def unit(self, col, row, at, case):
        """the unit at (col, row) whose operands lie at `at` of the values, one behind the other in the case's order"""
        return self.unit_of(col, row, *[at + sum(len(part) for part in case[:i]) for i in range(len(case))])

    def unit_of(self, col, row, *offsets):
        return (col, row) + offsets

    def unit_def(self, case):
        """one unit on a thread of its own -> (the Unit, its cells, the lookup values in queue order)"""
        ctx, chip, _ = thread(self.lb)
        u = self.define(ctx, chip, case)
        return u, list(ctx.advice), [c.value for c in chip.lookup_manager.cells_to_lookup.get(ctx.tag(), [])]

    def head(self, params_ptr):
        return [params_ptr, self.op]

    def tail(self):
        return []


class _Ranged(Kind):
    """a kind with two operands, params and range gaps; api: its layout, fill, fill_with_ranges and range_tables functions of plonk.py"""

    def __init__(self, sp):
        self.sp, self.params, self.lb = sp, sp.params(), sp.lb

    def _op(self):
        return [self.op]

    def define(self, ctx, chip, case, tag=0):
        return self.definition(ctx, chip, operand(case[0], 2 * tag), operand(case[1], 2 * tag + 1))

    def layout(self, lib=None):
        return self.api[0](self.params, *self._op(), lib)

    def fill(self, ctx, cols, usable, bps, d_vals, nvals, d_res, nres, units, count=None):
        self.api[1](ctx, cols, usable, bps, self.params, *self._op(), d_vals, nvals, d_res, nres, units, count)

    def fill_ranges(self, ctx, cols, usable, bps, lks, d_vals, nvals, d_res, nres, units, slots):
        self.api[2](ctx, cols, usable, bps, lks, self.params, *self._op(), d_vals, nvals, d_res, nres, units, slots)

    def range_tables(self, bps, ncols, units, slots):
        return self.api[3](bps, ncols, self.params, *self._op(), units, slots)

    def head(self, params_ptr):
        return [params_ptr] + self._op()


class FpMul(_Ranged):
    """FpChip::mul; a case: (a's k + 1 values, b's)"""
    name, entry, table = "fp_mul", "h2hip_fp_mul_fill_dev", staticmethod(PL.fp_mul_table)
    api = (PL.fp_mul_layout, PL.fp_mul_fill, PL.fp_mul_fill_with_ranges, PL.fp_mul_range_tables)

    def __init__(self, sp):
        _Ranged.__init__(self, sp)
        self.nres = 3 * sp.k + 1

    def _op(self):
        return []

    def definition(self, ctx, chip, a, b):
        from tests import fp_mul_checks
        return fp_mul_checks.fp_mul(ctx, chip, self.sp, a, b)


class EcOp(_Ranged):
    """ec_add_unequal, ec_double or ec_sub_unequal, not strict; a case: (P's 2 (k + 1) values, Q's); ec_double does not read Q"""
    entry, table = "h2hip_ec_fill_dev", staticmethod(PL.ec_op_table)
    api = (PL.ec_layout, PL.ec_fill, PL.ec_fill_with_ranges, PL.ec_range_tables)

    def __init__(self, sp, op):
        _Ranged.__init__(self, sp)
        self.op, self.nres = op, 9 * sp.k + 3
        self.name = {PL.EC_ADD_UNEQUAL: "add_unequal", PL.EC_DOUBLE: "double", PL.EC_SUB_UNEQUAL: "sub_unequal"}[op]

    def definition(self, ctx, chip, pt, qt):
        from tests import ec_strict_checks
        return ec_strict_checks.curve_op(ctx, chip, self.sp, self.op, pt, qt)


class Cmp(_Ranged):
    """FpChip's comparisons of one mask; a case: (a's k + 1 values, b's)"""
    entry, table = "h2hip_fp_cmp_fill_dev", staticmethod(PL.fp_mul_table)
    api = (PL.fp_cmp_layout, PL.fp_cmp_fill, PL.fp_cmp_fill_with_ranges, PL.fp_cmp_range_tables)

    def __init__(self, sp, mask):
        _Ranged.__init__(self, sp)
        k = sp.k
        self.op, self.name = mask, "cmp mask %d" % mask
        self.nres = (k + 1) * (bool(mask & PL.FP_CMP_REDUCE_A) + bool(mask & PL.FP_CMP_REDUCE_B)) + (1 if mask & PL.FP_CMP_EQUAL else 0)

    def definition(self, ctx, chip, a, b):
        from tests import ec_strict_checks
        return ec_strict_checks.cmp_op(ctx, chip, self.sp, self.op, a, b)


class Select(Kind):
    """ec_select; a case: (P's 2 (k + 1) values, Q's, [sel])"""
    name, op, w, entry, table = "select", PL.EC_SELECT, 0, "h2hip_ec_select_fill_dev", staticmethod(PL.ec_select_table)

    def __init__(self, sp):
        self.sp, self.params, self.nres = sp, sp.params(), 2 * (sp.k + 1)

    def define(self, ctx, chip, case, tag=0):
        from tests import ec_select_checks
        p, q, s = case
        return ec_select_checks.ec_select(ctx, self.sp, operand(p, 3 * tag), operand(q, 3 * tag + 1), operand(s, 3 * tag + 2)[0])

    def unit_of(self, col, row, p, q, sel=0):
        return (col, row, p, q, sel)

    def layout(self, lib=None):
        return PL.ec_select_layout(self.params, self.op, self.w, lib)

    def fill(self, ctx, cols, usable, bps, d_vals, nvals, d_res, nres, units, count=None):
        PL.ec_select_fill(ctx, cols, usable, bps, self.params, self.op, self.w, d_vals, nvals, d_res, nres, units, count)

    def head(self, params_ptr):
        return [params_ptr, self.op, self.w]


class FromBits(Select):
    """ec_select_from_bits; a case: (the table's 2^w points flat, the w bits)"""
    op = PL.EC_SELECT_FROM_BITS

    def __init__(self, sp, w):
        Select.__init__(self, sp)
        self.w, self.name = w, "from_bits w = %d" % w

    def define(self, ctx, chip, case, tag=0):
        from tests import ec_select_checks
        table, bits = case
        pt = self.nres
        cells = operand(table, 2 * tag)
        return ec_select_checks.ec_select_from_bits(ctx, self.sp, [cells[j * pt:(j + 1) * pt] for j in range(1 << self.w)], operand(bits, 2 * tag + 1))

    def unit_of(self, col, row, table, bits):
        return (col, row, table, 0, bits)


class Bits(Kind):
    """GateChip::num_to_bits; a case: ([the value],)"""
    entry, table = "h2hip_num_to_bits_fill_dev", staticmethod(PL.bits_unit_table)

    def __init__(self, nb):
        self.nb, self.nres, self.name = nb, nb, "num_to_bits %d" % nb

    def define(self, ctx, chip, case, tag=0):
        from tests import ec_select_checks
        return ec_select_checks.num_to_bits(ctx, operand(case[0], tag)[0], self.nb)

    def layout(self, lib=None):
        return PL.num_to_bits_layout(self.nb, lib)

    def fill(self, ctx, cols, usable, bps, d_vals, nvals, d_res, nres, units, count=None):
        PL.num_to_bits_fill(ctx, cols, usable, bps, d_vals, nvals, d_res, nres, self.nb, units, count)

    def head(self, params_ptr):
        return []

    def tail(self):
        return [self.nb]


# ------------------------------------------------------------------------------------------------ the fill against its definition
def check_fill(ctx, kind, pool, count, nl=1):
    """`count` units per call over three gate columns (no breaks, a one-row hole after every odd unit), until every case of the pool was a
    unit.  The bare call: own cells equal the definition's, the gaps and every other cell keep the sentinel, results_dev equals the
    definition's results.  For a kind with range gaps also its *_with_ranges call over nl lookup columns: the whole run and the lookup
    columns equal the definition's, the queue starting at a position that is no multiple of nl."""
    lay = kind.layout(ctx.lib)
    vals, at = flatten(pool)
    nres = kind.nres
    cache = {}
    done = 0
    d_vals = ctx.to_device(fr(vals))
    try:
        while done < len(pool):
            units, defs, slots, rows, slot = [], [], [], [1, 3, 0], nl + 1 if nl > 1 else 1
            for j in range(count):
                i = (done + j) % len(pool)
                if i not in cache:
                    cache[i] = kind.unit_def(pool[i])
                u, cells, lookups = cache[i]
                assert len(cells) == lay[0]
                col = j % 3
                units.append(kind.unit(col, rows[col], at[i], pool[i]))
                defs.append((u, cells, lookups))
                slots.append(slot)
                rows[col] += len(cells) + (j % 2)
                if kind.fill_ranges:
                    slot += len(lookups) + (j % 2)
            done += count
            rows_n = max(max(rows), -(-slot // nl)) + 9
            where = lookup_positions(slot, nl)
            for with_ranges in (False, True) if kind.fill_ranges else (False,):
                want = [np.tile(SENTINEL, (rows_n, 1)) for _ in range(3)]
                want_lk = [np.tile(SENTINEL, (rows_n, 1)) for _ in range(nl if kind.fill_ranges else 0)]
                want_res = np.tile(SENTINEL, (count * nres + 2, 1))
                d_cols = [ctx.to_device(c) for c in want]
                d_lk = [ctx.to_device(c) for c in want_lk]
                d_res = ctx.to_device(want_res)
                for j, (unit, (u, cells, lookups), s) in enumerate(zip(units, defs, slots)):
                    keep = np.ones(len(cells), dtype=bool) if with_ranges else own_mask(u)
                    want[unit[0]][unit[1]:unit[1] + len(cells)][keep] = fr(cells)[keep]
                    want_res[j * nres:(j + 1) * nres] = fr(u.results)
                    if with_ranges:
                        for i, v in enumerate(fr(lookups) if lookups else []):
                            c, r = where[s + i]
                            want_lk[c][r] = v
                try:
                    if with_ranges:
                        kind.fill_ranges(ctx, d_cols, rows_n - 2, None, d_lk, d_vals, len(vals), d_res, count * nres, units, slots)
                    else:
                        kind.fill(ctx, d_cols, rows_n - 2, None, d_vals, len(vals), d_res, count * nres, units)
                    ctx.sync()
                    what = "%s, count = %d, nl = %d, ranges = %s" % (kind.name, count, nl, with_ranges)
                    if kind.sp is not None:
                        what = "(n, k, lb) = (%d, %d, %d), " % (kind.sp.n, kind.sp.k, kind.sp.lb) + what
                    compare(ctx, d_cols, want, what + " (gate columns)")
                    if kind.fill_ranges:
                        compare(ctx, d_lk, want_lk, what + " (lookup columns)")
                    compare(ctx, [d_res], [want_res], what + " (results)")
                finally:
                    for ptr in d_cols + d_lk + [d_res]:
                        ctx.free(ptr)
    finally:
        ctx.free(d_vals)


def check_no_results(ctx, kind, cases, spare, below):
    """results_dev = NULL: the same own cells.  The cases one below the other in one column of (their cells + spare) rows, of which all but
    `below` are usable"""
    vals, at = flatten(cases)
    defs = [kind.unit_def(case) for case in cases]
    ncells = len(defs[0][1])
    rows_n = len(cases) * ncells + spare
    units = [kind.unit(0, 2 + j * (ncells + 1), at[j], case) for j, case in enumerate(cases)]
    want = np.tile(SENTINEL, (rows_n, 1))
    for unit, (u, cells, _l) in zip(units, defs):
        own = own_mask(u)
        want[unit[1]:unit[1] + ncells][own] = fr(cells)[own]
    d_col, d_vals = ctx.to_device(np.tile(SENTINEL, (rows_n, 1))), ctx.to_device(fr(vals))
    try:
        kind.fill(ctx, [d_col], rows_n - below, None, d_vals, len(vals), None, 0, units)
        ctx.sync()
        compare(ctx, [d_col], [want], kind.name + " without results")
    finally:
        ctx.free(d_col)
        ctx.free(d_vals)


# ------------------------------------------------------------------------------------------------ column breaks
def break_points(filler, ncells, targets):
    """the break points that put break b on cell targets[b][1] of unit targets[b][0], in a thread of `filler` cells and then units of ncells"""
    idx = [filler + unit * ncells + c for unit, c in targets]
    return [idx[0]] + [b - a for a, b in zip(idx, idx[1:])]


def check_breaks(ctx, kind, cases, targets, filler, usable, ncols):
    """one thread (`filler` plain cells, then the cases as units back to back, each reading operands of its own) laid into ncols columns of
    `usable` rows by virtual_region.assign_witnesses and by the fill from each unit's first cell, from the same break points; for a kind with
    range gaps also the lookup column by LookupAnyManager.assign_raw and by the fill, else the results.  Break b falls on cell targets[b][1]
    of unit targets[b][0]: the cell the case names."""
    th, chip, _ = thread()
    th.advice += list(range(100, 100 + filler))
    th.selector += [False] * filler
    defs = [kind.define(th, chip, case, j) for j, case in enumerate(cases)]
    ncells = defs[0].end - defs[0].start
    assert all(u.end - u.start == ncells for u in defs) and ncells == kind.layout(ctx.lib)[0]
    bps = break_points(filler, ncells, targets)
    total = len(th.advice)
    at = place(0, 0, total, bps, ncols)[0]
    first = first_positions(total, bps, ncols)
    for (unit, c), b, col in zip(targets, bps, range(ncols)):   # the break cell is the cell the case names
        i = filler + unit * ncells + c
        assert (i, col, b) in at and (i, col + 1, 0) in at, (kind.name, unit, c)
    vals, offs = flatten(cases)
    units = [kind.unit(*first[u.start], offs[j], cases[j]) for j, u in enumerate(defs)]
    nlk = 1 if kind.fill_ranges else 0
    rows_n, nres, nunits = usable + 9, kind.nres, len(cases)
    region = VR.Region(rows_n, ncols + nlk)
    VR.assign_witnesses([th], list(range(ncols)), region, bps)
    if nlk:
        chip.lookup_manager.witness_gen_only = True
        chip.lookup_manager.assign_raw([ncols], region)
    want = [np.tile(SENTINEL, (rows_n, 1)) for _ in range(ncols + nlk)]
    for c in range(ncols + nlk):
        rows = sorted(region.advice[c])
        want[c][rows] = fr([region.advice[c][r] for r in rows])
    start = [np.tile(SENTINEL, (rows_n, 1)) for _ in range(ncols + nlk)]
    start[0][:filler] = want[0][:filler]
    d_cols = [ctx.to_device(c) for c in start]
    d_vals = ctx.to_device(fr(vals))
    d_res = ctx.to_device(np.tile(SENTINEL, (nunits * nres + 1, 1)))
    try:
        what = "breaks (%s, cells %s, %d columns)" % (kind.name, [c for _u, c in targets], ncols)
        if nlk:
            kind.fill_ranges(ctx, d_cols[:ncols], usable, bps, d_cols[ncols:], d_vals, len(vals), d_res, nunits * nres, units, [u.queue for u in defs])
            ctx.sync()
            compare(ctx, d_cols, want, what)
        else:
            kind.fill(ctx, d_cols, usable, bps, d_vals, len(vals), d_res, nunits * nres, units)
            ctx.sync()
            compare(ctx, d_cols, want, what)
            compare(ctx, [d_res], [np.concatenate([fr(u.results) for u in defs] + [np.tile(SENTINEL, (1, 1))])], what + " (results)")
    finally:
        for ptr in d_cols + [d_vals, d_res]:
            ctx.free(ptr)


# ------------------------------------------------------------------------------------------------ the refusals
def par(n=88, k_=3, lb=8, p=(1 << 256) - (1 << 32) - 977, flags=0):
    return PL.fp_params(n, k_, lb, p, flags)


# what h2hip_fp_params is refused for by every entry point that takes one: (what, the reason, par's arguments)
FP_PARAMS_REFUSALS = [
    ("flags != 0", "flags", dict(flags=1)),
    ("limb_bits 63", "limb_bits outside", dict(n=63, k_=4, p=(1 << 252) - 1)),
    ("limb_bits 128", "limb_bits outside", dict(n=128, k_=2)),
    ("num_limbs 1", "num_limbs outside", dict(k_=1)),
    ("num_limbs 5", "num_limbs outside", dict(n=64, k_=5)),
    ("n k > 320", "> 320", dict(n=107, k_=3, p=(1 << 320) - 1)),
    ("p == 0", "zero", dict(p=0)),
    ("p < 2^(n (k - 1))", "exactly num_limbs", dict(p=(1 << 176) - 1)),
    ("p >= 2^(n k)", "exactly num_limbs", dict(p=1 << 264)),
    ("quot_max_bits >= n k", "quot_max_bits", dict(p=(1 << 252) - 1)),
    ("a limb of p equal to 1", "equals 1", dict(p=(1 << 255) + (1 << 88) + 12345)),
    ("lookup_bits 0", "lookup_bits", dict(lb=0)),
    ("lookup_bits 64", "lookup_bits", dict(lb=64)),
]


def layout_refused(what, call):
    try:
        call()
    except H.H2HipError as e:
        assert e.code == ERR_INVALID, what
    else:
        raise AssertionError(what + " was accepted")


class RefusalBench:
    """three sentinel columns of n_rows, the operands `vals`, a sentinel results buffer of res_rows; `refused` and the call builders over
    them; the refusals of trace_host.h's fused_fill in terms of the kind: ok and other are the operand offsets of two good units that do not
    share an operand, ncells the kind's cells, lanes the lanes per unit of its placing kernel.  Use as a context manager."""

    def __init__(self, ctx, kind, vals, ok, other, ncells, lanes, res_rows, label=""):
        self.ctx, self.kind, self.vals, self.nv, self.ncells, self.lanes, self.label = ctx, kind, vals, len(vals), ncells, lanes, label
        self.n_rows, self.usable, self.res_rows = 2 * ncells + 60, 2 * ncells + 50, res_rows
        self.ok_ops, self.other_ops, self.ok = ok, other, kind.unit_of(0, 0, *ok)
        self.sent, self.sent_res = np.tile(SENTINEL, (self.n_rows, 1)), np.tile(SENTINEL, (res_rows, 1))
        self.d_cols = [ctx.to_device(self.sent) for _ in range(3)]
        self.d_vals = ctx.to_device(fr(vals))
        self.d_res = ctx.to_device(self.sent_res)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for ptr in self.d_cols + [self.d_vals, self.d_res]:
            self.ctx.free(ptr)

    def over(self, kind, ok, other, ncells, lanes, label):
        """the same buffers for another entry point (they are freed with this bench)"""
        b = copy.copy(self)
        b.kind, b.ok_ops, b.other_ops, b.ok, b.ncells, b.lanes, b.label = kind, ok, other, kind.unit_of(0, 0, *ok), ncells, lanes, label
        return b

    def unit(self, col, row, ops=None):
        return self.kind.unit_of(col, row, *(self.other_ops if ops is None else ops))

    def refused(self, what, reason, call):
        ctx, what = self.ctx, self.label + what
        try:
            call()
        except H.H2HipError as e:
            assert e.code == ERR_INVALID, (what, e.code)
            msg = ctx.lib.h2hip_last_error().decode()
            assert reason in msg, (what, msg)
        else:
            raise AssertionError("%s was accepted" % what)
        ctx.sync()
        for ptr in self.d_cols:
            assert np.array_equal(ctx.download(ptr, (self.n_rows, 4)), self.sent), "%s: a cell was written" % what
        assert np.array_equal(ctx.download(self.d_res, (self.res_rows, 4)), self.sent_res), "%s: a result was written" % what

    def fill(self, units, cols=None, usable_rows=None, bps=None, vdev=None, vlen=None, rdev=None, rlen=None, **changes):
        """the call through the Python wrapper; changes: the kind's params, op, w or nb"""
        kind = self.kind.with_(**changes) if changes else self.kind
        return lambda: kind.fill(self.ctx, self.d_cols if cols is None else cols, self.usable if usable_rows is None else usable_rows, bps,
                                 self.d_vals if vdev is None else vdev, self.nv if vlen is None else vlen, self.d_res if rdev is None else rdev,
                                 self.res_rows if rlen is None else rlen, units)

    def raw(self, columns=True, params=True, values=True, table=True, count=1):
        """the library function itself, over a table of the one unit ok; False: NULL"""
        ctx, kind = self.ctx, self.kind
        cols = (_vp * 3)(*[_vp(int(ptr)) for ptr in self.d_cols])
        tab = C.cast(kind.table([self.ok]), _vp)
        pp = C.cast(C.pointer(kind.params), _vp) if kind.sp is not None else None
        return lambda: ctx._chk(getattr(ctx.lib, kind.entry)(ctx.handle, cols if columns else None, 3, self.usable, None, *kind.head(pp if params else None),
                                                             _vp(int(self.d_vals)) if values else None, self.nv, _vp(int(self.d_res)), self.res_rows,
                                                             *kind.tail(), tab if table else None, count))

    def refuse_nulls(self):
        self.refused("columns NULL", "NULL argument", self.raw(columns=False))
        if self.kind.sp is not None:
            self.refused("params NULL", "NULL argument", self.raw(params=False))
        self.refused("values NULL", "NULL argument", self.raw(values=False))
        self.refused("units NULL", "NULL argument", self.raw(table=False))

    def refuse_params(self, only=None, behind=None):
        """FP_PARAMS_REFUSALS (only: those named), and behind the one `behind` names the module's own: {what: [(what, reason, par's arguments)]}"""
        for what, reason, args in FP_PARAMS_REFUSALS:
            if only is None or what in only:
                self.refused(what, reason, self.fill([self.ok], params=par(**args)))
            for what2, reason2, args2 in (behind or {}).get(what, []):
                self.refused(what2, reason2, self.fill([self.ok], params=par(**args2)))

    def refuse_placement(self):
        ok, usable, ncells, d_cols = self.ok, self.usable, self.ncells, self.d_cols
        self.refused("column index out of range", "column index", self.fill([ok, self.unit(3, 0)]))
        self.refused("a NULL column", "column index", self.fill([ok, self.unit(1, 0)], cols=[d_cols[0], 0, d_cols[2]]))
        self.refused("a run that leaves the usable rows", "usable rows", self.fill([ok, self.unit(1, usable - ncells + 1)]))
        self.refused("a run that leaves the last column", "last column", self.fill([ok, self.unit(2, usable - ncells + 1)], bps=[usable - 1, usable - 1]))
        self.refused("a break point >= usable_rows", "break point", self.fill([ok], bps=[10, usable]))

    def refuse_results_len(self):
        self.refused("results_len too small", "results_len", self.fill([self.ok, self.unit(1, 0)], rlen=2 * self.kind.nres - 1))

    def refuse_count(self):
        self.refused("count times the lanes of a unit > 2^32", "2^32", self.raw(count=(1 << 32) // self.lanes + 1))

    def refuse_overlaps(self, first_gap=None, break_copy=True):
        self.refused("two units' cells overlap", "cells overlap", self.fill([self.ok, self.unit(0, self.ncells - 1)]))
        if first_gap is not None:
            self.refused("a unit inside another's gap", "cells overlap", self.fill([self.ok, self.unit(0, first_gap)]))
        if break_copy:
            self.refused("a break copy inside another unit", "cells overlap",
                         self.fill([self.unit(1, 0, self.ok_ops), self.unit(0, 20)], bps=[25, self.usable - 1]))

    def refuse_aliasing(self, inside):
        """inside: operand offsets that lie in the cells a unit at (1, 0) writes, with column 1 as values_dev"""
        self.refused("an operand inside cells this call writes", "operand range", self.fill([self.unit(1, 0, inside)], vdev=self.d_cols[1], vlen=self.usable))
        self.refused("the results inside cells this call writes", "results overlap",
                     self.fill([self.unit(1, 0, self.ok_ops)], rdev=self.d_cols[1] + 32 * 10, rlen=self.kind.nres))
        self.refused("the results over operands of the call", "operand range", self.fill([self.ok], rdev=self.d_vals, rlen=self.nv))


# ------------------------------------------------------------------------------------------------ entry points refuse alike
ALIKE_CLASSES = ["a break point >= usable_rows", "a run leaving the usable rows", "two units overlapping", "an operand inside written cells",
                 "the results inside written cells", "results_len too small"]


@pytest.fixture(scope="module")
def alike_bench(request):
    """for a test module that names KINDS and NV: a context, the kinds, three sentinel columns long enough for two
    units of the largest kind, NV operands and a sentinel results buffer"""
    from tests.emu_util import emu_context

    ctx = emu_context()
    kinds = request.module.KINDS
    usable = 2 * max(kd.layout(ctx.lib)[0] for kd in kinds) + 50
    sent, sent_res = np.tile(SENTINEL, (usable + 10, 1)), np.tile(SENTINEL, (4 * max(kd.nres for kd in kinds), 1))
    d_cols = [ctx.to_device(sent) for _ in range(3)]
    d_vals, d_res = ctx.to_device(fr(list(range(1, request.module.NV + 1)))), ctx.to_device(sent_res)
    yield ctx, kinds, usable, sent, sent_res, d_cols, d_vals, d_res
    for ptr in d_cols + [d_vals, d_res]:
        ctx.free(ptr)
    ctx.close()


def check_refuse_alike(bench, cls, case):
    """case(kind, cells, usable, d_cols) -> (the substring every entry point's own refusal test looks for, the call's arguments behind the
    columns: (column, row, first operand, second operand) units, break points, values_dev (None: the operands' buffer), values_len,
    results_dev (None: the results buffer), results_len).  Every kind refuses with H2HIP_ERR_INVALID under its own function's name, writes
    nothing, and all give one reason."""
    ctx, kinds, usable, sent, sent_res, d_cols, d_vals, d_res = bench
    reasons = {}
    for kd in kinds:
        reason, (units, bps, vdev, vlen, rdev, rlen) = case(kd, kd.layout(ctx.lib)[0], usable, d_cols)
        with pytest.raises(H.H2HipError) as e:
            kd.fill(ctx, d_cols, usable, bps, d_vals if vdev is None else vdev, vlen, d_res if rdev is None else rdev, rlen, [kd.unit_of(*u) for u in units])
        assert e.value.code == ERR_INVALID, (kd.name, cls, e.value.code)
        msg = ctx.lib.h2hip_last_error().decode()
        head = kd.entry + ": invalid argument: "
        assert msg.startswith(head) and reason in msg, (kd.name, cls, msg)
        reasons[kd.name] = msg[len(head):]
        ctx.sync()
        for ptr in d_cols:
            assert np.array_equal(ctx.download(ptr, sent.shape), sent), "%s, %s: a cell was written" % (kd.name, cls)
        assert np.array_equal(ctx.download(d_res, sent_res.shape), sent_res), "%s, %s: a result was written" % (kd.name, cls)
    assert len(reasons) == len(kinds) and len(set(reasons.values())) == 1, (cls, reasons)


# ------------------------------------------------------------------------------------------------ the names in every layer
def check_names(constants=(), functions=(), structs=(), mirrored=()):
    """constants [(name, the Python value)]: the header's #define and the Rust sys crate's const equal it; functions: declared in the header and
    the sys crate, exported by the library; structs [(name, the ctypes class, bytes)]: the same fields of the same types in all three;
    mirrored: functions also named in the C++ mirror and the safe Rust wrapper"""
    hdr = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    rs = open(os.path.join(ROOT, "ffi", "rust", "h2hip-sys", "src", "lib.rs")).read()
    for name, py in constants:
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == py == int(re.search(r"pub const %s: u32 = (\d+);" % name, rs).group(1)), name
    lib = H.load_library()
    for fn in functions:
        assert ("int %s(" % fn) in hdr and ("pub fn %s(" % fn) in rs and hasattr(lib, fn), fn
    cmap = {"uint32_t": "u32", "uint64_t": "u64", "uint8_t": "u8"}
    pymap = {C.c_uint32: "u32", C.c_uint64: "u64"}
    for name, py, size in structs:
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s\s*;" % (name, name), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        c_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                ty, names = decl.split(None, 1)
                for nm in names.split(","):
                    arr = re.fullmatch(r"(\w+)\[(\d+)\]", nm.strip())
                    c_fields.append((arr.group(1), "[%s; %s]" % (cmap[ty], arr.group(2))) if arr else (nm.strip(), cmap[ty]))
        rs_body = re.search(r"pub struct %s\s*\{(.*?)\}" % name, rs, flags=re.S).group(1)
        rs_fields = re.findall(r"pub ([a-z_]+): (\[[a-z0-9]+; \d+\]|[a-z0-9]+)", rs_body)
        py_fields = [(nm, pymap[ty] if ty in pymap else "[u8; %d]" % ty._length_) for nm, ty in py._fields_]
        assert c_fields == rs_fields == py_fields, (name, c_fields, rs_fields, py_fields)
        assert C.sizeof(py) == size, name
    for layer in ("halo2-lib_amd/host/halo2_proofs.hpp", "ffi/rust/h2hip-sys/src/safe.rs"):
        src = open(os.path.join(ROOT, layer)).read()
        for fn in mirrored:
            assert fn in src, (layer, fn)


# ------------------------------------------------------------------------------------------------ inside a proof
class ProofBench:
    """a BaseConfig circuit at 2^kk rows built twice through the Context mirror by program(builder) (for the key, then with the key's break
    points for the witness), over as many gate columns as the layout fills, starting from num_advice; keygen from the mirror's selectors
    and copies.  calls is what program returned, first[i] the (column, row) of thread cell i.  buffers() makes the device columns, check_*
    are the proof's checks.  Use as a context manager."""

    def __init__(self, ctx, kk, nl, lb, seed, program, num_advice=12):
        self.ctx, self.seed, self.nl, self.n = ctx, seed, nl, 1 << kk
        na = num_advice
        while True:                                        # the number of gate columns the layout fills (an empty one would have a disjoint selector)
            sh = P.Shape(kk, na, nl, 1, 1, lb)
            kb = VR.BaseCircuitBuilder(False)
            program(kb)
            advice_k, fixed, copies, instances, bps = kb.synthesize(sh)
            if len(bps) == na - 1:
                break
            na = len(bps) + 1
        assert na >= 2 and len(bps) >= 1
        pb = VR.BaseCircuitBuilder(True)
        pb.break_points = bps
        self.calls = program(pb)
        advice, _, _, _, _ = pb.synthesize(sh)
        assert all(np.array_equal(a, b) for a, b in zip(advice, advice_k))
        self.sh, self.na, self.bps, self.advice, self.fixed, self.copies, self.instances = sh, na, bps, advice, fixed, copies, instances
        self.first = first_positions(sum(len(t.advice) for t in pb.threads), bps, na)
        self.d_gate = self.d_lookup = self.gpk = self.kzg = None
        self.kzg, self.srs_params = srs(ctx, kk, seed)
        self.gpk = PL.keygen(self.kzg, PL.BaseCircuitParams.new(kk, na, nl, 1, 1, lb), fixed, copies)
        self.budget = rng_budget(sh)

    def buffers(self, extra, loaded):
        """one device buffer [gate columns][extra elements for the calls' results], zero but for the loaded witnesses (ranges of flat indices
        of the gate allocation, which must lie in column 0 at their index), and the zeroed lookup columns -> the index of the first extra element"""
        ctx, n, na = self.ctx, self.n, self.na
        self.host = np.zeros((na * n + extra, 4), dtype=np.uint64)
        for rng in loaded:
            assert all(self.first[i] == (0, i) for i in rng)
            self.host[rng.start:rng.stop] = self.advice[0][rng.start:rng.stop]
        self.d_gate = ctx.to_device(self.host)
        self.d_lookup = ctx.to_device(np.zeros((self.nl * n, 4), dtype=np.uint64))
        self.d_cols = [self.d_gate + 32 * n * c for c in range(na)]
        self.d_lks = [self.d_lookup + 32 * n * c for c in range(self.nl)]
        return na * n

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for ptr in (self.d_gate, self.d_lookup):
            if ptr is not None:
                self.ctx.free(ptr)
        self.gpk.free()
        self.kzg.free()

    def cell(self, i):
        c, r = self.first[i]
        return ints(self.advice[c][r:r + 1])[0]

    def check_columns(self):
        got = np.concatenate([self.ctx.download(self.d_gate, (self.na, self.n, 4)), self.ctx.download(self.d_lookup, (self.nl, self.n, 4))])
        for c in range(self.na + self.nl):
            assert np.array_equal(got[c], self.advice[c]), "advice column %d differs from the Python-computed advice" % c

    def check_witness(self, **kw):
        return PL.check_witness(self.gpk, self.d_cols + self.d_lks, self.instances, advice_on_device=True, **kw)

    def changed(self, i, **kw):
        """thread cell i changed by one on the device -> check_witness's report; the cell is put back"""
        c, r = self.first[i]
        self.ctx.upload(self.d_cols[c] + 32 * r, fr([(ints(self.advice[c][r:r + 1])[0] + 1) % R]))
        report = self.check_witness(max_failures=64, **kw)
        self.ctx.upload(self.d_cols[c] + 32 * r, self.advice[c][r:r + 1])
        return report

    def check_proof(self, host=True, oracle=False):
        """the proof over the device-filled columns has the bytes of the proof over the Python-computed advice (host) and of the oracle
        prover's (oracle); both verifiers accept it; check_witness finds nothing"""
        rng = lambda: PreDrawnRng(self.budget, 2000 + self.seed)
        if host:
            want = PL.create_proof(self.gpk, self.advice, self.instances, rng())
        got = PL.create_proof(self.gpk, self.d_cols + self.d_lks, self.instances, rng(), advice_on_device=True)
        assert not host or got == want, "the proof over the device-filled trace differs from the one over the Python-computed advice"
        inst = [ints(v) for v in self.instances]
        if oracle:
            asm = P.PermutationAssembly(self.sh)
            for l, r in self.copies:
                asm.copy(l, r)
            opk = P.keygen(self.srs_params, self.sh, self.fixed, asm, 2)
            assert got == P.create_proof(self.srs_params, opk, self.advice, inst, rng(), 2), "the proof differs from the oracle prover's over the host-laid trace"
        assert PL.verify_proof(self.gpk, self.instances, got), "h2hip_plonk_verify_proof rejects the proof"
        assert P.verify_proof(self.srs_params, vk_from_gpu(self.sh, self.gpk), inst, got), "the test verifier rejects the proof"
        total_f, fails = self.check_witness()
        assert total_f == 0, fails
