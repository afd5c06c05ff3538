"""The refusals the fused fills share (trace_host.h's fused_fill) applied to the fourth fused entry point, on the CPU-emulated build:
h2hip_ec_select_fill_dev, for both of its ops, given the bad argument of each class of tests/test_fused_fill_refusals.py refuses with
H2HIP_ERR_INVALID and the reason h2hip_ec_fill_dev gives for it, and writes nothing.  Every refusal of the entry point on its own is in
tests/ec_select_checks.py (check_rejections)."""
import numpy as np
import pytest

import halo2_lib_amd as H
from halo2_lib_amd import plonk as PL
from tests import ec_fill_checks as E
from tests import fp_mul_checks as F
from tests.fp_mul_checks import ERR_INVALID, SENTINEL, fr

SP = F.Spec(88, 3, 8, F.SECP_P)
NV = 48   # elements of the operands' buffer: six points of 2 (k + 1)
PT = 2 * (SP.k + 1)
CLASSES = ["a break point >= usable_rows", "a run leaving the usable rows", "two units overlapping", "an operand inside written cells",
           "the results inside written cells", "results_len too small"]


def entry_points(lib):
    """(name, fill taking (column, row, first operand, second operand) units, cells, results): the curve operation as the yardstick, then the
    two selections (a selection from bits at w = 1: the table at the first operand, its bit at the second)"""
    p = SP.params()
    sel = lambda op, w, to5: (lambda ctx, cols, usable, bps, *a: PL.ec_select_fill(ctx, cols, usable, bps, p, op, w, *a[:-1], [to5(*u) for u in a[-1]]))
    return [("h2hip_ec_fill_dev", lambda ctx, cols, usable, bps, *a: PL.ec_fill(ctx, cols, usable, bps, p, E.ADD, *a), PL.ec_layout(p, E.ADD, lib).num_cells, 9 * SP.k + 3),
            ("h2hip_ec_select_fill_dev", sel(PL.EC_SELECT, 0, lambda c, r, a, b: (c, r, a, b, 0)), PL.ec_select_layout(p, PL.EC_SELECT, 0, lib).num_cells, PT),
            ("h2hip_ec_select_fill_dev", sel(PL.EC_SELECT_FROM_BITS, 1, lambda c, r, a, b: (c, r, a, 0, b)),
             PL.ec_select_layout(p, PL.EC_SELECT_FROM_BITS, 1, lib).num_cells, PT)]


@pytest.fixture(scope="module")
def bench():
    from tests.emu_util import emu_context

    ctx = emu_context()
    eps = entry_points(ctx.lib)
    usable = 2 * max(e[2] for e in eps) + 50
    sent, sent_res = np.tile(SENTINEL, (usable + 10, 1)), np.tile(SENTINEL, (4 * max(e[3] for e in eps), 1))
    d_cols = [ctx.to_device(sent) for _ in range(3)]
    d_vals, d_res = ctx.to_device(fr(list(range(1, NV + 1)))), ctx.to_device(sent_res)
    yield ctx, eps, usable, sent, sent_res, d_cols, d_vals, d_res
    for ptr in d_cols + [d_vals, d_res]:
        ctx.free(ptr)
    ctx.close()


def _case(cls, cells, results, usable, d_cols):
    """the call's arguments behind the columns: units, break points, values_dev (None: the operands' buffer), values_len, results_dev (None:
    the results buffer), results_len -- and the substring the entry points' own refusal tests look for"""
    ol, ok = 2 * PT, (0, 0, 0, 2 * PT)
    return {
        "a break point >= usable_rows": ("break point", ([ok], [10, usable], None, NV, None, 4 * results)),
        "a run leaving the usable rows": ("usable rows", ([ok, (1, usable - cells + 1, PT, ol)], None, None, NV, None, 4 * results)),
        "two units overlapping": ("cells overlap", ([ok, (0, cells - 1, PT, ol)], None, None, NV, None, 4 * results)),
        "an operand inside written cells": ("operand range", ([(1, 0, usable - 40, 5)], None, d_cols[1], usable, None, 4 * results)),
        "the results inside written cells": ("results overlap", ([(1, 0, 0, ol)], None, None, NV, d_cols[1] + 32 * 10, results)),
        "results_len too small": ("results_len", ([ok, (1, 0, PT, ol)], None, None, NV, None, 2 * results - 1)),
    }[cls]


@pytest.mark.parametrize("cls", CLASSES)
def test_the_selections_refuse_as_the_curve_operation_does(bench, cls):
    ctx, eps, usable, sent, sent_res, d_cols, d_vals, d_res = bench
    reasons = []
    for name, fill, cells, results in eps:
        reason, (units, bps, vdev, vlen, rdev, rlen) = _case(cls, cells, results, usable, d_cols)
        with pytest.raises(H.H2HipError) as e:
            fill(ctx, d_cols, usable, bps, d_vals if vdev is None else vdev, vlen, d_res if rdev is None else rdev, rlen, units)
        assert e.value.code == ERR_INVALID, (name, cls, e.value.code)
        msg = ctx.lib.h2hip_last_error().decode()
        head = name + ": invalid argument: "
        assert msg.startswith(head) and reason in msg, (name, cls, msg)
        reasons.append(msg[len(head):])
        ctx.sync()
        for ptr in d_cols:
            assert np.array_equal(ctx.download(ptr, sent.shape), sent), "%s, %s: a cell was written" % (name, cls)
        assert np.array_equal(ctx.download(d_res, sent_res.shape), sent_res), "%s, %s: a result was written" % (name, cls)
    assert len(set(reasons)) == 1, (cls, reasons)
