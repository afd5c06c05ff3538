"""The refusals the fused fills share (trace_host.h's fused_fill), on the CPU-emulated build: h2hip_fp_mul_fill_dev, h2hip_ec_fill_dev and
h2hip_fp_cmp_fill_dev given the same bad argument refuse with H2HIP_ERR_INVALID and the same reason, and write nothing.  Every refusal
of each entry point on its own is in the check modules (fp_mul_checks, ec_fill_checks, ec_strict_checks: check_rejections)."""
import numpy as np
import pytest

import halo2_lib_amd as H
from halo2_lib_amd import plonk as PL
from tests import ec_fill_checks as E
from tests import fp_mul_checks as F
from tests.fp_mul_checks import ERR_INVALID, SENTINEL, fr

SP = F.Spec(88, 3, 8, F.SECP_P)
NV = 32   # elements of the operands' buffer: three points of 2 (k + 1)


class Kind:
    """one entry point: its call, and its unit's cells, results and operand length (the step between operands that do not overlap)"""

    def __init__(self, name, fill, layout, results, operand):
        self.name, self.fill, self.cells, self.results, self.operand = name, fill, layout.num_cells, results, operand


def kinds(lib):
    p, k = SP.params(), SP.k
    cmp_lay = PL.fp_cmp_layout(p, 7, lib)
    return [Kind("h2hip_fp_mul_fill_dev", lambda ctx, cols, usable, bps, *a: PL.fp_mul_fill(ctx, cols, usable, bps, p, *a), PL.fp_mul_layout(p, lib), 3 * k + 1, k + 1),
            Kind("h2hip_ec_fill_dev", lambda ctx, cols, usable, bps, *a: PL.ec_fill(ctx, cols, usable, bps, p, E.ADD, *a), PL.ec_layout(p, E.ADD, lib), 9 * k + 3,
                 2 * (k + 1)),
            Kind("h2hip_fp_cmp_fill_dev", lambda ctx, cols, usable, bps, *a: PL.fp_cmp_fill(ctx, cols, usable, bps, p, 7, *a), cmp_lay, cmp_lay.results_per_unit, k + 1)]


@pytest.fixture(scope="module")
def bench():
    """a context, three sentinel columns long enough for two units of the largest kind, the operands and a sentinel results buffer"""
    from tests.emu_util import emu_context

    ctx = emu_context()
    ks = kinds(ctx.lib)
    usable = 2 * max(kd.cells for kd in ks) + 50
    sent, sent_res = np.tile(SENTINEL, (usable + 10, 1)), np.tile(SENTINEL, (4 * max(kd.results for kd in ks), 1))
    d_cols = [ctx.to_device(sent) for _ in range(3)]
    d_vals, d_res = ctx.to_device(fr(list(range(1, NV + 1)))), ctx.to_device(sent_res)
    yield ctx, ks, usable, sent, sent_res, d_cols, d_vals, d_res
    for ptr in d_cols + [d_vals, d_res]:
        ctx.free(ptr)
    ctx.close()


# class -> (the substring every entry point's own refusal test looks for, kind -> the call's arguments behind the columns: units, break
# points, values_dev (None: the operands' buffer), values_len, results_dev (None: the results buffer), results_len)
def _cases(kd, usable, d_cols):
    ol, ok = kd.operand, (0, 0, 0, kd.operand)
    return {
        "a break point >= usable_rows": ("break point", ([ok], [10, usable], None, NV, None, 4 * kd.results)),
        "a run leaving the usable rows": ("usable rows", ([ok, (1, usable - kd.cells + 1, ol, 2 * ol)], None, None, NV, None, 4 * kd.results)),
        "two units overlapping": ("cells overlap", ([ok, (0, kd.cells - 1, ol, 2 * ol)], None, None, NV, None, 4 * kd.results)),
        "an operand inside written cells": ("operand range", ([(1, 0, 5, 30)], None, d_cols[1], usable, None, 4 * kd.results)),
        "the results inside written cells": ("results overlap", ([(1, 0, 0, ol)], None, None, NV, d_cols[1] + 32 * 10, kd.results)),
        "results_len too small": ("results_len", ([ok, (1, 0, ol, 2 * ol)], None, None, NV, None, 2 * kd.results - 1)),
    }


CLASSES = ["a break point >= usable_rows", "a run leaving the usable rows", "two units overlapping", "an operand inside written cells",
           "the results inside written cells", "results_len too small"]


@pytest.mark.parametrize("cls", CLASSES)
def test_the_three_fused_fills_refuse_alike(bench, cls):
    ctx, ks, usable, sent, sent_res, d_cols, d_vals, d_res = bench
    reasons = {}
    for kd in ks:
        reason, (units, bps, vdev, vlen, rdev, rlen) = _cases(kd, usable, d_cols)[cls]
        with pytest.raises(H.H2HipError) as e:
            kd.fill(ctx, d_cols, usable, bps, d_vals if vdev is None else vdev, vlen, d_res if rdev is None else rdev, rlen, units)
        assert e.value.code == ERR_INVALID, (kd.name, cls, e.value.code)
        msg = ctx.lib.h2hip_last_error().decode()
        head = kd.name + ": invalid argument: "
        assert msg.startswith(head) and reason in msg, (kd.name, cls, msg)
        reasons[kd.name] = msg[len(head):]
        ctx.sync()
        for ptr in d_cols:
            assert np.array_equal(ctx.download(ptr, sent.shape), sent), "%s, %s: a cell was written" % (kd.name, cls)
        assert np.array_equal(ctx.download(d_res, sent_res.shape), sent_res), "%s, %s: a result was written" % (kd.name, cls)
    assert len(set(reasons.values())) == 1, (cls, reasons)
