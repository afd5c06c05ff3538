"""The refusals the fused fills share (trace_host.h's fused_fill) applied to the fourth fused entry point, on the CPU-emulated build:
h2hip_ec_select_fill_dev, for both of its ops, given the bad argument of each class of tests/test_fused_fill_refusals.py refuses with
H2HIP_ERR_INVALID and the reason h2hip_ec_fill_dev gives for it, and writes nothing.  Every refusal of the entry point on its own is in
tests/ec_select_checks.py (check_rejections)."""
import pytest

from halo2_lib_amd import plonk as PL
from tests import fp_mul_checks as F
from tests.fused_fill_harness import ALIKE_CLASSES, EcOp, FromBits, Select, alike_bench, check_refuse_alike   # noqa: F401 (alike_bench is a fixture)

SP = F.Spec(88, 3, 8, F.SECP_P)
NV = 48   # elements of the operands' buffer: six points of 2 (k + 1)
PT = 2 * (SP.k + 1)
# the curve operation as the yardstick, then the two selections (a selection from bits at w = 1: the table at the first operand, its bit at
# the second)
KINDS = [EcOp(SP, PL.EC_ADD_UNEQUAL), Select(SP), FromBits(SP, 1)]


def _case(cls, kd, cells, usable, d_cols):
    ol, ok = 2 * PT, (0, 0, 0, 2 * PT)
    return {
        "a break point >= usable_rows": ("break point", ([ok], [10, usable], None, NV, None, 4 * kd.nres)),
        "a run leaving the usable rows": ("usable rows", ([ok, (1, usable - cells + 1, PT, ol)], None, None, NV, None, 4 * kd.nres)),
        "two units overlapping": ("cells overlap", ([ok, (0, cells - 1, PT, ol)], None, None, NV, None, 4 * kd.nres)),
        "an operand inside written cells": ("operand range", ([(1, 0, usable - 40, 5)], None, d_cols[1], usable, None, 4 * kd.nres)),
        "the results inside written cells": ("results overlap", ([(1, 0, 0, ol)], None, None, NV, d_cols[1] + 32 * 10, kd.nres)),
        "results_len too small": ("results_len", ([ok, (1, 0, PT, ol)], None, None, NV, None, 2 * kd.nres - 1)),
    }[cls]


@pytest.mark.parametrize("cls", ALIKE_CLASSES)
def test_the_selections_refuse_as_the_curve_operation_does(alike_bench, cls):
    check_refuse_alike(alike_bench, cls, lambda *a: _case(cls, *a))
