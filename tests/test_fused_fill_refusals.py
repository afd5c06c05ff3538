"""The refusals the fused fills share (trace_host.h's fused_fill), on the CPU-emulated build: h2hip_fp_mul_fill_dev, h2hip_ec_fill_dev and
h2hip_fp_cmp_fill_dev given the same bad argument refuse with H2HIP_ERR_INVALID and the same reason, and write nothing.  Every refusal
of each entry point on its own is in the check modules (fp_mul_checks, ec_fill_checks, ec_strict_checks: check_rejections)."""
import pytest

from halo2_lib_amd import plonk as PL
from tests import fp_mul_checks as F
from tests.fused_fill_harness import ALIKE_CLASSES, Cmp, EcOp, FpMul, alike_bench, check_refuse_alike   # noqa: F401 (alike_bench is a fixture)

SP = F.Spec(88, 3, 8, F.SECP_P)
NV = 32   # elements of the operands' buffer: three points of 2 (k + 1)
KINDS = [FpMul(SP), EcOp(SP, PL.EC_ADD_UNEQUAL), Cmp(SP, 7)]


def _case(cls, kd, cells, usable, d_cols):
    """ol: the kind's operand length, the step between operands that do not overlap"""
    ol = {"fp_mul": SP.k + 1, "add_unequal": 2 * (SP.k + 1), "cmp mask 7": SP.k + 1}[kd.name]
    ok = (0, 0, 0, ol)
    return {
        "a break point >= usable_rows": ("break point", ([ok], [10, usable], None, NV, None, 4 * kd.nres)),
        "a run leaving the usable rows": ("usable rows", ([ok, (1, usable - cells + 1, ol, 2 * ol)], None, None, NV, None, 4 * kd.nres)),
        "two units overlapping": ("cells overlap", ([ok, (0, cells - 1, ol, 2 * ol)], None, None, NV, None, 4 * kd.nres)),
        "an operand inside written cells": ("operand range", ([(1, 0, 5, 30)], None, d_cols[1], usable, None, 4 * kd.nres)),
        "the results inside written cells": ("results overlap", ([(1, 0, 0, ol)], None, None, NV, d_cols[1] + 32 * 10, kd.nres)),
        "results_len too small": ("results_len", ([ok, (1, 0, ol, 2 * ol)], None, None, NV, None, 2 * kd.nres - 1)),
    }[cls]


@pytest.mark.parametrize("cls", ALIKE_CLASSES)
def test_the_three_fused_fills_refuse_alike(alike_bench, cls):
    check_refuse_alike(alike_bench, cls, lambda *a: _case(cls, *a))
