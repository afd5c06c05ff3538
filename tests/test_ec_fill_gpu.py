"""EccChip's ec_add_unequal and ec_double filled on the GPU (h2hip_ec_fill_dev): the checks of tests/ec_fill_checks.py, and unit counts
around the workgroup sizes of both kernels (one lane per unit, SOLVE_BLOCK lanes per workgroup; one lane per (unit, segment), PLACE_BLOCK
lanes per workgroup)."""
import pytest

import halo2_lib_amd as H
from tests import ec_fill_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = H.Context()
    yield c
    c.close()


@pytest.mark.parametrize("op", sorted(K.OPS))
@pytest.mark.parametrize("modulus", sorted(K.MODULI))
@pytest.mark.parametrize("n,k,lb", K.PARAMS, ids=["%d_%d_%d" % p for p in K.PARAMS])
def test_fill_against_its_definition(ctx, n, k, lb, modulus, op):
    K.check_op_fill(ctx, n, k, lb, modulus, K.OPS[op], 5)


@pytest.mark.parametrize("op", sorted(K.OPS))
@pytest.mark.parametrize("n,k,lb", K.PARAMS, ids=["%d_%d_%d" % p for p in K.PARAMS])
def test_one_unit_per_call(ctx, n, k, lb, op):
    sp = K.Spec(n, k, lb, K.SECP_P)
    pool = K.operand_pool(sp, "secp256k1_p")
    K.check_op_fill(ctx, n, k, lb, "secp256k1_p", K.OPS[op], 1, pool=pool[:2] + pool[6:10] + pool[-3:])


@pytest.mark.parametrize("op", sorted(K.OPS))
@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_lookup_cells_over_two_columns(ctx, n, k, lb, op):
    K.check_op_fill(ctx, n, k, lb, "secp256k1_n", K.OPS[op], 5, nl=2)


def test_reductions_with_different_carry_widths(ctx):
    K.check_three_carry_widths(ctx)


@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_points_read_from_a_previous_calls_results(ctx, n, k, lb):
    K.check_chained(ctx, n, k, lb)


@pytest.mark.parametrize("op", sorted(K.OPS))
@pytest.mark.parametrize("count", [K.SOLVE_BLOCK - 1, K.SOLVE_BLOCK, K.SOLVE_BLOCK + 1], ids=["one_before", "on_the_edge", "one_past"])
def test_units_around_the_solving_workgroup(ctx, count, op):
    K.check_op_fill(ctx, 88, 3, 18, "secp256k1_p", K.OPS[op], count)


@pytest.mark.parametrize("op", sorted(K.OPS))
@pytest.mark.parametrize("edge", [-1, 0, 1], ids=["one_lane_before", "on_the_edge", "one_lane_past"])
def test_units_around_the_placing_workgroup(ctx, edge, op):
    """the unit count whose lanes (count times the unit's segments, an odd number) end one lane before, on and one lane past a workgroup edge"""
    slots = K.segments(3, K.OPS[op])
    count = edge * pow(slots, -1, K.PLACE_BLOCK) % K.PLACE_BLOCK or K.PLACE_BLOCK
    assert (count * slots - edge) % K.PLACE_BLOCK == 0 and count * slots > K.PLACE_BLOCK
    K.check_op_fill(ctx, 88, 3, 8, "secp256k1_p", K.OPS[op], count)


@pytest.mark.parametrize("ncols", [2, 3])
@pytest.mark.parametrize("case", K.BREAK_CASES)
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case, ncols):
    K.check_op_breaks(ctx, case, ncols)


def test_rejections(ctx):
    K.check_rejections(ctx)


def test_curve_operations_inside_a_proof(ctx):
    K.check_proof(ctx, 11, seed=93, nl=2)


def test_equal_x_with_different_y_inside_a_circuit(ctx):
    K.check_proof(ctx, 11, seed=93, nl=2, mode="equal_x")
