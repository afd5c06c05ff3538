"""The curve arithmetic of a strict MSM trace filled on the GPU (h2hip_ec_fill_dev with SUB_UNEQUAL, h2hip_fp_cmp_fill_dev,
plonk.ec_fill_strict_with_ranges): the checks of tests/ec_strict_checks.py, and unit counts around the workgroup sizes of both kernels of
both fills (one lane per unit, SOLVE_BLOCK lanes per workgroup; one lane per (unit, segment), PLACE_BLOCK lanes per workgroup)."""
import pytest

import halo2_lib_amd as H
from tests import ec_fill_checks as K
from tests import ec_strict_checks as S

pytestmark = pytest.mark.gpu
IDS = ["%d_%d_%d" % p for p in S.PARAMS]


@pytest.fixture(scope="module")
def ctx():
    c = H.Context()
    yield c
    c.close()


@pytest.mark.parametrize("modulus", sorted(S.MODULI))
@pytest.mark.parametrize("n,k,lb", S.PARAMS, ids=IDS)
def test_sub_unequal_against_its_definition(ctx, n, k, lb, modulus):
    S.check_sub_fill(ctx, n, k, lb, modulus, 5)


@pytest.mark.parametrize("mask", S.MASKS)
@pytest.mark.parametrize("modulus", sorted(S.MODULI))
@pytest.mark.parametrize("n,k,lb", S.PARAMS, ids=IDS)
def test_comparison_against_its_definition(ctx, n, k, lb, modulus, mask):
    S.check_cmp_fill(ctx, n, k, lb, modulus, mask, 7)


@pytest.mark.parametrize("n,k,lb", S.PARAMS, ids=IDS)
def test_one_unit_per_call(ctx, n, k, lb):
    sp = S.Spec(n, k, lb, S.SECP_P)
    pool = S.sub_pool(sp, "secp256k1_p")
    S.check_sub_fill(ctx, n, k, lb, "secp256k1_p", 1, pool=pool[:2] + pool[6:10] + pool[-3:])
    pool = S.cmp_pool(sp)
    for mask in (3, 4, 7):
        S.check_cmp_fill(ctx, n, k, lb, "secp256k1_p", mask, 1, pool=pool[2:5] + pool[-4:])


@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_lookup_cells_over_two_columns(ctx, n, k, lb):
    S.check_sub_fill(ctx, n, k, lb, "secp256k1_n", 5, nl=2)
    for mask in (2, 7):
        S.check_cmp_fill(ctx, n, k, lb, "secp256k1_n", mask, 5, nl=2)


@pytest.mark.parametrize("count", [S.SOLVE_BLOCK - 1, S.SOLVE_BLOCK, S.SOLVE_BLOCK + 1], ids=["one_before", "on_the_edge", "one_past"])
def test_units_around_the_solving_workgroup(ctx, count):
    S.check_sub_fill(ctx, 88, 3, 18, "secp256k1_p", count)
    S.check_cmp_fill(ctx, 88, 3, 18, "secp256k1_p", 7, count)


def _edge_count(slots, edge):
    """the unit count whose lanes (count times the unit's segments) end `edge` lanes past a workgroup edge, past the first workgroup"""
    count = edge * pow(slots, -1, S.PLACE_BLOCK) % S.PLACE_BLOCK or S.PLACE_BLOCK
    if count * slots <= S.PLACE_BLOCK:
        count += S.PLACE_BLOCK
    assert (count * slots - edge) % S.PLACE_BLOCK == 0 and count * slots > S.PLACE_BLOCK
    return count


@pytest.mark.parametrize("edge", [-1, 0, 1], ids=["one_lane_before", "on_the_edge", "one_lane_past"])
def test_units_around_the_placing_workgroup(ctx, edge):
    """SUB_UNEQUAL has ADD_UNEQUAL's segments (an odd number); the comparison of mask 7 has 5 k = 15, the one of mask 5 has 3 k = 9"""
    S.check_sub_fill(ctx, 88, 3, 8, "secp256k1_p", _edge_count(K.segments(3, K.ADD), edge))
    for mask in (7, 5):
        S.check_cmp_fill(ctx, 88, 3, 8, "secp256k1_p", mask, _edge_count(S.cmp_segments(3, mask), edge))


@pytest.mark.parametrize("mask", [4, 5, 6, 7])
@pytest.mark.parametrize("op", ["add_unequal", "sub_unequal"])
def test_strict_operation_in_two_fused_calls(ctx, op, mask):
    S.check_strict(ctx, 88, 3, 8, {"add_unequal": S.ADD, "sub_unequal": S.SUB}[op], mask)


def test_strict_operation_with_four_limbs(ctx):
    S.check_strict(ctx, 64, 4, 8, S.SUB, 7, count=3)


@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_strict_addition_reads_a_subtractions_results(ctx, n, k, lb):
    S.check_chained(ctx, n, k, lb)


@pytest.mark.parametrize("ncols", [2, 3])
@pytest.mark.parametrize("case", S.BREAK_CASES)
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case, ncols):
    S.check_strict_breaks(ctx, case, ncols)


def test_rejections(ctx):
    S.check_rejections(ctx)


def test_msm_fragment_inside_a_proof(ctx):
    S.check_proof(ctx, 11, seed=97, nl=2)


def test_equal_x_is_caught_by_the_pinned_equality_cell(ctx):
    S.check_proof(ctx, 11, seed=97, nl=2, mode="equal_x")
