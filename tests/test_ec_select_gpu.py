"""Point selections and scalar bits of an MSM trace filled on the GPU (h2hip_ec_select_fill_dev, h2hip_num_to_bits_fill_dev): the checks of
tests/ec_select_checks.py, and unit counts around the workgroup sizes of the three kernels (one lane per unit, SOLVE_BLOCK lanes per
workgroup; one lane per (unit, segment), PLACE_BLOCK lanes per workgroup; one lane per (unit, bit), BITS_BLOCK lanes per workgroup)."""
import pytest

import halo2_lib_amd as H
from tests import ec_select_checks as S

pytestmark = pytest.mark.gpu
IDS = ["%d_%d_%d" % p for p in S.PARAMS]
WINDOWED = [(n, k, lb, w) for n, k, lb in S.PARAMS for w in S.WINDOWS[k]]
EDGES = pytest.mark.parametrize("edge", [-1, 0, 1], ids=["one_lane_before", "on_the_edge", "one_lane_past"])


@pytest.fixture(scope="module")
def ctx():
    c = H.Context()
    yield c
    c.close()


def test_layouts_equal_the_definition(ctx):
    S.check_layouts(ctx)


@pytest.mark.parametrize("modulus", sorted(S.MODULI))
@pytest.mark.parametrize("n,k,lb", S.PARAMS, ids=IDS)
def test_select_against_its_definition(ctx, n, k, lb, modulus):
    S.check_select_fill(ctx, n, k, lb, modulus)


@pytest.mark.parametrize("modulus", sorted(S.MODULI))
@pytest.mark.parametrize("n,k,lb,w", WINDOWED, ids=["%d_%d_%d_w%d" % p for p in WINDOWED])
def test_select_from_bits_against_its_definition(ctx, n, k, lb, w, modulus):
    S.check_from_bits_fill(ctx, n, k, lb, modulus, w)


@pytest.mark.parametrize("nb", S.NUM_BITS)
def test_num_to_bits_against_its_definition(ctx, nb):
    S.check_bits_fill(ctx, nb)


def test_one_unit_per_call_and_no_results(ctx):
    sp = S.Spec(88, 3, 8, S.SECP_P)
    S.check_select_fill(ctx, 88, 3, 8, "secp256k1_p", 1, pool=S.select_pool(sp, "secp256k1_p")[:3])
    S.check_from_bits_fill(ctx, 88, 3, 8, "secp256k1_p", 2, 1, pool=S.from_bits_pool(sp, 2, "secp256k1_p")[:3])
    S.check_bits_fill(ctx, 5, 1, pool=S.bits_pool(5)[2:5])
    S.check_no_results(ctx)


@pytest.mark.parametrize("count", [S.SOLVE_BLOCK - 1, S.SOLVE_BLOCK, S.SOLVE_BLOCK + 1], ids=["one_before", "on_the_edge", "one_past"])
def test_units_around_the_solving_workgroup(ctx, count):
    """ec_select has 2 (k + 1) = 8 lanes per unit in the placing kernel, so its lanes end on a workgroup edge only at multiples of 32 units and
    never one lane off it: 63, 64 and 65 units are also one unit before, on and one unit past the placing kernel's second edge"""
    S.check_select_fill(ctx, 88, 3, 18, "secp256k1_p", count)
    S.check_from_bits_fill(ctx, 88, 3, 18, "secp256k1_p", 2, count)


@EDGES
def test_units_around_the_placing_workgroup(ctx, edge):
    """a selection from bits has 2^w - 1 + 2 (chains pieces (+ 1)) segments, an odd number: 9 at (3, 1), 17 at (3, 2)"""
    for w in (1, 2):
        S.check_from_bits_fill(ctx, 88, 3, 8, "secp256k1_p", w, S.edge_count(S.from_bits_segments(3, w), edge))


@EDGES
def test_units_around_the_bits_workgroup(ctx, edge):
    S.check_bits_fill(ctx, 5, S.edge_count(5, edge, S.BITS_BLOCK))


@pytest.mark.parametrize("ncols", [2, 3])
@pytest.mark.parametrize("name,case", S.BREAK_CASES, ids=["%s-%s" % c for c in S.BREAK_CASES])
def test_column_breaks_as_assign_witnesses_makes_them(ctx, name, case, ncols):
    if case == "two" and ncols == 2:
        ncols = 3   # (two breaks in one unit need three columns: the case runs there under both ids)
    S.check_select_breaks(ctx, name, case, ncols)


@pytest.mark.parametrize("curve", sorted(S.CURVES))
def test_bits_feed_a_selection_feed_an_addition_feed_a_selection(ctx, curve):
    S.check_chained(ctx, curve)


def test_four_limbs_chained(ctx):
    S.check_chained(ctx, "secp256k1_p", 64, 4, 8, count=2)


def test_rejections(ctx):
    S.check_rejections(ctx)


def test_window_step_inside_a_proof(ctx):
    S.check_proof(ctx, 11, seed=101, nl=2)


def test_a_scalar_that_does_not_fit_is_caught_by_the_copy_of_the_sum(ctx):
    S.check_proof(ctx, 11, seed=101, nl=2, s=5)
