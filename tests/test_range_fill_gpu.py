"""Range checks filled on the GPU (h2hip_range_fill_checks_dev): the checks of tests/range_fill_checks.py, and lane counts around the
kernel's workgroup size (one lane per (unit, slot), BLOCK lanes per workgroup, one row of workgroups)."""
import pytest

import halo2_lib_amd as H
from tests import range_fill_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = H.Context()
    yield c
    c.close()


@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("lb,rb", K.PAIRS, ids=["%d_%d" % p for p in K.PAIRS])
def test_fill_against_its_definition(ctx, lb, rb, count):
    K.check_fill(ctx, lb, rb, count)


@pytest.mark.parametrize("nl", [2, 3])
@pytest.mark.parametrize("lb,rb", [(8, 8), (8, 5), (13, 88)])
def test_lookup_cells_over_several_columns(ctx, lb, rb, nl):
    K.check_fill(ctx, lb, rb, 5, nl=nl)


@pytest.mark.parametrize("count", [1, 5])
def test_check_less_than(ctx, count):
    K.check_fill(ctx, 10, 64, count, nl=2, less_than=True)


def test_is_less_than_prefix_and_its_last_limb(ctx):
    K.check_is_less_than_prefix(ctx)


@pytest.mark.parametrize("count", [36, 37, 1000], ids=["252_lanes", "259_lanes", "7000_lanes"])
def test_units_straddle_workgroups(ctx, count):
    """(12, 84): S = 7 slots per unit does not divide the workgroup's 256 lanes"""
    assert K.slots(12, 84) == 7 and count * 7 in (K.BLOCK - 4, K.BLOCK + 3, 7000)
    K.check_fill(ctx, 12, 84, count, nl=2)


@pytest.mark.parametrize("count", [32, 33], ids=["one_full_workgroup", "one_lane_more"])
def test_fill_around_the_workgroup_size(ctx, count):
    """(13, 88): S = 8, so 32 units fill one workgroup exactly"""
    assert K.slots(13, 88) * 32 == K.BLOCK
    K.check_fill(ctx, 13, 88, count)


@pytest.mark.parametrize("case", sorted(K.BREAK_CASES))
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case):
    K.check_breaks(ctx, case)


def test_rejections(ctx):
    K.check_rejections(ctx)


def test_range_checks_inside_a_proof(ctx):
    K.check_proof(ctx, 11, seed=91, nl=2)
