"""Range checks filled on the device (h2hip_range_fill_checks_dev), on the CPU-emulated build: the fill against the RangeChip mirror, the
layout function, both LESS_THAN forms, column breaks as assign_witnesses makes them, the refusals, the struct in every layer and a proof whose
range-check cells and lookup column the fill writes.  The checks live in tests/range_fill_checks.py and run on the GPU from
tests/test_range_fill_gpu.py."""
import pytest

from tests import range_fill_checks as K


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def test_layout_equals_the_mirrors_counts():
    K.check_layout()


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


@pytest.mark.parametrize("case", sorted(K.BREAK_CASES))
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case):
    K.check_breaks(ctx, case)


def test_rejections(ctx):
    K.check_rejections(ctx)


def test_range_check_struct_agrees_across_header_rust_and_ctypes():
    K.check_struct_layout()


def test_range_checks_inside_a_proof(ctx):
    K.check_proof(ctx, 10, seed=91)
