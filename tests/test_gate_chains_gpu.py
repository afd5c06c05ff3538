"""Flex-gate chains filled on the GPU (h2hip_gate_fill_chains_dev): the checks of tests/gate_chain_checks.py, and the tile-totals level of
the scan at P - 1, P and P + 1 tiles."""
import pytest

from tests import gate_chain_checks as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import halo2_lib_amd as H

    c = H.Context()
    yield c
    c.close()


def test_fill_against_its_definition(ctx):
    GC.check_fill(ctx)


@pytest.mark.parametrize("pairs", [(GC.P - 1) * GC.T, GC.P * GC.T, (GC.P + 1) * GC.T + 3], ids=["P_minus_1_tiles", "P_tiles", "P_plus_1_tiles"])
def test_fill_across_the_tile_totals_pass(ctx, pairs):
    GC.check_fill_large(ctx, pairs)


def test_rejections(ctx):
    GC.check_rejections(ctx)


def test_reference_inner_products(ctx):
    GC.check_reference_kats(ctx)


@pytest.mark.parametrize("start_a", [False, True], ids=["from_zero", "start_a"])
def test_column_break_as_assign_witnesses_makes_it(ctx, start_a):
    GC.check_column_break(ctx, start_a)


def test_select_chains_inside_a_proof(ctx):
    GC.check_select_proof(ctx, 11, 8, seed=61)
