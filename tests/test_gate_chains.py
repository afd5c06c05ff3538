"""Flex-gate chains filled on the device (h2hip_gate_fill_chains_dev), on the CPU-emulated build: the fill against its definition, the
refusals, the reference's inner-product answers, column breaks as the layout engine makes them, and a proof whose phase-1 gate columns are
select_by_indicator chains written by the fill.  The checks live in tests/gate_chain_checks.py and run on the GPU from
tests/test_gate_chains_gpu.py."""
import pytest

from tests import gate_chain_checks as GC


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def test_fill_against_its_definition(ctx):
    GC.check_fill(ctx)


def test_rejections(ctx):
    GC.check_rejections(ctx)


def test_reference_inner_products(ctx):
    GC.check_reference_kats(ctx)


@pytest.mark.parametrize("start_a", [False, True], ids=["from_zero", "start_a"])
def test_column_break_as_assign_witnesses_makes_it(ctx, start_a):
    GC.check_column_break(ctx, start_a)


def test_select_chains_inside_a_proof(ctx):
    GC.check_select_proof(ctx, 10, 8, seed=61)


def test_gate_chain_struct_agrees_across_header_rust_and_ctypes():
    GC.check_struct_layout()
