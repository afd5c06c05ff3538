"""In-circuit Poseidon traces filled on the device (h2hip_poseidon_fill_hashes_dev), on the CPU-emulated build: the Python restatement
against the textbook sponge and the golden KATs, the fill against the restatement, independent answers, the optimised spec, column breaks as
assign_witnesses makes them, the refusals, and a proof whose hash cells the fill writes.  The checks live in tests/poseidon_trace_checks.py
and run on the GPU from tests/test_poseidon_trace_gpu.py."""
import pytest

from tests import poseidon_trace_checks as K


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def test_restatement_equals_the_textbook_sponge_and_the_golden_kats():
    K.check_restatement()


@pytest.mark.parametrize("t", [3, 5])
@pytest.mark.parametrize("count", [1, 5])
def test_fill_against_its_definition(ctx, t, count):
    rate = t - 1
    K.check_fill(ctx, t, count, (0, 1, rate - 1, rate, rate + 1, 2 * rate) if count == 5 else (1, rate))


def test_independent_answers(ctx):
    K.check_independent(ctx)


def test_optimised_spec_equals_the_python_derivation(ctx):
    K.check_spec_optimize(ctx)


@pytest.mark.parametrize("case", ["first", "middle_last_behind"])
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case):
    K.check_breaks(ctx, case)


def test_rejections(ctx):
    from tests.emu_util import emu_context

    fresh = emu_context()
    try:
        K.check_rejections(ctx, fresh)
    finally:
        fresh.close()


def test_merkle_root_inside_a_proof(ctx):
    K.check_proof(ctx, 10, seed=73)


def test_poseidon_hash_struct_agrees_across_header_rust_and_ctypes():
    K.check_struct_layout()
