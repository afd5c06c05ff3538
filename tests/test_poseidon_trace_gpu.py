"""In-circuit Poseidon traces filled on the GPU (h2hip_poseidon_fill_hashes_dev): the checks of tests/poseidon_trace_checks.py, and unit
counts around the kernel's workgroup size (one lane per unit, BLOCK lanes per workgroup, one row of workgroups)."""
import pytest

import halo2_lib_amd as H
from tests import poseidon_trace_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = H.Context()
    yield c
    c.close()


@pytest.mark.parametrize("t", [3, 5])
@pytest.mark.parametrize("count", [1, 5])
def test_fill_against_its_definition(ctx, t, count):
    rate = t - 1
    K.check_fill(ctx, t, count, (0, 1, rate - 1, rate, rate + 1, 2 * rate) if count == 5 else (1, rate))


@pytest.mark.parametrize("count", [K.BLOCK - 1, K.BLOCK, K.BLOCK + 1], ids=["B_minus_1", "B", "B_plus_1"])
def test_fill_around_the_workgroup_size(ctx, count):
    K.check_fill(ctx, 3, count, (1,), with_states=(True,))


def test_independent_answers(ctx):
    K.check_independent(ctx)


def test_optimised_spec_equals_the_python_derivation(ctx):
    K.check_spec_optimize(ctx)


@pytest.mark.parametrize("case", ["first", "middle_last_behind"])
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case):
    K.check_breaks(ctx, case)


def test_rejections(ctx):
    fresh = H.Context()
    try:
        K.check_rejections(ctx, fresh)
    finally:
        fresh.close()


def test_merkle_root_inside_a_proof(ctx):
    K.check_proof(ctx, 11, seed=73)
