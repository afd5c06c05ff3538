"""RLC circuits on the GPU: the checks of tests/rlc_checks.py at k = 10, and shape B at k = 14 with phase 1 filled on the device
(phase_witness_dev + rlc_fill_chains) against the same proof with host-computed columns."""
import pytest

from tests import rlc_checks as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import halo2_lib_amd as H

    c = H.Context()
    yield c
    c.close()


@pytest.mark.parametrize("gamma", RC.FILL_GAMMAS, ids=["zero", "one", "r_minus_1", "random"])
def test_fill_against_its_definition(ctx, gamma):
    RC.check_fill(ctx, gamma)


def test_fill_rejections(ctx):
    RC.check_fill_rejections(ctx)


@pytest.mark.parametrize("count", [1, 3, 65])
def test_quotient_rlc_gate_every_point(ctx, count):
    RC.check_quotient_rlc_gate(ctx, 12, 10, count)


def test_quotient_rlc_gate_several_points_per_lane(ctx):
    RC.check_quotient_rlc_gate(ctx, 20, 18, 2, sampled=4096)


@pytest.mark.parametrize("shape", ["a", "b"])
def test_proof_bytes_k10(ctx, shape):
    params, inst = (RC.shape_a if shape == "a" else RC.shape_b)(10, 8)
    RC.check_proof_bytes(ctx, params, inst, seed=50 + ord(shape), threads=8)


def test_shape_b_k14_filled_on_the_device(ctx):
    RC.check_device_fill_proof(ctx, 14, 8, seed=23)


def test_soundness(ctx):
    RC.check_soundness(ctx, 10, 8, seed=7)


def test_limits(ctx):
    RC.check_limits(ctx, 10, 8, seed=11)


def test_phased_keys_unmoved(ctx):
    RC.check_phased_keys_unmoved(ctx, 10, 8)
