"""Every NTT pass plan and first-pass branch on the GPU: the checks of tests/ntt_plan_checks.py, bit-exact against the C oracle.  (The same checks
run on the emulated kernels from tests/test_ntt_plans.py, up to 2^17; that the case lists reach the branches they are named for is asserted there,
for both lists, without a kernel.)"""
import pytest

import halo2_lib_amd as H
from tests import ntt_plan_checks as K

pytestmark = pytest.mark.gpu

NT = 16   # oracle threads


@pytest.fixture(scope="module")
def ctx():
    c = H.Context()
    yield c
    c.close()


@pytest.mark.parametrize("log_n", K.TRANSFORMS_GPU)
def test_forward_transform(ctx, log_n):
    K.check_forward(ctx, log_n, NT)


@pytest.mark.parametrize("log_n", K.TRANSFORMS_GPU)
def test_inverse_transform_with_the_fused_divisor(ctx, log_n):
    K.check_inverse(ctx, log_n, NT)


@pytest.mark.parametrize("k,ek", K.EXTENSIONS_GPU)
def test_coset_extension_and_back(ctx, k, ek):
    K.check_extension(ctx, k, ek, NT)


def test_batched_extension_of_33_columns(ctx):
    K.check_extension_batch(ctx, NT)


def test_batched_inverse_of_33_columns(ctx):
    K.check_ifft_batch(ctx, NT)


@pytest.mark.parametrize("case", K.KNOB_PLANS_GPU, ids=K.knob_id)
def test_knob_plans(ctx, case):
    K.check_knob_plan(ctx, case, NT)
