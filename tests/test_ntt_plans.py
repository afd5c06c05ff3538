"""Every NTT pass plan and first-pass branch on the CPU-emulated build: the checks of tests/ntt_plan_checks.py, bit-exact against the C oracle.
The emulator compiles the same kernels and the same driver, so the plans are the ones the GPU runs; what it cannot falsify is an ordering across a
barrier (lanes are fibres), which is why the same cases run on the GPU from tests/test_ntt_plans_gpu.py.  The emulated lists stop at 2^17: the 2^19
and 2^22 extensions, the transforms from 2^18 on and the 2^22 knob plans are GPU-only (see the checks module)."""
import pytest

from tests import ntt_plan_checks as K

NT = 4   # oracle threads


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def test_the_cases_reach_the_branches_they_are_named_for():
    K.check_cases_reach_their_branches()


@pytest.mark.parametrize("log_n", K.TRANSFORMS_EMU)
def test_forward_transform(ctx, log_n):
    K.check_forward(ctx, log_n, NT)


@pytest.mark.parametrize("log_n", K.TRANSFORMS_EMU)
def test_inverse_transform_with_the_fused_divisor(ctx, log_n):
    K.check_inverse(ctx, log_n, NT)


@pytest.mark.parametrize("k,ek", K.EXTENSIONS_EMU)
def test_coset_extension_and_back(ctx, k, ek):
    K.check_extension(ctx, k, ek, NT)


def test_batched_extension_of_33_columns(ctx):
    K.check_extension_batch(ctx, NT)


def test_batched_inverse_of_33_columns(ctx):
    K.check_ifft_batch(ctx, NT)


@pytest.mark.parametrize("case", K.KNOB_PLANS_EMU, ids=K.knob_id)
def test_knob_plans(ctx, case):
    K.check_knob_plan(ctx, case, NT)
