"""Proving and verifying over a caller-supplied transcript on the GPU: the checks of tests/transcript_checks.py at k = 10, and the schedule
switches (round-1 overlap, permutation inside the commitment batch, lazy upload, device RNG, device advice) at k = 12."""
import pytest

from tests import transcript_checks as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    import halo2_lib_amd as H

    ctx = H.Context()
    c = TC.Cases(ctx, lambda name: 10)
    yield c
    c.free()
    ctx.close()


@pytest.mark.parametrize("shape", TC.SHAPES)
def test_t1_through_the_callbacks_equals_the_builtin_entry(cases, shape):
    TC.check_t1_equals_builtin(cases(shape))


@pytest.mark.parametrize("shape", TC.SHAPES)
def test_t2_equals_the_python_prover(cases, shape, monkeypatch):
    TC.check_t2_equals_python_prover(cases(shape), monkeypatch)


@pytest.mark.parametrize("shape", TC.SHAPES)
def test_accumulator(cases, shape):
    TC.check_accumulator(cases(shape))


@pytest.mark.parametrize("shape", ["base2", "rlc"])
def test_rejections(cases, shape):
    TC.check_rejections(cases(shape))


@pytest.mark.parametrize("shape", TC.SHAPES)
def test_aborts(cases, shape):
    TC.check_aborts(cases(shape))


@pytest.mark.parametrize("shape", ["base1", "phased"])
def test_refusals(cases, shape):
    TC.check_refusals(cases(shape))


def test_schedule_switches(cases):
    TC.check_schedule_switches(cases.ctx)
