"""Proving and verifying over a caller-supplied transcript on the CPU-emulated build: T1 (the oracle's Blake2b transcript) through the callbacks
against the built-in entries, T2 (a Poseidon sponge the library has never seen) against the Python provers, the accumulator, the rejections,
the aborts and the refusals.  The checks live in tests/transcript_checks.py and run on the GPU from tests/test_transcript_gpu.py."""
import pytest

from tests import rlc_checks as RC
from tests import transcript_checks as TC

K = {"base1": 5, "base2": 6, "dyn": 5, "phased": 5, "rlc": RC.EMU_K}


@pytest.fixture(scope="module")
def cases():
    from tests.emu_util import emu_context

    ctx = emu_context()
    c = TC.Cases(ctx, K.__getitem__)
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


@pytest.mark.parametrize("shape", ["base2", "dyn", "phased"])
def test_aborts(cases, shape):
    TC.check_aborts(cases(shape))


@pytest.mark.parametrize("shape", ["base1", "phased"])
def test_refusals(cases, shape):
    TC.check_refusals(cases(shape))


def test_transcript_struct_agrees_across_header_rust_and_ctypes():
    TC.check_struct_layout()
