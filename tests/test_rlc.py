"""RLC circuits on the CPU-emulated build: the device fill and the quotient kernel against their definitions, proof bytes against the test-side
prover (tests/shape_oracle.py), soundness, the refusals, and multi-phase keys before and after.  The checks live in tests/rlc_checks.py and run
on the GPU from tests/test_rlc_gpu.py."""
import pytest

from tests import rlc_checks as RC
from tests.util import R


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
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
def test_proof_bytes(ctx, shape):
    params, inst = (RC.shape_a if shape == "a" else RC.shape_b)(10, 8)   # (k = 10 takes the emulated build and the test prover 2 - 3 s together)
    RC.check_proof_bytes(ctx, params, inst, seed=50 + ord(shape), threads=8)


def test_soundness(ctx):
    RC.check_soundness(ctx, RC.EMU_K, 4, seed=7)


def test_limits(ctx):
    RC.check_limits(ctx, RC.EMU_K, 4, seed=11)


def test_phased_keys_unmoved(ctx):
    RC.check_phased_keys_unmoved(ctx, RC.EMU_K, 4)


def test_rlc_structs_agree_across_header_rust_and_ctypes():
    RC.check_struct_layouts()
