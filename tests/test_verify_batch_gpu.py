"""The batch verifier and the checked decompressor on the GPU (tests/verify_batch_checks.py holds the checks; tests/test_verify_batch.py runs
them on the CPU-emulated build).  Every key and its proofs are made once per module."""
import os
import subprocess

import pytest

import halo2_lib_amd as H
from tests import verify_batch_checks as VB

pytestmark = pytest.mark.gpu

BUILDERS = {
    "base": lambda ctx: VB.base_case(ctx, (12, 2, 1, 1, 1, 11), 16),
    "wide": lambda ctx: VB.base_case(ctx, (13, 4, 2, 2, 2, 10), 5),
    "k9": lambda ctx: VB.base_case(ctx, (9, 1, 1, 1, 0, 8), 2),
    "no_table": lambda ctx: VB.base_case(ctx, (10, 1, 0, 1, 0, None), 2),
    "dyn": lambda ctx: VB.dyn_case(ctx, 9, 16, accesses=200, mem_len=64),
    "phased": lambda ctx: VB.phased_case(ctx, "e", 9, 16),
    "phased_three": lambda ctx: VB.phased_case(ctx, "c", 10, 2),
}
KINDS = ["base", "dyn", "phased"]


@pytest.fixture(scope="module")
def ctx():
    c = H.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = BUILDERS[name](ctx)
        return made[name]

    yield get
    for c in made.values():
        c.free()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_checked_decompressor_gpu(ctx, n):
    VB.check_decompressor(ctx, n)


@pytest.mark.parametrize("count", [1, 2, 5, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_accept_gpu(cases, kind, count):
    VB.check_accept(cases(kind), count)


@pytest.mark.parametrize("name,count", [("wide", 5), ("k9", 2), ("no_table", 2), ("phased_three", 2)])
def test_accept_other_shapes_gpu(cases, name, count):
    VB.check_accept(cases(name), count)


@pytest.mark.parametrize("kind", KINDS + ["wide"])
def test_accumulator_gpu(cases, kind):
    VB.check_accumulator(cases(kind))


@pytest.mark.parametrize("mutation", VB.MUTATIONS)
@pytest.mark.parametrize("kind", KINDS + ["wide"])
def test_reject_gpu(cases, kind, mutation):
    VB.check_reject(cases(kind), mutation)


@pytest.mark.parametrize("kind", KINDS + ["wide"])
def test_reject_two_bad_proofs_gpu(cases, kind):
    VB.check_reject_two(cases(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_protocol_gpu(cases, kind):
    VB.check_protocol(cases(kind))


@pytest.mark.parametrize("kind", KINDS + ["wide"])
def test_single_verifier_agrees_with_the_oracle_gpu(cases, kind):
    VB.check_single_against_oracle(cases(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_python_mirror_gpu(cases, kind):
    VB.check_python_mirror(cases(kind))


def test_cpp_mirror_gpu():
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "halo2-lib_amd", "host", "selftest")
    if not os.path.exists(exe):   # normally prebuilt by __graft_entry__.build()
        import __graft_entry__ as g

        g.build()
    out = subprocess.run([exe, "9", "--verify-batch"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "verify_batch selftest OK" in out.stdout, out.stdout + out.stderr
