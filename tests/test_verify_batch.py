"""The batch verifier and the checked decompressor on the CPU-emulated build (tests/verify_batch_checks.py holds the checks; the GPU runs
them in tests/test_verify_batch_gpu.py).  The emulated kernels are slow, so every key and its proofs are made once per module."""
import pytest

import tests.emu_util  # noqa: F401  (puts tests/emu on the path)

from tests import verify_batch_checks as VB

BASE_SHAPES = {"two_columns": (6, 2, 2, 2, 1, 3), "wide": (5, 6, 4, 1, 1, 3), "no_table": (6, 1, 0, 1, 0, None), "k7": (7, 2, 1, 1, 1, 5),
               "q_lookup": (6, 1, 1, 1, 0, 4)}
BUILDERS = {
    "base": lambda ctx: VB.base_case(ctx, BASE_SHAPES["two_columns"], 16),
    "wide": lambda ctx: VB.base_case(ctx, BASE_SHAPES["wide"], 5),
    "no_table": lambda ctx: VB.base_case(ctx, BASE_SHAPES["no_table"], 2),
    "k7": lambda ctx: VB.base_case(ctx, BASE_SHAPES["k7"], 2),
    "q_lookup": lambda ctx: VB.base_case(ctx, BASE_SHAPES["q_lookup"], 2),
    "dyn": lambda ctx: VB.dyn_case(ctx, 5, 16),
    "phased": lambda ctx: VB.phased_case(ctx, "e", 5, 16),
    "phased_three": lambda ctx: VB.phased_case(ctx, "c", 5, 2),
}
KINDS = ["base", "dyn", "phased"]


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
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
def test_checked_decompressor_emulated(ctx, n):
    VB.check_decompressor(ctx, n)


@pytest.mark.parametrize("count", [1, 2, 5, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_accept_emulated(cases, kind, count):
    VB.check_accept(cases(kind), count)


@pytest.mark.parametrize("name,count", [("wide", 5), ("no_table", 2), ("k7", 2), ("q_lookup", 2), ("phased_three", 2)])
def test_accept_other_shapes_emulated(cases, name, count):
    VB.check_accept(cases(name), count)


@pytest.mark.parametrize("kind", KINDS + ["wide"])
def test_accumulator_emulated(cases, kind):
    VB.check_accumulator(cases(kind))


@pytest.mark.parametrize("mutation", VB.MUTATIONS)
@pytest.mark.parametrize("kind", KINDS + ["wide"])
def test_reject_emulated(cases, kind, mutation):
    VB.check_reject(cases(kind), mutation)


@pytest.mark.parametrize("kind", KINDS + ["wide"])
def test_reject_two_bad_proofs_emulated(cases, kind):
    VB.check_reject_two(cases(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_protocol_emulated(cases, kind):
    VB.check_protocol(cases(kind))


@pytest.mark.parametrize("kind", KINDS + ["wide"])
def test_single_verifier_agrees_with_the_oracle_emulated(cases, kind):
    VB.check_single_against_oracle(cases(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_python_mirror_emulated(cases, kind):
    VB.check_python_mirror(cases(kind))


def test_cpp_mirror_over_emulated_kernels(tmp_path):
    """plonk::verify_proofs of halo2-lib_amd/host/halo2_proofs.hpp compiles and decides a small batch (selftest.cpp --verify-batch)"""
    import os
    import subprocess

    import build_emu   # tests/emu, on the path through tests.emu_util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = build_emu.build()
    exe = str(tmp_path / "selftest_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(root, "halo2-lib_amd", "host", "selftest.cpp"), "-L" + os.path.dirname(lib),
                           "-lh2hip_emu", "-Wl,-rpath," + os.path.dirname(lib), "-lpthread"])
    out = subprocess.run([exe, "6", "--verify-batch"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "verify_batch selftest OK" in out.stdout, out.stdout + out.stderr
