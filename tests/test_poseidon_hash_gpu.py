"""GPU: PoseidonHasher batches and Merkle trees on the device, the checks of tests/poseidon_hash_checks.py at the sizes at which the tree
changes kernels (one lane per node above 2^14 (t = 3) / 2^15 (t = 5) nodes per level, one lane group per node up to there, one launch for the
top): a tree of 2^16 leaves has levels up to 2^15 nodes, one of 2^17 leaves the first level past the t = 5 switch-over."""
import os
import subprocess

import pytest

import halo2_lib_amd as H
from tests import poseidon_hash_checks as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = H.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("t,length,n", K.FIX_CASES)
def test_fixed_length(ctx, t, length, n):
    K.check_fixed_length(ctx, t, length, n)


@pytest.mark.parametrize("t", [3, 5])
def test_variable_length(ctx, t):
    K.check_variable_length(ctx, t)


def test_misuse(ctx):
    fresh = H.Context(device=0)
    try:
        K.check_misuse(ctx, fresh)
    finally:
        fresh.close()


@pytest.mark.parametrize("t,log_leaves", K.TREE_ORACLE_CASES)
def test_tree_against_oracle(ctx, t, log_leaves):
    K.check_tree_against_oracle(ctx, t, log_leaves)


@pytest.mark.parametrize("log_leaves", list(range(15)) + [16, 17])
@pytest.mark.parametrize("t", [3, 5])
def test_tree_levels_across_the_switch_overs(ctx, t, log_leaves):
    K.check_tree_levels(ctx, t, log_leaves)


@pytest.mark.parametrize("t", [3, 5])
def test_permute_batch_unchanged(ctx, t):
    K.check_permute_unchanged(ctx, t)


def test_python_mirror(ctx):
    K.check_mirror(ctx)


def test_cpp_mirror():
    exe = os.path.join(ROOT, "halo2-lib_amd", "host", "selftest")
    if not os.path.exists(exe):   # normally prebuilt by the package's build
        import __graft_entry__ as g

        g.build()
    out = subprocess.run([exe, "7", "--poseidon"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "poseidon selftest OK" in out.stdout, out.stdout + out.stderr
