"""GPU: the kernels of h(X)'s numerator at the extended-domain sizes at which a lane takes several points (tests/quotient_scale_checks.py):
2, 4 and 8 points per lane of the permutation kernels at 2^19, 2^20 and 2^21 points, two and four sweeps of the gate and lookup kernels, both
paths of divide_by_vanishing_poly, extended_to_coeff on full-degree data, and the whole chain on one device accumulator.  "Both forms" are
quotient_29 = 1 (unsaturated limbs, the default) and 0 (the saturated kernels)."""
import pytest

import halo2_lib_amd as H
from tests import quotient_scale_checks as K

pytestmark = pytest.mark.gpu
BOTH, DEFAULT = (1, 0), (1,)


@pytest.fixture(scope="module")
def ctx():
    c = H.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("k,ek,per_lane,forms", [(17, 19, 2, BOTH), (18, 20, 4, DEFAULT), (19, 21, 8, BOTH)])
def test_permutation_sets(ctx, k, ek, per_lane, forms):
    K.check_permutation_sets(ctx, k, ek, forms, expect_per_lane=per_lane)


def test_permutation_sets_sharded_form(ctx):
    """ext_k == k, a coset shift that is not ZETA, the generator of the 2^k domain: what the sharded prover's quotient_pass passes"""
    K.check_permutation_sets(ctx, 19, 19, BOTH, shift=K.sharded_shift(), expect_per_lane=2)


def test_permutation_sets_edge_patterns(ctx):
    K.check_permutation_sets(ctx, 17, 19, BOTH, edge=True, expect_per_lane=2)


@pytest.mark.parametrize("k,ek,per_lane", [(17, 19, 2), (19, 21, 8)])
def test_permutation_set_jobs(ctx, k, ek, per_lane):
    K.check_permutation_set_jobs(ctx, k, ek, BOTH, expect_per_lane=per_lane)


@pytest.mark.parametrize("k,ek", [(18, 20), (19, 21)])
def test_gate_batch(ctx, k, ek):
    K.check_gate_batch(ctx, k, ek, BOTH)


@pytest.mark.parametrize("k,ek", [(18, 20), (19, 21)])
def test_lookups(ctx, k, ek):
    K.check_lookups(ctx, k, ek, BOTH)


@pytest.mark.parametrize("k", [19, 18, 17, 5])
def test_divide_by_vanishing_poly(ctx, k):
    """2^(21 - k) = 4 (the prover's case), 8 (the last shape whose inverses travel as kernel arguments), 16 (the first table) and 2^16 (the largest)"""
    K.check_divide(ctx, k, 21)


def test_divide_by_vanishing_poly_sharded_form(ctx):
    K.check_divide(ctx, 21, 21, shift=K.sharded_shift())


def test_divide_by_vanishing_poly_refuses_long_tables(ctx):
    K.check_divide_refuses_long_tables(ctx)


@pytest.mark.parametrize("ek", [5, 11, 14, 19, 21])
def test_extended_to_coeff_full_degree(ctx, ek):
    K.check_extended_to_coeff_full_degree(ctx, ek)


@pytest.mark.parametrize("ek", [5, 14, 19])
def test_coeff_to_extended_in_place(ctx, ek):
    K.check_coeff_to_extended_in_place(ctx, ek)


def test_chain_on_one_accumulator(ctx):
    K.check_chain(ctx, 19, 21)
