"""FpChip::mul filled on the GPU (h2hip_fp_mul_fill_dev): the checks of tests/fp_mul_checks.py, and unit counts around the workgroup sizes
of both kernels (one lane per unit, SOLVE_BLOCK lanes per workgroup; one lane per (unit, slot), PLACE_BLOCK lanes per workgroup)."""
import pytest

import halo2_lib_amd as H
from tests import fp_mul_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = H.Context()
    yield c
    c.close()


@pytest.mark.parametrize("modulus", sorted(K.MODULI))
@pytest.mark.parametrize("n,k,lb", K.PARAMS, ids=["%d_%d_%d" % p for p in K.PARAMS])
def test_fill_against_its_definition(ctx, n, k, lb, modulus):
    K.check_mul_fill(ctx, n, k, lb, modulus, 5)


@pytest.mark.parametrize("n,k,lb", K.PARAMS, ids=["%d_%d_%d" % p for p in K.PARAMS])
def test_one_unit_per_call(ctx, n, k, lb):
    sp = K.Spec(n, k, lb, K.SECP_P)
    K.check_mul_fill(ctx, n, k, lb, "secp256k1_p", 1, pairs=K.operand_pairs(sp, 0xF9)[14:22] + K.operand_pairs(sp, 0xF9)[-2:])


@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_lookup_cells_over_two_columns(ctx, n, k, lb):
    K.check_mul_fill(ctx, n, k, lb, "secp256k1_n", 5, nl=2)


@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_operands_read_from_a_previous_calls_results(ctx, n, k, lb):
    K.check_chained(ctx, n, k, lb, "secp256k1_p")


def test_results_may_be_null(ctx):
    K.check_results_null(ctx)


@pytest.mark.parametrize("count", [K.SOLVE_BLOCK - 1, K.SOLVE_BLOCK, K.SOLVE_BLOCK + 1], ids=["one_before", "on_the_edge", "one_past"])
def test_units_around_the_solving_workgroup(ctx, count):
    K.check_mul_fill(ctx, 88, 3, 18, "secp256k1_p", count)


@pytest.mark.parametrize("count", [17, 18, 239, 255, 256, 257], ids=["255_lanes", "270_lanes", "3585_lanes", "3825_lanes", "3840_lanes", "3855_lanes"])
def test_units_around_the_placing_workgroup(ctx, count):
    """(88, 3): 15 slots per unit.  17 units end one lane before the first edge (255 lanes), 256 units exactly on the fifteenth (3,840),
    239 units one lane past the fourteenth (3,585 = 14 * 256 + 1); 18, 255 and 257 units end further from an edge"""
    assert K.slots(3) == 15 and 17 * 15 == K.PLACE_BLOCK - 1 and 256 * 15 % K.PLACE_BLOCK == 0 and 239 * 15 % K.PLACE_BLOCK == 1
    K.check_mul_fill(ctx, 88, 3, 8, "secp256k1_p", count)


@pytest.mark.parametrize("ncols", [2, 3])
@pytest.mark.parametrize("case", K.BREAK_CASES)
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case, ncols):
    K.check_mul_breaks(ctx, case, ncols)


def test_rejections(ctx):
    K.check_rejections(ctx)


def test_field_multiplications_inside_a_proof(ctx):
    K.check_proof(ctx, 11, seed=93, nl=2)


def test_truncated_quotient_inside_a_circuit(ctx):
    K.check_proof(ctx, 11, seed=93, nl=2, truncated=True)


def test_truncated_quotient_fails_a_range_lookup(ctx):
    K.check_proof(ctx, 11, seed=93, nl=2, truncated=True, xs=[(1 << 264) - 1, (3 << 254) + 12345, (1 << 264) - 1])


def test_improper_limb_inside_a_circuit(ctx):
    """a_1 = 2^n: the carries round toward zero"""
    sp = K.Spec(88, 3, K.PROOF_LB, K.SECP_P)
    a = sp.crt(K.SECP_N)
    a[1] = 1 << 88
    K.check_proof(ctx, 11, seed=93, nl=2, truncated=True, xs=[a, K.SECP_P - 7, 12345])
