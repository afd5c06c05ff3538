"""The curve arithmetic of a strict MSM trace filled on the device (ec_sub_unequal, FpChip's comparisons, and the two as a strict operation),
on the CPU-emulated build: the definition's own checks, the fill against it for every mask, parameter set and modulus, the layouts and the
range tables, chained calls, column breaks as assign_witnesses makes them, the refusals, the names in every layer and a proof of an MSM
fragment whose trace the device calls write.  The checks live in tests/ec_strict_checks.py and run on the GPU from tests/test_ec_strict_gpu.py."""
import pytest

from tests import ec_strict_checks as S

IDS = ["%d_%d_%d" % p for p in S.PARAMS]


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def test_the_definition_holds_its_own_checks():
    S.check_definition()


def test_the_pools_hold_every_sign_of_quotient_and_every_borrow():
    S.check_pool_signs()


def test_layouts_and_range_tables_equal_the_definition():
    S.check_layout_and_ranges()


@pytest.mark.parametrize("modulus", sorted(S.MODULI))
@pytest.mark.parametrize("n,k,lb", S.PARAMS, ids=IDS)
def test_sub_unequal_against_its_definition(ctx, n, k, lb, modulus):
    S.check_sub_fill(ctx, n, k, lb, modulus, 5)


@pytest.mark.parametrize("mask", S.MASKS)
@pytest.mark.parametrize("modulus", sorted(S.MODULI))
@pytest.mark.parametrize("n,k,lb", S.PARAMS, ids=IDS)
def test_comparison_against_its_definition(ctx, n, k, lb, modulus, mask):
    S.check_cmp_fill(ctx, n, k, lb, modulus, mask, 7)


@pytest.mark.parametrize("n,k,lb", S.PARAMS, ids=IDS)
def test_one_unit_per_call(ctx, n, k, lb):
    sp = S.Spec(n, k, lb, S.SECP_P)
    pool = S.sub_pool(sp, "secp256k1_p")
    S.check_sub_fill(ctx, n, k, lb, "secp256k1_p", 1, pool=pool[:2] + pool[6:10] + pool[-3:])
    pool = S.cmp_pool(sp)
    for mask in (3, 4, 7):
        S.check_cmp_fill(ctx, n, k, lb, "secp256k1_p", mask, 1, pool=pool[2:5] + pool[-4:])


@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_lookup_cells_over_two_columns(ctx, n, k, lb):
    S.check_sub_fill(ctx, n, k, lb, "secp256k1_n", 5, nl=2)
    for mask in (2, 7):
        S.check_cmp_fill(ctx, n, k, lb, "secp256k1_n", mask, 5, nl=2)


@pytest.mark.parametrize("mask", [4, 5, 6, 7])
@pytest.mark.parametrize("op", ["add_unequal", "sub_unequal"])
def test_strict_operation_in_two_fused_calls(ctx, op, mask):
    S.check_strict(ctx, 88, 3, 8, {"add_unequal": S.ADD, "sub_unequal": S.SUB}[op], mask)


def test_strict_operation_with_four_limbs(ctx):
    S.check_strict(ctx, 64, 4, 8, S.SUB, 7, count=3)


@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_strict_addition_reads_a_subtractions_results(ctx, n, k, lb):
    S.check_chained(ctx, n, k, lb)


@pytest.mark.parametrize("ncols", [2, 3])
@pytest.mark.parametrize("case", S.BREAK_CASES)
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case, ncols):
    S.check_strict_breaks(ctx, case, ncols)


def test_rejections(ctx):
    S.check_rejections(ctx)


def test_names_agree_across_header_rust_and_ctypes():
    S.check_names_in_every_layer()


def test_msm_fragment_inside_a_proof(ctx):
    S.check_proof(ctx, 10, seed=97, nl=2)


def test_equal_x_is_caught_by_the_pinned_equality_cell(ctx):
    S.check_proof(ctx, 10, seed=97, nl=2, mode="equal_x")
