"""EccChip's ec_add_unequal and ec_double filled on the device (h2hip_ec_fill_dev), on the CPU-emulated build: the definition's own checks,
the fill against it for every parameter set, modulus and operation, the layout and the range tables, chained calls, column breaks as
assign_witnesses makes them, the refusals, the structs in every layer and a proof whose curve operations three fill calls write.  The checks
live in tests/ec_fill_checks.py and run on the GPU from tests/test_ec_fill_gpu.py."""
import pytest

from tests import ec_fill_checks as K


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def test_the_definition_holds_its_own_checks():
    K.check_definition()


def test_the_pools_hold_every_sign_of_quotient():
    K.check_pool_signs()


def test_layout_and_range_tables_equal_the_definition():
    K.check_layout_and_ranges()


@pytest.mark.parametrize("op", sorted(K.OPS))
@pytest.mark.parametrize("modulus", sorted(K.MODULI))
@pytest.mark.parametrize("n,k,lb", K.PARAMS, ids=["%d_%d_%d" % p for p in K.PARAMS])
def test_fill_against_its_definition(ctx, n, k, lb, modulus, op):
    K.check_op_fill(ctx, n, k, lb, modulus, K.OPS[op], 5)


@pytest.mark.parametrize("op", sorted(K.OPS))
@pytest.mark.parametrize("n,k,lb", K.PARAMS, ids=["%d_%d_%d" % p for p in K.PARAMS])
def test_one_unit_per_call(ctx, n, k, lb, op):
    sp = K.Spec(n, k, lb, K.SECP_P)
    pool = K.operand_pool(sp, "secp256k1_p")
    K.check_op_fill(ctx, n, k, lb, "secp256k1_p", K.OPS[op], 1, pool=pool[:2] + pool[6:10] + pool[-3:])


@pytest.mark.parametrize("op", sorted(K.OPS))
@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_lookup_cells_over_two_columns(ctx, n, k, lb, op):
    K.check_op_fill(ctx, n, k, lb, "secp256k1_n", K.OPS[op], 5, nl=2)


def test_reductions_with_different_carry_widths(ctx):
    K.check_three_carry_widths(ctx)


@pytest.mark.parametrize("n,k,lb", [(88, 3, 8), (64, 4, 8)])
def test_points_read_from_a_previous_calls_results(ctx, n, k, lb):
    K.check_chained(ctx, n, k, lb)


@pytest.mark.parametrize("ncols", [2, 3])
@pytest.mark.parametrize("case", K.BREAK_CASES)
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case, ncols):
    K.check_op_breaks(ctx, case, ncols)


def test_rejections(ctx):
    K.check_rejections(ctx)


def test_ec_structs_agree_across_header_rust_and_ctypes():
    K.check_struct_layout()


def test_curve_operations_inside_a_proof(ctx):
    K.check_proof(ctx, 10, seed=93, nl=2)


def test_equal_x_with_different_y_inside_a_circuit(ctx):
    K.check_proof(ctx, 10, seed=93, nl=2, mode="equal_x")
