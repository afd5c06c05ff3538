"""FpChip::mul filled on the device (h2hip_fp_mul_fill_dev), on the CPU-emulated build: the definition's own checks, the fill against it for
every parameter set and modulus, the layout function and trace_seek, column breaks as assign_witnesses makes them, the refusals, the structs
in every layer and a proof whose field multiplications two fill calls write.  The checks live in tests/fp_mul_checks.py and run on the GPU
from tests/test_fp_mul_gpu.py."""
import pytest

from tests import fp_mul_checks as K


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def test_the_definition_holds_its_own_checks():
    K.check_definition()


def test_layout_and_trace_seek_equal_the_definition():
    K.check_layout_and_seek()


def test_trace_seek_equals_assign_witnesses_placement_on_an_exhaustive_grid():
    K.check_seek_grid()


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


@pytest.mark.parametrize("ncols", [2, 3])
@pytest.mark.parametrize("case", K.BREAK_CASES)
def test_column_breaks_as_assign_witnesses_makes_them(ctx, case, ncols):
    K.check_mul_breaks(ctx, case, ncols)


def test_rejections(ctx):
    K.check_rejections(ctx)


def test_fp_structs_agree_across_header_rust_and_ctypes():
    K.check_struct_layout()


def test_field_multiplications_inside_a_proof(ctx):
    K.check_proof(ctx, 10, seed=93)


def test_truncated_quotient_inside_a_circuit(ctx):
    K.check_proof(ctx, 10, seed=93, truncated=True)


def test_truncated_quotient_fails_a_range_lookup(ctx):
    K.check_proof(ctx, 10, seed=93, truncated=True, xs=[(1 << 264) - 1, (3 << 254) + 12345, (1 << 264) - 1])


def test_improper_limb_inside_a_circuit(ctx):
    """a_1 = 2^n: the carries round toward zero"""
    sp = K.Spec(88, 3, K.PROOF_LB, K.SECP_P)
    a = sp.crt(K.SECP_N)
    a[1] = 1 << 88
    K.check_proof(ctx, 10, seed=93, truncated=True, xs=[a, K.SECP_P - 7, 12345])
