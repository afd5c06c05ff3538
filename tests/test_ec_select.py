"""Point selections and scalar bits of an MSM trace filled on the device (h2hip_ec_select_fill_dev, h2hip_num_to_bits_fill_dev), on the
CPU-emulated build: the definition's own checks, the fills against it for every parameter set, modulus and window, the layouts, column breaks
as assign_witnesses makes them, chained calls, the refusals, the names in every layer and a proof of one window step whose trace the device
calls write.  The checks live in tests/ec_select_checks.py and run on the GPU from tests/test_ec_select_gpu.py."""
import pytest

from tests import ec_select_checks as S

IDS = ["%d_%d_%d" % p for p in S.PARAMS]
WINDOWED = [(n, k, lb, w) for n, k, lb in S.PARAMS for w in S.WINDOWS[k]]


@pytest.fixture(scope="module")
def ctx():
    from tests.emu_util import emu_context

    c = emu_context()
    yield c
    c.close()


def test_the_definition_holds_its_own_checks():
    S.check_definition()


def test_layouts_equal_the_definition(ctx):
    S.check_layouts(ctx)


@pytest.mark.parametrize("modulus", sorted(S.MODULI))
@pytest.mark.parametrize("n,k,lb", S.PARAMS, ids=IDS)
def test_select_against_its_definition(ctx, n, k, lb, modulus):
    S.check_select_fill(ctx, n, k, lb, modulus)


@pytest.mark.parametrize("modulus", sorted(S.MODULI))
@pytest.mark.parametrize("n,k,lb,w", WINDOWED, ids=["%d_%d_%d_w%d" % p for p in WINDOWED])
def test_select_from_bits_against_its_definition(ctx, n, k, lb, w, modulus):
    S.check_from_bits_fill(ctx, n, k, lb, modulus, w)


@pytest.mark.parametrize("nb", S.NUM_BITS)
def test_num_to_bits_against_its_definition(ctx, nb):
    S.check_bits_fill(ctx, nb)


def test_one_unit_per_call_and_no_results(ctx):
    sp = S.Spec(88, 3, 8, S.SECP_P)
    S.check_select_fill(ctx, 88, 3, 8, "secp256k1_p", 1, pool=S.select_pool(sp, "secp256k1_p")[:3])
    S.check_from_bits_fill(ctx, 88, 3, 8, "secp256k1_p", 2, 1, pool=S.from_bits_pool(sp, 2, "secp256k1_p")[:3])
    S.check_bits_fill(ctx, 5, 1, pool=S.bits_pool(5)[2:5])
    S.check_no_results(ctx)


@pytest.mark.parametrize("ncols", [2, 3])
@pytest.mark.parametrize("name,case", S.BREAK_CASES, ids=["%s-%s" % c for c in S.BREAK_CASES])
def test_column_breaks_as_assign_witnesses_makes_them(ctx, name, case, ncols):
    if case == "two" and ncols == 2:
        ncols = 3   # (two breaks in one unit need three columns: the case runs there under both ids)
    S.check_select_breaks(ctx, name, case, ncols)


@pytest.mark.parametrize("curve", sorted(S.CURVES))
def test_bits_feed_a_selection_feed_an_addition_feed_a_selection(ctx, curve):
    S.check_chained(ctx, curve)


def test_four_limbs_chained(ctx):
    S.check_chained(ctx, "secp256k1_p", 64, 4, 8, count=2)


def test_rejections(ctx):
    S.check_rejections(ctx)


def test_names_agree_across_header_rust_and_ctypes():
    S.check_names_in_every_layer()


def test_window_step_inside_a_proof(ctx):
    S.check_proof(ctx, 10, seed=101, nl=2)


def test_a_scalar_that_does_not_fit_is_caught_by_the_copy_of_the_sum(ctx):
    S.check_proof(ctx, 10, seed=101, nl=2, s=5)
