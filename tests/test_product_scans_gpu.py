"""Prefix and grand products past 1024 scan tiles, zero factors on the positions the inversion and the scan treat specially, and the pointwise
kernels where every lane walks its grid-stride loop, on the GPU: the checks of tests/product_scan_checks.py, bit-exact against the serial C
oracle.  (The same checks run on the emulated kernels from tests/test_product_scans.py.)"""
import pytest

import halo2_lib_amd as H
from tests import product_scan_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = H.Context()
    yield c
    c.close()


# ---- A1: 1024 tiles (per = 1), 1025 tiles (per = 2, lane 512 takes one total), 2050 tiles (per = 3, lane 683 takes one total)
@pytest.mark.parametrize("length", K.LONG_LENGTHS)
def test_prefix_product_around_and_beyond_1024_tiles(ctx, length):
    K.check_prefix_product(ctx, length)


@pytest.mark.parametrize("n", K.LONG_LENGTHS)
def test_grand_product_around_and_beyond_1024_tiles(ctx, n):
    K.check_grand_product(ctx, n)


def test_telescoping_grand_product_over_2050_tiles(ctx):
    K.check_telescoping(ctx, K.LONG_LENGTHS[-1])


# ---- A2 / A3
def test_three_chained_sets_at_k_20(ctx):
    K.check_grand_products(ctx, 3, (1 << 20) - 6, True)


def test_two_unchained_segments_of_1025_tiles(ctx):
    K.check_grand_products(ctx, 2, K.TILE * 1024, False)


# ---- A4
@pytest.mark.parametrize("length", K.SHORT_LENGTHS)
def test_prefix_product_short_edges(ctx, length):
    K.check_prefix_product(ctx, length)


@pytest.mark.parametrize("chained", [False, True], ids=["unchained", "chained"])
@pytest.mark.parametrize("seg_len", [5, 2049])
@pytest.mark.parametrize("segments", [33, 65])
def test_grand_products_across_scatter_groups(ctx, segments, seg_len, chained):
    K.check_grand_products(ctx, segments, seg_len, chained)


def test_empty_segments(ctx):
    K.check_empty_segments(ctx)


def test_65536_segments_are_refused(ctx):
    K.check_too_many_segments(ctx)


# ---- B
def test_zero_denominators_where_a_lanes_run_starts_and_ends(ctx):
    K.check_zero_denominators(ctx)


@pytest.mark.parametrize("at", [K.TILE * 1024 - 1, K.TILE * 1024], ids=["last_of_tile_1023", "first_of_tile_1024"])
def test_zero_numerator_in_the_last_of_1025_tiles(ctx, at):
    K.check_zero_numerator_long(ctx, K.TILE * 1024 + 1, at)


@pytest.mark.parametrize("at_scan", [8 * K.TILE - 1, 8 * K.TILE], ids=["last_of_tile_7", "first_of_tile_8"])
def test_zero_numerator_in_the_last_chained_set(ctx, at_scan):
    K.check_zero_numerator_chained(ctx, at_scan)


@pytest.mark.parametrize("n,run", K.RUN_LENGTHS, ids=["run%d" % r for _, r in K.RUN_LENGTHS])
def test_in_place_inversion_at_the_automatic_run_lengths(ctx, n, run):
    K.check_invert_in_place(ctx, n, run)


# ---- C: n = 2^20 + 259
def test_binops_two_sweeps_and_a_bit(ctx):
    K.check_binops(ctx)


def test_scaled_sums_two_sweeps_and_a_bit(ctx):
    K.check_scaled_sums(ctx)


@pytest.mark.parametrize("count", [16, 5])
def test_linear_combination_two_sweeps_and_a_bit(ctx, count):
    K.check_linear_combination(ctx, count)


def test_lookup_product_terms_two_sweeps_and_a_bit(ctx):
    K.check_lookup_terms(ctx)


def test_assigned_resolve_two_sweeps_and_a_bit(ctx):
    K.check_assigned_resolve(ctx)
