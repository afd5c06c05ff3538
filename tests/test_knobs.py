"""CPU-only: the tuning knobs' legal domains and their inheritance (H2_KNOB_TABLE in halo2-lib_amd/csrc/internal.h, h2hip_set_param).
Values are set and read back on an emulated context of this module's own; no kernel runs with a value outside a domain.  The differential
checks of what the knobs select are tests/knob_checks.py (test_emu_kernels.py / test_gpu_parity.py)."""
import os
import re

import pytest

import halo2_lib_amd as H
from tests.emu_util import emu_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIT = ([0, 1], [-1, 2, 3, 1 << 30])
# name -> (values that must be accepted: every boundary and the values just inside it, values that must be refused: just outside,
# negative, non-powers of two where a power of two is required)
DOMAINS = {
    "msm_window_bits": ([0, 4, 5, 15, 16], [-1, 1, 2, 3, 17, 32]),
    "msm_chunk": ([0, 2, 3, 4095, 4096], [-1, 1, 4097]),
    "msm_chunk_lone": ([-1, 0, 1, 2, 4095, 4096], [-2, 4097, -(1 << 31)]),
    "msm_seg": ([1, 2, 4, 512, 1024], [-4, 0, 3, 6, 1000, 2048]),
    "msm_quad_tails": BIT,
    "msm_quad_seg_max": ([0, 1, 32768, (1 << 31) - 1], [-1, -(1 << 31)]),
    "msm_sort_threads": ([256, 512, 1024], [-256, 0, 255, 257, 768, 2048]),
    "msm_sort_groups": ([0, 1, 2, 1023, 1024], [-1, 1025]),
    "msm_hist_split": ([0, 1, 2, 4, 8, 16, 32, 64], [-1, -2, 3, 5, 6, 7, 48, 63, 65, 128]),
    "msm_hist_packed": BIT,
    "msm_scatter_split": ([0, 1, 2, 32, 64], [-1, -2, 3, 6, 63, 65, 128]),
    "msm_scatter_full_lds": BIT,
    "msm_table_split": BIT,
    "msm_lanes": ([0, 1, 3, 4], [-1, 5]),
    "msm_stagger_sorts": ([-1, 0, 1], [-2, 2]),
    "msm_fuse_cols": ([0, 1, 31, 32], [-1, 33]),
    "msm_defer_reduce": BIT,
    "clean_on_lane": BIT,
    "ntt_tile_bits": ([4, 5, 9, 10], [-1, 0, 3, 11]),
    "ntt_min_col_bits": ([0, 1, 4, 5], [-1, 6]),
    "ntt_full_table": BIT,
    "ntt_tile_kernel": BIT,
    "ntt_debug_skip": ([0, 1, 2], [-1, 3]),
    "quotient_29": BIT,
    "kate_29": BIT,
    "kate_coeffs_per_lane": ([0, 1, 2, 4, 8], [-1, 3, 5, 6, 7, 9, 16]),
    "fr_invert_run": ([0, 1, 2, 1023, 1024], [-1, 1025]),
    "lookup_big_tile_bits": ([12, 13, 27, 28], [-1, 11, 29]),
    "host_poll": BIT,
    "plonk_warm_keygen": BIT,
    "plonk_tail_overlap": BIT,
    "plonk_side_on_lanes": BIT,
    "plonk_permute_in_commit": BIT,
    "plonk_merge_products": BIT,
    "plonk_shard_side": ([0, 1, 2], [-1, 3]),
    "plonk_route_rows": BIT,
    "plonk_lazy_upload": BIT,
    "plonk_early_intt": BIT,
    "plonk_gate_before_join": BIT,
}
# domains that are whole ranges between their boundaries (the others are the listed values)
RANGES = {"msm_window_bits", "msm_chunk", "msm_chunk_lone", "msm_quad_seg_max", "msm_sort_groups", "msm_lanes", "msm_fuse_cols", "ntt_tile_bits",
          "ntt_min_col_bits", "fr_invert_run", "lookup_big_tile_bits"}
# knobs read on the caller's context only (H2_PARENT_ONLY): the batch driver's and create_proof's
PARENT_ONLY = {"msm_lanes", "msm_stagger_sorts", "msm_fuse_cols", "msm_defer_reduce", "clean_on_lane", "plonk_warm_keygen", "plonk_tail_overlap",
               "plonk_side_on_lanes", "plonk_permute_in_commit", "plonk_merge_products", "plonk_shard_side", "plonk_route_rows", "plonk_lazy_upload",
               "plonk_early_intt", "plonk_gate_before_join"}


def _knob_table():
    """{name: (inherited, reason)} from H2_KNOB_TABLE"""
    src = open(os.path.join(ROOT, "halo2-lib_amd", "csrc", "internal.h")).read()
    start = src.index("#define H2_KNOB_TABLE(K)")
    end = src.index("\n\n", start)
    out = {}
    for m in re.finditer(r'K\(([a-z0-9_]+),\s*(H2_INHERITED|H2_PARENT_ONLY\("([^"]+)"\))', src[start:end]):
        out[m.group(1)] = (m.group(2) == "H2_INHERITED", m.group(3))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = emu_context()
    yield c
    c.close()


def test_knob_table_covers_exactly_the_accepted_names(ctx):
    table = _knob_table()
    assert set(table) == set(DOMAINS), (sorted(set(table) ^ set(DOMAINS)))
    for name in DOMAINS:
        ctx.get_param(name)   # accepted
    for bad in ("", "msm", "msm_window_bits ", "MSM_WINDOW_BITS", "ntt_w8", "is_lane", "profiling", "num_cus"):
        with pytest.raises(H.H2HipError):
            ctx.get_param(bad)
        with pytest.raises(H.H2HipError):
            ctx.set_param(bad, 0)


def test_defaults_are_legal():
    c = emu_context()   # a fresh context
    try:
        for name, (ok, _) in DOMAINS.items():
            v = c.get_param(name)
            assert v in ok or (name in RANGES and min(ok) <= v <= max(ok)), (name, v)
    finally:
        c.close()


@pytest.mark.parametrize("name", sorted(DOMAINS))
def test_domain(ctx, name):
    ok, bad = DOMAINS[name]
    default = ctx.get_param(name)
    try:
        for v in ok:
            ctx.set_param(name, v)
            assert ctx.get_param(name) == v, (name, v)
        for prev in (ok[0], ok[-1]):
            ctx.set_param(name, prev)
            for v in bad:
                with pytest.raises(H.H2HipError) as e:
                    ctx.set_param(name, v)
                assert e.value.code == -1 and name in str(e.value), (name, v, str(e.value))   # H2HIP_ERR_INVALID, with the knob named
                assert ctx.get_param(name) == prev, (name, v)   # the stored value stays
    finally:
        ctx.set_param(name, default)
    assert ctx.get_param(name) == default


def test_parent_only_knobs():
    table = _knob_table()
    parent_only = {n for n, (inh, _) in table.items() if not inh}
    assert parent_only == PARENT_ONLY, sorted(parent_only ^ PARENT_ONLY)
    assert all(len(why) > 10 for n, (inh, why) in table.items() if not inh)


def test_inherited_knobs_reach_every_child_context():
    """every inherited knob that selects a kernel path set to a non-default value on the PARENT only: the batch lanes and the prover's side
    context run with it, and the proof bytes still equal the oracle prover's (precomputed bases: the batch MSM's lanes carry the commitments)"""
    from tests.test_plonk_prover import _check

    inherited = {n for n, (inh, _) in _knob_table().items() if inh}
    path = {"msm_window_bits": 9, "msm_chunk": 7, "msm_chunk_lone": 5, "msm_seg": 2, "msm_quad_tails": 0, "msm_quad_seg_max": 1, "msm_sort_threads": 256,
            "msm_sort_groups": 3, "msm_hist_split": 2, "msm_hist_packed": 0, "msm_scatter_split": 4, "msm_scatter_full_lds": 1, "msm_table_split": 0,
            "ntt_tile_bits": 6, "ntt_min_col_bits": 1, "ntt_full_table": 0, "ntt_tile_kernel": 0, "quotient_29": 0, "kate_29": 0,
            "kate_coeffs_per_lane": 2, "fr_invert_run": 3, "lookup_big_tile_bits": 12, "host_poll": 0}
    assert set(path) == inherited - {"ntt_debug_skip"}   # (the diagnostic skip produces wrong results by design)
    c = emu_context()
    try:
        for n, v in path.items():
            assert c.get_param(n) != v, n
            c.set_param(n, v)
        out = _check(c, 6, 2, 1, 1, 1, 4, seed=5, threads=4, oracle_prover=True, precompute=True, second_proof=False)
        out[6].free()
        out[7].free()
        assert all(c.get_param(n) == v for n, v in path.items())
    finally:
        c.close()
