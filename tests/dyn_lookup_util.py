"""Shared by the dynamic-lookup tests (CPU-emulated and GPU): a RAMCircuit (virtual_region/tests/lookups/memory.rs:30-158) proven by libh2hip and
by the test-side CPU prover (tests/shape_oracle.py) on the same SRS and RNG stream."""
import numpy as np

from halo2_lib_amd import halo2_proofs as HP
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import virtual_region as V
from oracle import bn254 as O
from oracle import plonk as P
from tests import shape_oracle as SO
from tests.util import PreDrawnRng, R


def ram_circuit(k, accesses, mem_len, key_cols, lu_sets, seed, prank=False, num_fixed=1):
    """-> (RAMCircuit, DynLookupCircuitParams, advice, fixed, copies): memory values and access pointers drawn from `seed`"""
    g = np.random.default_rng(seed)
    memory = [int(v) for v in g.integers(1, 2**62, size=mem_len)]
    ptrs = [int(v) for v in g.integers(0, mem_len, size=accesses)]
    circ = V.RAMCircuit(memory, ptrs, key_cols, prank=prank)
    params = PL.DynLookupCircuitParams.new(k, circ.num_advice_needed(k), num_fixed, key_cols, lu_sets)
    advice, fixed, copies = circ.synthesize(params)
    return circ, params, advice, fixed, copies


def rng_budget(sh):
    n, bf = sh.n, sh.blinding_factors
    return (sh.num_advice_total * (bf + 2) + len(sh.lookups) * (2 * (bf + 1) + 2 + bf + 1) + sh.num_perm_sets * (bf + 1) + n + 1 +
            sh.quotient_poly_degree + 16)


def oracle_shape(params):
    return SO.Shape.dyn(params.k, params.num_advice, params.num_fixed, params.key_cols, params.lu_sets)


def srs(ctx, k, seed):
    s_toxic = 0x1D0C0FFEE1234567890ABCDEF + seed
    kzg = HP.ParamsKZG.setup(ctx, k, s_toxic)
    params = P.Params.setup(k, s_toxic, g=ctx.bases_download(kzg.g), g_lagrange=ctx.bases_download(kzg.g_lagrange))
    return kzg, params


def oracle_pk(sh, params, fixed, copies, threads):
    asm = P.PermutationAssembly(sh)
    for l, r in copies:
        asm.copy(l, r)
    return P.keygen(params, sh, fixed, asm, threads)


def vk_from_gpu(sh, gpk):
    pts = lambda a: O.limbs_to_points(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 8))
    return P.VerifyingKey(sh, pts(gpk.fixed_commitments), pts(gpk.permutation_commitments), gpk.transcript_repr)


def oracle_verify(params, vk, proof):
    return SO.oracle_verify(params, vk, [], proof)


def prove_both(ctx, k, accesses, mem_len, key_cols, lu_sets, seed, threads=2, oracle_prover=True):
    """keygen + create_proof on libh2hip and (oracle_prover) on the test prover.  -> (gpk, kzg, params, vk, proof, oracle proof or None, sh, advice)"""
    circ, dp, advice, fixed, copies = ram_circuit(k, accesses, mem_len, key_cols, lu_sets, seed)
    sh = oracle_shape(dp)
    kzg, params = srs(ctx, k, seed)
    gpk = PL.keygen(kzg, dp, fixed, copies)
    shape = gpk.shape
    assert (shape.degree, shape.extended_k, shape.blinding_factors, shape.usable_rows, shape.num_perm_sets, shape.num_fixed_total,
            shape.num_advice_total, shape.num_lookups, shape.table_col, shape.q_lookup_col) == (
        sh.degree, sh.extended_k, sh.blinding_factors, sh.usable_rows, sh.num_perm_sets, sh.num_fixed_total, sh.num_advice_total, len(sh.lookups), -1, -1)
    budget = rng_budget(sh)
    got = PL.create_proof(gpk, advice, [], PreDrawnRng(budget, 1000 + seed))
    want = None
    if oracle_prover:
        pk = oracle_pk(sh, params, fixed, copies, threads)
        assert pk.vk.transcript_repr == gpk.transcript_repr, "verifying keys differ (fixed / permutation commitments)"
        want = SO.create_proof(params, pk, advice, [], PreDrawnRng(budget, 1000 + seed), threads)
        vk = pk.vk
    else:
        vk = vk_from_gpu(sh, gpk)
    return gpk, kzg, params, vk, got, want, sh, advice


__all__ = ["ram_circuit", "rng_budget", "oracle_shape", "srs", "oracle_pk", "vk_from_gpu", "oracle_verify", "prove_both", "PreDrawnRng", "R"]
