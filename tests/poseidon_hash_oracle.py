"""TEST INFRASTRUCTURE ONLY.  The sponge H of PoseidonHasher (halo2-base/src/poseidon/hasher/mod.rs: hash_fix_len_array, hash_var_len_array —
equal to pse-poseidon's native sponge, hasher/tests/hasher.rs:40-47,97-101,138-154) over oracle.poseidon.Spec's textbook permutation."""
import functools

from oracle.poseidon import Spec

SPECS = {3: (8, 57), 5: (8, 60)}   # the two instances the reference's own tests use


@functools.lru_cache(maxsize=None)
def spec(t, r_f=None, r_p=None):
    if r_f is None:
        r_f, r_p = SPECS[t]
    return Spec(t, r_f, r_p)


def init_state(t):
    return [1 << 64] + [0] * (t - 1)   # hasher/state.rs:20-25


def H(sp, m):
    """absorb m in chunks of RATE (a short chunk gets the padding 1), one more permutation of the empty chunk when len(m) is a multiple of
    RATE (0 included), digest = s[1]"""
    rate = sp.t - 1
    s = init_state(sp.t)
    for at in range(0, len(m), rate):
        s = sp.absorb_and_permute(s, m[at:at + rate])
    if len(m) % rate == 0:
        s = sp.absorb_and_permute(s, [])
    return s[1]


def merkle_tree(sp, leaves):
    """heap layout: nodes[n + i] = leaf i, nodes[j] = H([nodes[2j], nodes[2j+1]]), nodes[0] = 0"""
    n = len(leaves)
    nodes = [0] * n + list(leaves)
    for j in range(n - 1, 0, -1):
        nodes[j] = H(sp, [nodes[2 * j], nodes[2 * j + 1]])
    return nodes
