"""Poseidon hashing times: h2hip_poseidon_hash_batch_dev and h2hip_poseidon_merkle_tree_dev next to the same work composed from
h2hip_poseidon_permute_batch_dev alone (what a caller could do before the hashing calls existed).
Usage: python tools/poseidon_hash_time.py [reps] [part ...]   parts: hash tree composed (default: all)
  hash      hash_batch of 2^20 messages of len 2, 8 and 64 at t = 3
  tree      merkle_tree of 2^10, 2^16 and 2^20 leaves at t = 3 and t = 5
  composed  the same trees and the len = 2 hash from the permutation call: per level one permutation from the initial state with the child pairs
            as inputs, for t = 3 a second one without inputs, then a strided copy of s[1]; and the permutation call alone (permutations / s)
`composed` uses only symbols every build has, and `hash` / `tree` are skipped when the library lacks the hashing calls, so the same script times a
build of an earlier commit.  Everything stays on the device, on one stream shared with torch (which does the state refill and the strided copy of
the composition); each timed call ends with a stream synchronisation.  Per case: median, min and max of `reps` calls after two warm-up calls, one
JSON line each."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_lib_amd as H  # noqa: E402
from oracle.poseidon import Spec  # noqa: E402
from tests.util import fr, rand_fr  # noqa: E402

args = sys.argv[1:]
reps = int(args[0]) if args and args[0].isdigit() else 10
parts = [a for a in args if not a.isdigit()] or ["hash", "tree", "composed"]
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = H.Context(stream=stream.cuda_stream)
lib = ctx.lib
have_hash = hasattr(lib, "h2hip_poseidon_hash_batch_dev") and hasattr(lib, "h2hip_poseidon_merkle_tree_dev")
SPECS = {3: Spec(3, 8, 57), 5: Spec(5, 8, 60)}
vp = C.c_void_p


def set_spec(t):
    sp = SPECS[t]
    ctx.poseidon_set_spec(t, sp.r_f, sp.r_p, fr([c for row in sp.constants for c in row]), fr([m for row in sp.mds for m in row]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def timed(name, fn, **info):
    for _ in range(2):
        fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    out = dict(case=name, **info, reps=reps, ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
    print(json.dumps(out), flush=True)
    return float(np.median(ts))


def permute(states, inputs, num_inputs, n):
    ctx._chk(lib.h2hip_poseidon_permute_batch_dev(ctx.handle, vp(states.data_ptr()), vp(inputs.data_ptr()) if num_inputs else None, num_inputs, n))


def composed_level(t, init, states, nodes, w):
    """nodes[w:2w] = H of the child pairs nodes[2w:4w], from the permutation call: the pairs are adjacent, so they are its inputs as they lie"""
    states[:w].copy_(init[:w])
    permute(states, nodes[2 * w:], 2, w)
    if t == 3:
        permute(states, None, 0, w)
    nodes[w:2 * w].copy_(states[:w, 1])


if "hash" in parts and have_hash:
    set_spec(3)
    n = 1 << 20
    for length in (2, 8, 64):
        inp, out = dev(rand_fr(n * length, 7)), torch.empty((n, 4), dtype=torch.int64, device="cuda")
        ms = timed("hash_batch", lambda: ctx._chk(lib.h2hip_poseidon_hash_batch_dev(ctx.handle, vp(out.data_ptr()), vp(inp.data_ptr()), length, None, n)),
                   t=3, n=n, len=length)
        print(json.dumps({"case": "hash_batch", "len": length, "permutations_per_s": round(n * (length // 2 + 1) / ms * 1e3)}), flush=True)
        del inp, out

if "tree" in parts and have_hash:
    for t in (3, 5):
        set_spec(t)
        for d in (10, 16, 20):
            nodes = torch.zeros((2 << d, 4), dtype=torch.int64, device="cuda")
            nodes[1 << d:].copy_(dev(rand_fr(1 << d, 9)))
            timed("merkle_tree", lambda: ctx._chk(lib.h2hip_poseidon_merkle_tree_dev(ctx.handle, vp(nodes.data_ptr()), None, d)), t=t, log_leaves=d)
            print(json.dumps({"case": "merkle_tree", "t": t, "log_leaves": d, "root": nodes[1].cpu().numpy().view(np.uint64).tolist()}), flush=True)
            del nodes

if "composed" in parts:
    for t in (3, 5):
        set_spec(t)
        nmax = 1 << 20
        init = torch.zeros((nmax, t, 4), dtype=torch.int64, device="cuda")
        init[:, 0] = dev(fr([1 << 64]))[0]
        states = torch.empty_like(init)
        for d in (10, 16, 20):
            nodes = torch.zeros((2 << d, 4), dtype=torch.int64, device="cuda")
            nodes[1 << d:].copy_(dev(rand_fr(1 << d, 9)))

            def tree():
                for lv in range(d - 1, -1, -1):
                    composed_level(t, init, states, nodes, 1 << lv)

            timed("composed_tree", tree, t=t, log_leaves=d)
            print(json.dumps({"case": "composed_tree", "t": t, "log_leaves": d, "root": nodes[1].cpu().numpy().view(np.uint64).tolist()}), flush=True)
            del nodes
        if t == 3:
            n = 1 << 20
            pairs = torch.zeros((4 * n, 4), dtype=torch.int64, device="cuda")   # laid out like a tree level: the pairs at [2n, 4n), the digests at [n, 2n)
            pairs[2 * n:].copy_(dev(rand_fr(2 * n, 7)))
            timed("composed_hash", lambda: composed_level(3, init, states, pairs, n), t=3, n=n, len=2)
            inp = dev(rand_fr(2 * n, 11))
            states.copy_(init)
            ms = timed("permute_batch", lambda: permute(states, inp, 2, n), t=3, n=n)
            print(json.dumps({"case": "permute_batch", "permutations_per_s": round(n / ms * 1e3)}), flush=True)
            del pairs, inp
ctx.close()
