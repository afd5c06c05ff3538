#!/usr/bin/env python3
"""
bench.py — headline benchmark of the MI355X prover backend (contract: see the task statement).

One step = ONE `create_proof` for the configuration BASELINE.json's metric is quoted on: the k = 19 secp256k1-ECDSA shape of
halo2-ecc/configs/secp256k1/bench_ecdsa.config:1 (`h2hip_plonk_create_proof`: Blake2b transcript, 12 MSMs of 2^19 points, the lookup sort, grand
products, h(X) over the 2^21-point extended domain, evaluations, SHPLONK; proof bytes out).  Inputs are resident in HBM when the
timed region starts: SRS tables, proving key and the advice column (`advice_on_device`); the blinding scalars come from the host RNG callback as
in the reference.

A plain run sets up, warms up, times the steps, writes `--dump-outputs` if asked and prints the result line: the metric and its value, the
configuration and the HBM roofline of the dominant kernel from the timed steps' own HIP events.  `--full` adds everything else below, all of it
after the timed steps: the checks of the timed proof (verified, the same bytes from host-resident advice and from every RNG path), the further
timings, the rooflines and accounts that take runs of their own, the CPU baseline and the side blocks.

  value        = constraints/s = assigned advice cells of the circuit / seconds per proof
  roofline     = the proof's dominant kernel, msm_accum_kernel: algorithmic 96 B x 2^19 per launch over its mean duration inside the timed
                 region (HIP events on the launch streams); with --full, `roofline_int`: the same launch against the binding roof, the 254-bit
                 multiplier peak measured in the same run; `roofline_proof`: the whole proof's algorithmic products / bytes over its wall time;
                 `seconds_per_proof_host_advice`: the same call with the advice column in host memory (the Vec the Rust prover fills; its
                 16 MiB upload inside the call), the PCIe-inclusive rate
  cpu_baseline = the oracle's restatement of the same prover ("port": identical step list, C kernels) on the box's host cores, one full
                 proof, whose BYTES are compared with the GPU proof's
  msm_2_20     = the other half of the metric (BASELINE configs[1]): G1-adds/s of 2^20-point MSMs with its own roofline and CPU line;
  ntt_2_22, k8_witness_batches, create_proof_in_flight, create_proof_k21_pairing_shape, create_proof_config_sweep: further blocks, outside the timed region.

Multi-GPU (`--gpus N` under torch.distributed.run): `--scaling strong` (default) = ONE k = 19 proof per step with its work sharded over the N
GPUs, every rank emitting the same proof bytes; `--scaling weak` = an independent proof per GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


# ---------------------------------------------------------------- the contract line (BENCH_r05.parsed was null under a 23.7 KB line)
CONTRACT_LINE_MAX_BYTES = 6000


def _sig(x, digits=6):
    """floats to `digits` significant digits (the line is read by a parser, not a numerics test); ints, bools, strings, None unchanged"""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        if x != x or x in (float("inf"), float("-inf")):
            return None            # strict JSON: no NaN / Infinity
        return float("%.*g" % (digits, x))
    if isinstance(x, dict):
        return {str(k): _sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, digits) for v in x]
    if isinstance(x, np.generic):
        return _sig(x.item(), digits)
    return str(x)


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def contract_line(out: dict, extra_file: str = "bench_extra.json") -> str:
    """The ONE line the driver parses: the contract keys + roofline / roofline_int / roofline_proof / cpu_baseline and a few headline figures of
    the side blocks, strict JSON, < CONTRACT_LINE_MAX_BYTES.  Everything else of `out` lives in `extra_file` (and on an earlier stdout line);
    a plain run writes no such file and passes extra_file=None.  Blocks that `out` does not hold are left out (a plain run's roofline_int)."""
    cfg = out.get("config", {})
    line = _pick(out, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    line["metric"] = str(line.get("metric", ""))[:160]
    line["dtype"] = str(line.get("dtype", ""))[:60]
    line["config"] = {"workload": str(cfg.get("workload_short") or cfg.get("workload", ""))[:300],
                      **_pick(cfg, "constraints_per_proof", "msm_count", "msm_size", "extended_k", "degree", "proof_bytes"),
                      "sharding": str(cfg.get("sharding", ""))[:120]}
    rf = out.get("roofline", {})
    line["roofline"] = {**_pick(rf, "bound", "achieved", "peak", "unit", "frac", "traffic", "frac_of_binding_roof", "algorithmic_bytes_per_launch",
                                "avg_launch_ms", "launches"), "kernel": str(rf.get("kernel", ""))[:80]}
    ri = out.get("roofline_int")
    if ri:   # --full only: the multiplier peak takes a run of its own
        line["roofline_int"] = {**_pick(ri, "achieved", "peak", "unit", "frac", "algorithmic_products_per_launch", "window_bits", "windows"),
                                "kernel": str(ri.get("kernel", ""))[:40]}
    rp = out.get("roofline_proof", {})
    if rp:
        line["roofline_proof"] = {"products": rp.get("algorithmic", {}).get("products"), "bytes": rp.get("algorithmic", {}).get("bytes"),
                                  "int": _pick(rp.get("int", {}), "achieved", "peak", "unit", "frac", "ideal_ms"),
                                  "hbm": _pick(rp.get("hbm", {}), "achieved", "peak", "unit", "frac")}
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        c = _pick(cb, "value", "unit", "cores", "kind", "seconds", "threads", "proof_bytes_equal_to_gpu", "error")
        if "sample" in cb:
            c["sample"] = str(cb["sample"])[:160]
        if "error" in c:
            c["error"] = str(c["error"])[:200]
        line["cpu_baseline"] = c
    line.update(_pick(out, "speedup_vs_cpu_port", "seconds_per_proof_host_advice", "value_host_advice", "proof_verified_by_h2hip_plonk_verify_proof",
                      "proof_repeatable", "sharded_bytes_equal_unsharded"))
    m = next((out[k] for k in out if k.startswith("msm_2_") and isinstance(out[k], dict)), None)
    if m is not None:
        line["msm_2_20"] = {**_pick(m, "value", "unit", "ms_per_msm", "window_bits", "windows", "error"),
                            "int_frac": (m.get("roofline_int") or {}).get("frac"), "hbm_frac": (m.get("roofline") or {}).get("frac"),
                            "cpu_value": (m.get("cpu_baseline") or {}).get("value")}
    t = out.get("ntt_2_22")
    if isinstance(t, dict):
        line["ntt_2_22"] = {**_pick(t, "ntt_ms", "intt_ms", "roundtrip_bit_exact", "error"),
                            "int_frac": (t.get("roofline_int") or {}).get("frac"), "hbm_frac": (t.get("roofline") or {}).get("frac")}
    p21 = out.get("create_proof_k21_pairing_shape")
    if isinstance(p21, dict):
        b = _pick(p21, "seconds", "seconds_host_advice", "constraints_per_sec", "equals_committed_oracle_prover_digest", "verified_by_h2hip_plonk_verify_proof", "error")
        rp21 = p21.get("roofline_proof") or {}
        b["roofline_proof"] = {"products": (rp21.get("algorithmic") or {}).get("products"), "int_frac": (rp21.get("int") or {}).get("frac"),
                               "hbm_frac": (rp21.get("hbm") or {}).get("frac")}
        sh_ = p21.get("sharded")
        if isinstance(sh_, dict):
            b["sharded"] = _pick(sh_, "seconds", "world", "proof_bytes_equal_one_gpu", "equals_committed_oracle_prover_digest")
        if "error" in b:
            b["error"] = str(b["error"])[:200]
        line["create_proof_k21_pairing_shape"] = b
    cm = out.get("comm")
    if isinstance(cm, dict):
        line["comm"] = {"transport": str(cm.get("transport", ""))[:60], "distinct_gpus": cm.get("distinct_gpus"), "ranks": len(cm.get("ranks") or [])}
    ip = out.get("independent_proofs_per_gpu")
    if isinstance(ip, dict):
        line["independent_proofs_per_gpu"] = _pick(ip, "ms_per_step", "value", "unit", "scaling")
    if extra_file:
        line["extra"] = extra_file
    text = json.dumps(_sig(line), allow_nan=False, separators=(",", ":"))
    if len(text) >= CONTRACT_LINE_MAX_BYTES:   # never happens with the caps above; if it does, drop the side blocks rather than the contract keys
        for k in ("independent_proofs_per_gpu", "comm", "ntt_2_22", "msm_2_20", "create_proof_k21_pairing_shape", "roofline_proof"):
            line.pop(k, None)
            text = json.dumps(_sig(line), allow_nan=False, separators=(",", ":"))
            if len(text) < CONTRACT_LINE_MAX_BYTES:
                break
    assert len(text) < CONTRACT_LINE_MAX_BYTES, len(text)
    return text


def emit(out: dict) -> None:
    """bench_extra.json (+ gpurun_out/ when present) and an EARLIER stdout line (prefixed, so that no line-oriented parser takes it for the
    contract line) carry everything; the LAST stdout line is the compact contract line."""
    full = json.dumps(_sig(out, 9), allow_nan=False)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_extra.json"), "w") as f:
                    f.write(full + "\n")
            except OSError:
                pass
    sys.stdout.write("# bench_extra " + full + "\n")
    sys.stdout.flush()
    print(contract_line(out), flush=True)


# ---------------------------------------------------------------- --dump-outputs: what the timed path returned, so that two builds can be compared
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """DIR/<name>.npy per array, as float32 (exact for the byte values of a proof); refuses more than DUMP_MAX_BYTES in all"""
    conv = {name: np.asarray(a).astype(np.float32) for name, a in arrays.items()}
    total = sum(a.nbytes for a in conv.values())
    if total > DUMP_MAX_BYTES:
        raise ValueError("--dump-outputs: %d bytes exceed the %d-byte limit" % (total, DUMP_MAX_BYTES))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in conv.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ---------------------------------------------------------------- synthetic inputs (no oracle involved)
def _g1_add(P, S):
    (x1, y1), (x2, y2) = P, S
    if x1 == x2:
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return (x3, (lam * (x1 - x3) - y1) % Q)


def _limbs(vals, p):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    mask = (1 << 64) - 1
    for i, v in enumerate(vals):
        v = (v << 256) % p   # Montgomery form
        out[i] = [(v >> (64 * k)) & mask for k in range(4)]
    return out


def _g1_mul(k: int, P=(1, 2)):
    """k*P by double-and-add in affine big-int arithmetic (None = identity); used only to verify the timed results"""
    acc = None
    for bit in bin(k % R)[2:] if k % R else "":
        acc = None if acc is None else _g1_add(acc, acc)
        if bit == "1":
            acc = P if acc is None else _g1_add(acc, P)
    return acc


def known_dlog_bases_gpu(ctx, torch, dev, n: int, k0: int, d: int, first_index: int = 0):
    """n DISTINCT bases P_i = (k0 + (first_index + i)*d) * G built on the GPU (h2hip_g1_fixed_base_mul_batch_dev); returns a device
    tensor of n G1Affine points.  Because the discrete logs are known, an MSM over them has the closed form
    (sum_i s_i*(k0 + i*d)) * G, which bench.py uses to verify the timed results without any CPU MSM."""
    assert k0 + (first_index + n) * d < 1 << 63
    e = np.zeros((n, 4), dtype=np.uint64)
    e[:, 0] = np.uint64(k0) + (np.uint64(first_index) + np.arange(n, dtype=np.uint64)) * np.uint64(d)   # canonical integers
    r2 = _limbs([1 << 256], R)                                                       # Montgomery form of R: x (*) R^2 = x*R
    d_e = torch.from_numpy(e.view(np.int64)).to(dev)
    d_r2 = torch.from_numpy(np.repeat(r2, n, axis=0).view(np.int64)).to(dev)
    ctx._chk(ctx.lib.h2hip_fr_mul_batch_dev(ctx.handle, d_e.data_ptr(), d_e.data_ptr(), d_r2.data_ptr(), n))   # -> Montgomery limbs
    pts = torch.empty(n * 8, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()   # the context may run on a stream torch does not know about
    g = np.concatenate([_limbs([1], Q), _limbs([2], Q)], axis=1)
    ctx._chk(ctx.lib.h2hip_g1_fixed_base_mul_batch_dev(ctx.handle, g.ctypes.data, d_e.data_ptr(), n, pts.data_ptr()))
    ctx.sync()
    return pts


def closed_form_dlog(scal_limbs: np.ndarray, k0: int, d: int, first_index: int = 0) -> int:
    """sum_i v_i * (k0 + (first_index+i)*d) mod r for scalars given as raw Montgomery limbs (v_i = limbs_i / 2^256), vectorised:
    every 64-bit limb is split into 16-bit pieces so that the index-weighted sums stay below 2^64."""
    a = np.ascontiguousarray(scal_limbs, dtype=np.uint64).reshape(-1, 4)
    n = len(a)
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    s0 = s1 = 0
    for limb in range(4):
        for piece in range(4):
            v = (a[:, limb] >> np.uint64(16 * piece)) & np.uint64(0xFFFF)
            shift = 64 * limb + 16 * piece
            s0 += int(v.sum(dtype=np.uint64)) << shift
            s1 += int((v * idx).sum(dtype=np.uint64)) << shift
    return (s0 * k0 + s1 * d) * pow(1 << 256, -1, R) % R


def jac_to_affine(j):
    """(12,) u64 Montgomery limbs of a Jacobian point -> affine integer pair or None"""
    vals = []
    rinv = pow(1 << 256, -1, Q)
    for c in range(3):
        row = [int(x) for x in np.asarray(j).reshape(12)[4 * c:4 * c + 4]]
        vals.append((row[0] | row[1] << 64 | row[2] << 128 | row[3] << 192) * rinv % Q)
    X, Y, Z = vals
    if Z == 0:
        return None
    zi = pow(Z, -1, Q)
    return (X * zi * zi % Q, Y * zi * zi * zi % Q)


def synthetic_scalars(n: int, seed: int) -> np.ndarray:
    """uniform random valid F_r elements (raw Montgomery limbs, value < 2^252 < r)."""
    g = np.random.default_rng(seed)
    a = g.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def window_for(ctx, n):
    c = ctx.get_param("msm_window_bits")
    if c == 0:   # mirror of pick_window() in msm_tables.hip
        best, best_cost = 4, float("inf")
        for cc in range(4, 21):
            W = (255 + cc - 1) // cc
            cost = W * (10.0 * n + 28.0 * (1 << (cc - 1)) + 400.0 * cc)
            if cost < best_cost:
                best, best_cost = cc, cost
        c = best
    return c, (255 + c - 1) // c


def kernel_account(ctx, proofs):
    """{kernel: {"ms": per proof, "launches": per proof, "busy_ms": per proof}} from the library's HIP-event profile (h2hip_profile_dump)"""
    acc = {}
    for name, (ms, cnt, busy) in sorted(ctx.profile_dump().items(), key=lambda kv: -kv[1][0]):
        acc[name] = {"ms": round(ms / proofs, 4), "launches": round(cnt / proofs, 2), "busy_ms": round(busy / proofs, 4)}
    return acc


def proof_algorithmic_work(ctx, bp, sh):
    """the algorithmic work of one create_proof for a BaseCircuitParams shape (SURVEY.md §8d's formulas, summed over the proof's MSMs and
    transforms): 254-bit products = 10*n*W per MSM (XYZZ mixed addition, window of the implementation) + (m/2)*log2(m) per transform of m
    points; bytes = 96 B per (scalar, base) pair + 64 B per transformed element"""
    k, n = bp.k, 1 << bp.k
    c, W = window_for(ctx, n)
    msms = sh.num_commitments
    A, L, P = sh.num_advice_total, sh.num_lookups, sh.num_perm_sets
    cols = A + 3 * L + P                       # columns that go Lagrange -> coefficients -> extended coset
    ext = sh.extended_k
    intt, cntt, cintt = cols * (n // 2) * k, cols * ((1 << ext) // 2) * ext, ((1 << ext) // 2) * ext
    return {"msm_count": msms, "msm_window_bits": c, "msm_windows": W, "msm_products": 10.0 * n * W * msms,
            "transforms": {"lagrange_to_coeff": cols, "coeff_to_extended": cols, "extended_to_coeff": 1},
            "ntt_products": float(intt + cntt + cintt), "products": 10.0 * n * W * msms + intt + cntt + cintt,
            "bytes": 96.0 * n * msms + 64.0 * (cols * n + cols * (1 << ext) + (1 << ext))}


def measure_hbm_traffic(k, kernel="msm_accum_kernel"):
    """roofline.traffic: HBM bytes per launch of the dominant kernel from the PMC counters, collected as MI355X_MICROARCH.md's HBM / rocprofv3
    section prescribes — two SEPARATE `rocprofv3 --kernel-trace --pmc <counter>` passes (FETCH_SIZE, WRITE_SIZE) over a child run of this file's
    timed workload only (`--pmc-child`), bytes = (2 x FETCH_SIZE_KB + WRITE_SIZE_KB) x 1024: on gfx950 FETCH_SIZE tallies 128-byte requests as
    64 B (the guide's correction; calibration in profiles/archive/r02_hbm_counter_calibration.md).  Returns None (with the reason) if rocprofv3 is missing."""
    import glob
    import shutil
    import sqlite3
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    vals = {}
    tmp = tempfile.mkdtemp(prefix="h2pmc_", dir="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "-d", out, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--pmc-child", "--k", str(k),
                   "--steps", "4", "--warmup", "1"]
            env = dict(os.environ, TMPDIR="/tmp")
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=150)
            dbs = glob.glob(os.path.join(out, "**", "*.db"), recursive=True)
            if r.returncode != 0 or not dbs:
                return None, "%s pass failed (rc %d): %s" % (counter, r.returncode, (r.stderr or r.stdout)[-300:])
            db = sqlite3.connect(dbs[0])
            rows = db.execute("select kernel_name, count(*), avg(value) from counters_collection where counter_name=? and kernel_name like ? group by kernel_name",
                              (counter, "%" + kernel + "%")).fetchall()
            if not rows:
                return None, "no %s samples for %s" % (counter, kernel)
            vals[counter] = (sum(r_[1] * r_[2] for r_ in rows) / sum(r_[1] for r_ in rows), sum(r_[1] for r_ in rows))
        traffic = (2.0 * vals["FETCH_SIZE"][0] + vals["WRITE_SIZE"][0]) * 1024.0
        return {"bytes_per_launch": traffic, "fetch_size_kb_raw": vals["FETCH_SIZE"][0], "write_size_kb": vals["WRITE_SIZE"][0], "launches_sampled": vals["FETCH_SIZE"][1],
                "how": "two separate `rocprofv3 --kernel-trace --pmc FETCH_SIZE|WRITE_SIZE` child runs of `bench.py --pmc-child --steps 4` inside this run; "
                       "bytes = (2 x FETCH_SIZE_KB + WRITE_SIZE_KB) x 1024 (gfx950: FETCH_SIZE counts a 128-byte request as 64 B); mean over the child's launches of the "
                       "kernel (keygen's and the proofs' MSMs of 2^k points)"}, None
    except Exception as e:   # never let the optional measurement break the contract line
        return None, repr(e)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def headline(args, world, sharded, sh, cells, seconds, proof_bytes, msm_n, k_ms, k_cnt, k_busy_ms):
    """the result line's own fields, the same in a plain and a --full run: the metric and its value from the timed steps, the configuration, and
    the HBM roofline of the dominant kernel from the HIP events the timed steps carry (k_ms / k_cnt / k_busy_ms: h2hip_profile_get(_busy))"""
    k, n = args.k, 1 << args.k
    proofs_per_step = 1 if (world == 1 or sharded) else world
    k_avg_s = k_ms / max(k_cnt, 1) * 1e-3
    alg_bytes = 96.0 * msm_n
    return {
        "metric": ("create_proof constraints/sec (k=19 ECDSA configuration, halo2-ecc/configs/secp256k1/bench_ecdsa.config:1); MSM G1-adds/sec in `msm_2_%d`" % args.log_n) if k == 19 else
                  ("create_proof constraints/sec (--k %d: bench_ecdsa.config:1's 1 + 1 + 1 COLUMN SHAPE at another k — not a configuration of the reference; the k=21 "
                   "reference configuration is the pairing shape in `create_proof_k21_pairing_shape`); MSM G1-adds/sec in `msm_2_%d`" % (k, args.log_n)),
        "value": proofs_per_step * cells / seconds,
        "unit": "constraints/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": seconds * 1e3,
        "higher_is_better": True,
        "scaling": ("strong" if sharded else "weak") if world > 1 else args.scaling,   # N = 1: the mode the N > 1 lines of the same command use
        "vs_baseline": None,
        "dtype": "u32 (254-bit Montgomery integers as 8x32 / 9x29-bit limbs)",
        "data": "synthetic",
        "config": {"workload": "BASELINE configs[3]: h2hip_plonk_create_proof for the k=%d secp256k1-ECDSA configuration (bench_ecdsa.config:1: 1 advice column with the "
                               "lookup behind q_lookup, 1 constants column, lookup_bits %d, no instances), synthetic circuit-like witness (halo2_lib_amd/testing.py: "
                               "every gate satisfied, 0/1 / small / full-width cells, range-checked cells, copy constraints); one step = one proof: host wall clock "
                               "around the C call with the advice column resident in HBM (advice_on_device), incl. the generation of the 2^k blinding scalars (ChaCha12 "
                               "Fr::random stream of StdRng::seed_from_u64(0), on the device) and the proof bytes coming back; `seconds_per_proof_host_advice` = the same with the advice column staged from host "
                               "memory inside the call; witness generation (CPU gadgets, Rust) excluded" % (k, k - 1),
                   "workload_short": "BASELINE configs[3]: h2hip_plonk_create_proof, k=%d secp256k1-ECDSA shape (bench_ecdsa.config:1: 1 advice + 1 lookup + 1 constants column, "
                                     "lookup_bits %d), synthetic circuit-like witness resident in HBM; 1 step = 1 proof, bytes back on the host" % (k, k - 1),
                   "value_is": "constraints / seconds_per_proof with the advice column RESIDENT IN HBM when the timed region starts (the bench contract); the like-for-like "
                               "figure against a CPU prover (witness in host memory, its 16 MiB upload inside the call) is seconds_per_proof_host_advice / "
                               "value_host_advice — what speedup_vs_cpu_port is computed from",
                   "constraints_per_proof": cells, "constraints_definition": "assigned advice cells (SURVEY.md §8d)", "msm_count": sh.num_commitments, "msm_size": n,
                   "extended_k": sh.extended_k, "degree": sh.degree, "proof_bytes": proof_bytes,
                   "sharding": ("ONE proof per step over %d GPUs: commitments point-range sharded (2^%d / %d points per GPU), see DESIGN.md §6" % (world, k, world)) if sharded else
                               ("none (1 GPU)" if world == 1 else "%d independent proofs per step, one per GPU (replicas, no exchange)" % world)},
        "seconds_per_proof": seconds,
        "roofline": {"bound": "hbm", "kernel": "msm_accum_kernel (2^%d points per launch, %d launches per proof)" % (int(np.log2(msm_n)), round(k_cnt / args.steps)),
                     "achieved": alg_bytes / k_avg_s / 1e9 if k_avg_s > 0 else 0.0, "peak": 8000.0, "unit": "GB/s",
                     "frac": alg_bytes / k_avg_s / 8e12 if k_avg_s > 0 else 0.0,
                     "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": k_avg_s * 1e3, "launches": int(k_cnt),
                     "busy_ms_per_launch": k_busy_ms / max(k_cnt, 1)},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed create_proof calls (one step = one k=19 proof)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=19, help="the metric's configuration is k=19 (bench_ecdsa.config:1); other k: the same 1+1+1 column shape")
    ap.add_argument("--log-n", type=int, default=20, help="size of the MSM block (BASELINE configs[1])")
    ap.add_argument("--msm-steps", type=int, default=128, help="timed MSMs of the MSM block")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="N > 1, top-level line: strong = ONE k=19 proof per step, sharded over the N GPUs (north star; default); weak = every rank "
                         "proves its own circuit (independent replicas, no exchange).  The MSM block follows the same choice.")
    ap.add_argument("--sharded-proof", action="store_true", help="accepted for compatibility: with --gpus N > 1 the top-level line already IS the sharded k=19 proof (--scaling strong)")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, default) or gloo (exchange staged through the host; testing)")
    ap.add_argument("--shard-ntt-columns", choices=["auto", "on", "off"], default="auto",
                    help="sharded proof: lagrange_to_coeff dealt by column (H2HIP_SHARD_NTT_COLUMNS); auto = from 8 ranks")
    ap.add_argument("--share-device", action="store_true", help="testing on a 1-GPU box: every rank uses GPU 0 (requires --dist-backend gloo)")
    ap.add_argument("--param", action="append", default=[], help="name=value tuning knob passed to h2hip_set_param (repeatable)")
    ap.add_argument("--lanes", type=int, default=0, help="override msm_lanes (streams used by the batch API)")
    ap.add_argument("--no-replay", action="store_true", help="skip the MSM 2^20, NTT 2^22, K8 and k=21 blocks (extra fields)")
    ap.add_argument("--no-pmc-traffic", action="store_true", help="skip the two rocprofv3 PMC child runs (FETCH_SIZE / WRITE_SIZE) that fill roofline.traffic")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)   # set on the child runs: only the timed workload, no blocks, no children
    ap.add_argument("--no-sweep", action="store_true", help="skip create_proof over the reference's 18 benchmark shapes (an extra field, ~25 s)")
    ap.add_argument("--precompute", type=int, default=1, help="1: bases carry precomputed 2^(c*w) window tables (fixed-base SRS, H2HIP_BASES_PRECOMPUTE)")
    ap.add_argument("--batch", type=int, default=4, help="MSM block: MSMs issued per h2hip_msm_g1_batch_dev call (a prover commits several columns per round); 1 = synchronous")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's proof bytes to DIR/proof.npy (float32, one value per byte; rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also check the proof and run every further measurement (host-resident advice, RNG paths, kernel "
                         "account, rooflines, PMC traffic, CPU baseline, side blocks) and write bench_extra.json; the --no-* switches trim this")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch

    import halo2_lib_amd as H
    from halo2_lib_amd import halo2_proofs as HP
    from halo2_lib_amd import plonk as PL
    from halo2_lib_amd import testing as T

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.share_device:
            assert args.dist_backend == "gloo", "--share-device needs --dist-backend gloo (RCCL refuses two ranks on one GPU)"
            local_rank = 0
        torch.cuda.set_device(local_rank)
        if args.dist_backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=args.dist_backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    xdev = dev if args.dist_backend == "nccl" else None   # where the all-gather tensors live
    # a non-default torch stream: the legacy null stream adds implicit synchronisation to every launch
    tstream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(tstream)
    ctx = H.Context(device=local_rank, stream=tstream.cuda_stream)
    if args.lanes:
        ctx.set_param("msm_lanes", args.lanes)
    for kv in args.param:
        name, val = kv.split("=")
        ctx.set_param(name, int(val))

    # ------------------------------------------------------------------ the metric's configuration: create_proof, k = 19 ECDSA shape
    k = args.k
    n = 1 << k
    s_toxic = 0x1D0C0FFEE1234567890ABCDEF
    sharded = world > 1 and args.scaling == "strong"
    bp = PL.BaseCircuitParams.new(k, 1, 1, 1, 0, k - 1)
    sh = PL.shape_of(ctx, bp)

    class Backend:   # the synthetic witness is computed through the K8 batch kernels
        mul = staticmethod(ctx.fr_mul)
        add = staticmethod(ctx.fr_add)

    # set-up without collectives; the ranks then agree that all of them got through it before the first sharded proof
    err = None
    try:
        kzg = HP.ParamsKZG.setup(ctx, k, s_toxic, precompute=not sharded)   # sharded: only the rank's slice gets window tables
        circ = T.build_circuit(_ShapeView(bp, sh), 19 + (0 if sharded else rank), Backend)
        t0 = time.perf_counter()
        pk = PL.keygen(kzg, bp, circ.fixed, circ.copies)
        keygen_s = time.perf_counter() - t0
    except Exception as e:
        if world == 1:
            raise
        err = repr(e)
    sk, comm = None, None
    if world > 1:
        oks = [None] * world
        dist.all_gather_object(oks, err)
        if any(o is not None for o in oks):
            raise SystemExit("bench.py: set-up failed on some rank: %r" % (oks,))
        from halo2_lib_amd.multi_gpu import Comm, shard_proving_key

        comm = Comm(ctx, rccl=args.dist_backend == "nccl", device=xdev)   # libh2hip's own communicator (RCCL over xGMI / a gloo callback)
        if sharded:
            sk = shard_proving_key(pk, ctx.bases_download(kzg.g), ctx.bases_download(kzg.g_lagrange), device=xdev, precompute=True, comm=comm,
                                   shard_ntt_columns={"auto": None, "on": True, "off": False}[args.shard_ntt_columns])
        # what the N-rank run actually ran on: libh2hip's view of its communicator (h2hip_comm_info) and every rank's GPU, gathered for the line
        import ctypes as _C

        cw, cr, crccl = _C.c_int(), _C.c_int(), _C.c_int()
        ctx._chk(ctx.lib.h2hip_comm_info(comm.handle, _C.byref(cw), _C.byref(cr), _C.byref(crccl)))
        props = torch.cuda.get_device_properties(local_rank)
        mine = {"rank": cr.value, "world": cw.value, "is_rccl": bool(crccl.value), "cuda_device": local_rank, "gpu_name": props.name,
                "gpu_uuid": str(getattr(props, "uuid", "")), "pci_bus_id": getattr(props, "pci_bus_id", None)}
        comm_ranks = [None] * world
        dist.all_gather_object(comm_ranks, mine)

    # the timed proofs take the advice columns RESIDENT IN HBM (advice_on_device: the bench contract times the hot path with its inputs on the
    # device); the same call with the columns in host memory — the Vec the Rust prover fills, staged over PCIe inside the call — is timed
    # next to it (`seconds_per_proof_host_advice`).  The RNG stream is a host callback in both, as it is in the reference.
    adv_dev = [ctx.to_device(np.ascontiguousarray(c)) for c in circ.advice]
    prove = lambda stages=None: PL.create_proof(pk, adv_dev, circ.instances, PL.ChaChaRng(ctx.lib, 0, 12), stages, advice_on_device=True)
    t0 = time.perf_counter()
    first = prove()                      # the cold first proof after keygen (allocates the key's buffer pool, builds twiddle tables)
    cold_s = time.perf_counter() - t0
    for _ in range(max(0, args.warmup - 1)):
        prove()
    ctx.profile_reset()
    ctx.profile_filter("msm_accum_kernel")   # the timed region carries HIP events around the dominant kernel's launches only (12 per proof)
    ctx.profile_enable(True)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(args.steps):
        if args.pmc_child and step == args.steps - 1:
            ctx.bench_modmul(1, 1)       # a kernel the prover never launches: tools/rocprof_proof.py / rocprof_timeline.py take what follows the last one as ONE timed proof
        proof = prove()                  # returns after the proof bytes are on the host
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ctx.profile_enable(False)
    if world > 1:
        te = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        elapsed = float(te.item())
    seconds = elapsed / args.steps
    if args.dump_outputs and rank == 0:   # create_proof returns the proof bytes and nothing else
        dump_outputs(args.dump_outputs, {"proof": np.frombuffer(proof, dtype=np.uint8)})
    if args.pmc_child:   # a rocprofv3 PMC pass of the parent: the timed workload is all it wants
        pk.free()
        kzg.free()
        ctx.close()
        return
    if proof != first:
        raise SystemExit("bench.py: create_proof is not repeatable for a fixed RNG stream — refusing to report a number")
    # the timed steps' HIP events around msm_accum_kernel (profiling is off from here on, so later proofs add nothing to them)
    k_ms, k_cnt = ctx.profile_get("msm_accum_kernel")
    k_busy_ms = ctx.profile_get_busy("msm_accum_kernel")
    cells = 4 * (sh.usable_rows // 4)    # assigned advice cells: `constraints` of SURVEY.md §8d (total_advice of the circuit)
    msm_n = n // world if sharded else n
    if not args.full:   # a plain run: the result line and nothing else
        if rank == 0:
            print(contract_line(headline(args, world, sharded, sh, cells, seconds, len(proof), msm_n, k_ms, k_cnt, k_busy_ms), extra_file=None), flush=True)
        if sk is not None:
            sk.free()
        pk.free()
        kzg.free()
        if comm is not None:
            comm.destroy()
        ctx.close()
        if world > 1:
            dist.destroy_process_group()
        return

    # ------------------------------------------------------------------ --full: everything below runs after the timed steps
    # the prover's randomness: the reference hands create_proof `StdRng::seed_from_u64(0)` (halo2-base/src/utils/testing.rs:38) = ChaCha12 in
    # counter mode.  libh2hip's seeded generator reproduces that Fr::random stream and the prover generates its 2^k blinding scalars ON THE
    # DEVICE inside the timed call (PL.ChaChaRng, csrc/rng.hip).  `draws` = the same stream as an array (generated by the same kernel, once):
    # what the pre-drawn-array comparison figure and the CPU baseline consume, so that all of them produce the SAME proof bytes.
    rng_seed = PL.ChaChaRng(ctx.lib, 0, 12).state.seed
    d_draws = ctx.malloc(32 * (n + 4096))
    ctx._chk(ctx.lib.h2hip_rng_chacha_fill_dev(ctx.handle, d_draws, n + 4096, rng_seed, 12, 0))
    draws = ctx.download(d_draws, (n + 4096, 4))
    ctx.free(d_draws)
    prove_host = lambda: PL.create_proof(pk, circ.advice, circ.instances, PL.ChaChaRng(ctx.lib, 0, 12))
    prove_array = lambda: PL.create_proof(pk, adv_dev, circ.instances, PL.ArrayRng(draws), advice_on_device=True)
    prove_host_rng = lambda: PL.create_proof(pk, adv_dev, circ.instances, PL.ChaChaRng(ctx.lib, 0, 12, device=False), advice_on_device=True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        proof_host = prove_host()        # every rank: a sharded proof has collectives inside
    host_advice_s = (time.perf_counter() - t0) / args.steps
    if proof_host != proof:
        raise SystemExit("bench.py: host-resident and device-resident advice columns gave different proofs")
    if not PL.verify_proof(pk, circ.instances, proof):
        raise SystemExit("bench.py: the timed proof does not verify — refusing to report a number")
    # the same proof with its randomness prepared OUTSIDE the call (a pre-drawn array: what r03's headline timed) and with the stream generated
    # by the library's one-thread host generator inside the call (what a host-side rand_chacha would cost the caller): same bytes, both timed
    prove_array()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        proof_array = prove_array()
    array_rng_s = (time.perf_counter() - t0) / args.steps
    t0 = time.perf_counter()
    proof_host_rng = prove_host_rng()
    host_rng_s = time.perf_counter() - t0
    if proof_array != proof or proof_host_rng != proof:
        raise SystemExit("bench.py: the device-generated, host-generated and pre-drawn RNG streams gave different proofs")
    if world > 1:
        import hashlib

        digests = [None] * world
        dist.all_gather_object(digests, hashlib.sha256(proof).hexdigest())
        if sharded and len(set(digests)) != 1:
            raise SystemExit("bench.py: the ranks of a sharded proof emitted different bytes")

    out = None
    ctx.profile_filter("")
    k_avg_s = k_ms / max(k_cnt, 1) * 1e-3
    # outside the timed region: the same call with every kernel bracketed (the per-kernel account; ~200 launches x 2 events cost ~1 ms per proof),
    # then with per-stage laps (a stream synchronisation per stage)
    acct_proofs = 5
    ctx.profile_reset()
    ctx.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(acct_proofs):
        prove()
    all_profiled_s = (time.perf_counter() - t0) / acct_proofs
    ctx.profile_enable(False)
    stages = {}
    prove(stages)                        # every rank: a sharded proof has collectives inside
    if rank == 0:
        account = kernel_account(ctx, acct_proofs)
        busy_all_ms = ctx.profile_get_busy("") / acct_proofs
        mm_ms, mm_n = ctx.bench_modmul(16384, 256, 2)
        modmul_peak_sat = mm_n / (mm_ms * 1e-3)
        mm_ms, mm_n = ctx.bench_modmul(16384, 256, 2, unsaturated=True)
        modmul_peak = mm_n / (mm_ms * 1e-3)
        work = proof_algorithmic_work(ctx, bp, sh)
        c19, W19 = window_for(ctx, msm_n)
        proofs_per_step = 1 if (world == 1 or sharded) else world
        traffic_prof = None
        pmc_path = os.path.join(ROOT, "profiles", "r06_create_proof_k19_pmc_hbm.json")
        if not os.path.exists(pmc_path):
            pmc_path = os.path.join(ROOT, "profiles", "r05_create_proof_k19_pmc_hbm.json")
        if os.path.exists(pmc_path) and k == 19 and world == 1:
            import hashlib
            import subprocess

            raw = open(pmc_path, "rb").read()
            blob = hashlib.sha1(b"blob %d\0" % len(raw) + raw).hexdigest()   # = `git hash-object`: ties the quoted figure to the committed file
            traffic_prof = {"source": os.path.relpath(pmc_path, ROOT), "git_blob_sha1": blob, **json.loads(raw)}
        traffic_live, traffic_err = (None, "skipped (--no-pmc-traffic)")
        if world == 1 and not args.no_pmc_traffic:
            traffic_live, traffic_err = measure_hbm_traffic(k)
        out = headline(args, world, sharded, sh, cells, seconds, len(proof), msm_n, k_ms, k_cnt, k_busy_ms)
        out["roofline"].update({
            "bound_note": "bound / achieved / peak / unit / frac are the HBM figures the bench contract asks for (algorithmic bytes over the launch duration against "
                          "8 TB/s); the roof that BINDS this kernel is the 254-bit integer multiplier: `frac_of_binding_roof` = `roofline_int.frac`",
            "frac_of_binding_roof": (10.0 * msm_n * W19 / k_avg_s / modmul_peak) if k_avg_s > 0 else 0.0,
            "traffic": traffic_live["bytes_per_launch"] if traffic_live else None,
            "traffic_measurement": traffic_live if traffic_live else {"error": traffic_err},
            "traffic_note": "HBM bytes per launch from the PMC counters of two rocprofv3 child runs inside this run (null if rocprofv3 is unavailable: the "
                            "separately collected, committed figure is under `traffic_from_profiles` with the file's git blob hash)",
            "traffic_from_profiles": traffic_prof,
            "note": "algorithmic bytes = 96 B per (scalar, base) pair (SURVEY.md §8d); avg_launch_ms = mean duration of the kernel's launches inside the "
                    "timed region, HIP events on the launch streams (h2hip_profile_*); the binding roof of this kernel is the integer multiplier: `roofline_int`"})
        out.update({
            "seconds_per_proof_host_advice": host_advice_s, "value_host_advice": proofs_per_step * cells / host_advice_s,
            "seconds_per_proof_with_rng": {"device_generated_chacha12": seconds, "host_generated_chacha12_one_thread": host_rng_s, "predrawn_array_outside_the_call": array_rng_s,
                                           "proof_bytes_identical": True,
                                           "note": "the headline (`value`, seconds_per_proof) draws its blinding from `StdRng::seed_from_u64(0)`'s Fr::random stream (ChaCha12, "
                                                   "halo2-base/src/utils/testing.rs:38) generated on the device INSIDE the timed call (h2hip_chacha_rng_fill handed to create_proof: "
                                                   "csrc/rng.hip); host_generated = the same stream from libh2hip's one-thread host generator behind the RNG callback (1 proof); "
                                                   "predrawn_array = r03's set-up, randomness prepared before the call.  Stream layout [UPSTREAM-RECALL], block function pinned to RFC 8439"}, "seconds_per_proof_all_kernels_profiled": all_profiled_s, "cold_first_proof_seconds": cold_s, "keygen_seconds": keygen_s,
            "proof_verified_by_h2hip_plonk_verify_proof": True, "proof_repeatable": True,
            "stage_ms": {k_: round(v, 3) for k_, v in stages.items()}, "stage_ms_sum": round(sum(stages.values()), 3),
            "kernel_ms_per_proof": account, "gpu_busy_ms_per_proof": busy_all_ms,
            "kernel_account_note": "kernel_ms_per_proof / gpu_busy_ms_per_proof: %d further proofs with every launch bracketed by HIP events (not the timed region: the events of "
                                   "~200 launches add ~1 ms per proof); ms = sum of launch durations (launches of concurrent MSM lanes overlap), busy_ms = union of their spans" % acct_proofs,
            "roofline_int": {"bound": "integer multiplier (v_mad_u64_u32, 4 cycles per wave64)", "kernel": "msm_accum_kernel",
                             "achieved": 10.0 * msm_n * W19 / k_avg_s if k_avg_s > 0 else 0.0, "peak": modmul_peak, "unit": "modmul/s",
                             "frac": (10.0 * msm_n * W19 / k_avg_s / modmul_peak) if k_avg_s > 0 else 0.0,
                             "algorithmic_products_per_launch": 10.0 * msm_n * W19, "window_bits": c19, "windows": W19,
                             "peak_saturated_8x32": modmul_peak_sat, "silicon_issue_peak": 256 * 4 * 16 * 2.4e9 / 171.0,
                             "note": "peak = the chip's best 254-bit Montgomery multiplier known to us, measured in this run (h2hip_bench_modmul29: the unsaturated 9x29-limb form "
                                     "the kernel itself uses); algorithmic products = 10*n*W (XYZZ mixed addition 8M+2S per signed digit)"},
            "roofline_proof": {"algorithmic": work,
                               "int": {"achieved": work["products"] / seconds, "peak": modmul_peak, "unit": "modmul/s", "frac": work["products"] / seconds / modmul_peak,
                                       "ideal_ms": work["products"] / modmul_peak * 1e3},
                               "hbm": {"achieved": work["bytes"] / seconds / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": work["bytes"] / seconds / 8e12},
                               "note": "whole proof: (sum of the algorithmic products of its MSMs and transforms) / seconds_per_proof against the multiplier peak measured in "
                                       "this run; recompute from `algorithmic`, `seconds_per_proof` and `roofline_int.peak`"},
        })
        if not args.no_cpu_baseline:   # N > 1 as well: rank 0's host cores, the other ranks wait at the next barrier
            try:
                cb = cpu_baseline_create_proof(ctx, kzg, pk, circ, draws, proof, k, s_toxic)
                out["cpu_baseline"] = {"value": cells / cb["seconds"], "unit": "constraints/s", "cores": cb["cores"], "kind": "port", "sample": cb["sample"], **{
                    k_: v for k_, v in cb.items() if k_ not in ("cores", "kind", "sample")}}
                out["speedup_vs_cpu_port"] = cb["seconds"] / host_advice_s   # like for like: both take the witness from host memory
                out["speedup_vs_cpu_port_advice_resident_in_hbm"] = cb["seconds"] / seconds
            except Exception as e:
                out["cpu_baseline"] = {"error": repr(e)}
        if world > 1:
            sharded_exchanges = None
            if sharded:
                # the schedule of the last sharded proof as libh2hip ran it (h2hip_plonk_pk_last_exchanges), labelled in the order plonk.hip builds it
                cnt = _C.c_size_t(0)
                sizes = (_C.c_size_t * 32)()
                ctx._chk(ctx.lib.h2hip_plonk_pk_last_exchanges(pk.handle, sizes, 32, _C.byref(cnt)))
                ntt_cols = sk.shard_ntt_columns   # what shard_proving_key decided (by measurement when --shard-ntt-columns auto)
                what = ["hello (shape, point range, stages sharded, RNG digest)", "round 1: advice + permuted lookup columns",
                        "grand products: the row ranges' total products (and the go-ahead of their all-gather)",
                        ] + (["go-ahead before the all-gather of the first-round columns' coefficient forms (status only)"] if ntt_cols else []) + [
                        "round 2: grand products + random polynomial",
                        ] + (["go-ahead before the all-gather of the product columns' coefficient forms (status only)"] if ntt_cols else []) + [
                        "go-ahead before the coset all-gather (status only)", "h(X) pieces",
                        "evaluations: partial sums over the coefficient ranges", "SHPLONK: the ranges' partial evaluations at the rotation sets' points (carries)",
                        "SHPLONK W", "SHPLONK: the linearisation's partial evaluation at u (carry)", "SHPLONK W'"]
                nprod = sh.num_perm_sets + sh.num_lookups
                rows = -(-n // world)
                sharded_exchanges = {"host_allgather_payload_bytes_per_rank": [int(sizes[i]) for i in range(cnt.value)],
                                     "host_allgather_what": what if cnt.value == len(what) else "(%d exchanges: stages switched off)" % cnt.value,
                                     "device_allgathers_bytes_per_rank": {
                                         "grand product columns, this rank's rows (device to device)": 32 * nprod * (rows + 1),
                                         "h(X)'s numerator, this rank's cosets (device to device)": 32 * n * (-(-(1 << (sh.extended_k - k)) // world))},
                                     "status_word_bytes": 8}
            out["comm"] = {"transport": "RCCL (ncclAllGather on the context's stream; librccl dlopen'ed by libh2hip)" if comm_ranks[0]["is_rccl"] else
                                        "callback (torch.distributed %s all_gather on host tensors)" % args.dist_backend,
                           "ranks": comm_ranks, "distinct_gpus": len({r["gpu_uuid"] or r["pci_bus_id"] or r["cuda_device"] for r in comm_ranks}),
                           "sharded_proof_exchanges": None if not sharded else sharded_exchanges}
        out["reference_published"] = {"total_proof_time_s": 7.6, "source": "/root/reference/README.md:242 (32 vCPU r6a / M2 Max, end to end incl. witness generation; other hardware)"}
    if sk is not None:
        sk.free()
        # the other curve, in the same run: with the sharding taken off the key, every GPU proves on its own (N independent k = 19 proofs per step,
        # no exchange) — the weak-scaling aggregate next to the strong-scaling headline above.  The first of them is also the check that the SHARDED
        # proof of the timed region equals the UNSHARDED proof of the same key, witness and RNG stream byte for byte
        unsharded = prove()
        same = [None] * world
        dist.all_gather_object(same, unsharded == proof)
        if rank == 0:
            out["sharded_bytes_equal_unsharded"] = all(same)
        if not all(same):
            raise SystemExit("bench.py: the sharded proof differs from the unsharded proof of the same key on ranks %r" % [i for i, v in enumerate(same) if not v])
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            prove()
        torch.cuda.synchronize()
        dist.barrier()
        te = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        if rank == 0:
            rep_s = float(te.item()) / args.steps
            out["independent_proofs_per_gpu"] = {"what": "%d independent k=%d proofs per step, one per GPU, no exchange (weak scaling), same run" % (world, k),
                                                 "ms_per_step": rep_s * 1e3, "value": world * cells / rep_s, "unit": "constraints/s", "scaling": "weak"}
    pk.free()
    kzg.free()

    # ------------------------------------------------------------------ extra blocks (never part of the timed region above)
    if not args.no_replay:
        try:
            blk = msm_block(ctx, args, torch, dev, world, rank, dist, xdev, comm)
        except Exception as e:
            blk = {"error": repr(e)}
        if rank == 0:
            out["msm_2_%d" % args.log_n] = blk
    if world > 1 and not args.no_replay:
        # BASELINE configs[4] AS north_star STATES IT: the k = 21 BN254-pairing shape (bench_pairing.config:8: 2 gate + 1 lookup advice columns, 1 constants
        # column, lookup_bits 20) sharded over the N GPUs — every rank runs this block; the one-GPU proof of the same key is timed in the same run
        try:
            blk = create_proof_shape(ctx, 21, 2, 1, 1, 0, 20, reps=3, modmul_peak=modmul_peak if rank == 0 else None, golden=_golden_entry("pairing-21"),
                                     what="BASELINE configs[4]: the k=21 BN254-pairing configuration (halo2-ecc/configs/bn254/bench_pairing.config:8), 14 MSMs of 2^21, "
                                          "extended_k 23; `seconds` = one GPU (rank 0), `sharded` = the same proof over %d GPUs" % world,
                                     sharding={"comm": comm, "dist": dist, "torch": torch, "dev": dev, "xdev": xdev, "backend": args.dist_backend, "world": world, "rank": rank,
                                               "shard_ntt_columns": {"auto": None, "on": True, "off": False}[args.shard_ntt_columns]})
        except Exception as e:
            blk = {"error": repr(e)}
        if rank == 0:
            out["create_proof_k21_pairing_shape"] = blk
    if rank == 0 and world == 1 and not args.no_replay:
        for name, fn in (("ntt_2_22", lambda: ntt_config3(ctx, torch, dev, modmul_peak)),
                         ("k8_witness_batches", lambda: k8_batches(ctx, torch, dev, modmul_peak_sat, modmul_peak)),
                         ("witness_distribution", lambda: witness_distribution(ctx, args.k)),
                         ("create_proof_in_flight", lambda: create_proof_in_flight(ctx.device if hasattr(ctx, "device") else 0, args.k)),
                         ("create_proof_k21_pairing_shape", lambda: create_proof_shape(
                             ctx, 21, 2, 1, 1, 0, 20, reps=3, modmul_peak=modmul_peak, account_proofs=2, golden=_golden_entry("pairing-21"),
                             what="BASELINE configs[4] on ONE GPU: the k=21 BN254-pairing configuration "
                                  "(halo2-ecc/configs/bn254/bench_pairing.config:8), 14 MSMs of 2^21, extended_k 23"))):
            try:
                out[name] = fn()
            except Exception as e:   # never let an extra block break the contract line
                out[name] = {"error": repr(e)}
        if not args.no_sweep:
            try:
                out["create_proof_config_sweep"] = create_proof_config_sweep(ctx)
            except Exception as e:
                out["create_proof_config_sweep"] = {"error": repr(e)}
    if rank == 0:
        emit(out)
    if comm is not None:
        comm.destroy()
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


def msm_block(ctx, args, torch, dev, world, rank, dist, xdev, comm=None):
    """BASELINE configs[1]: 2^log_n-point G1 MSMs on resident scalars and bases (the other half of the metric: G1-adds/s), verified in-run against
    the closed form of known-dlog bases.  N > 1: point-range sharding — weak (every rank a 2^log_n slice of an N*2^log_n-point MSM) or strong."""
    from halo2_lib_amd.multi_gpu import sharded_msm, sharded_msm_batch

    steps, warmup = args.msm_steps, 8
    n_total = 1 << args.log_n
    n = n_total // world if args.scaling == "strong" else n_total   # points per rank
    # each rank owns its own slice of the (world * n)-point MSM: n DISTINCT known-dlog bases built on the GPU, and --batch
    # distinct uniformly random scalar columns (a prover round commits different columns; identical columns would share
    # cache lines between the concurrent lanes)
    K0, D = 0x1234567, 3
    pts_d = known_dlog_bases_gpu(ctx, torch, dev, n, K0, D, first_index=rank * n)
    bases = ctx.bases_from_device(pts_d.data_ptr(), n, 1 if args.precompute else 0)
    ncols = max(1, args.batch)
    scal_cols_h = [synthetic_scalars(n, seed=2000 + 97 * rank + j) for j in range(ncols)]
    scal_cols_d = [torch.from_numpy(c.view(np.int64)).to(dev) for c in scal_cols_h]
    scal_h, scal_d = scal_cols_h[0], scal_cols_d[0]
    torch.cuda.synchronize()
    last = {}

    def run_steps(cnt):
        """cnt MSMs over this rank's slice, issued in batches of --batch (pipelined over the context's lanes);
        N>1: one all-gather of the 96 B partials per batch through libh2hip's communicator + one host-side summation call."""
        done = 0
        res = None
        while done < cnt:
            b = min(args.batch, cnt - done)
            if b == 1:
                res = sharded_msm(ctx, bases, scal_d.data_ptr(), n, comm=comm)
            else:
                res = sharded_msm_batch(ctx, bases, [t.data_ptr() for t in scal_cols_d[:b]], n, comm=comm)
            last["cols"] = b
            done += b
        return res

    run_steps(warmup)
    ctx.profile_reset()
    ctx.profile_filter("msm_accum_kernel")   # the timed region brackets only the dominant kernel (its launch records its own events), like the headline
    ctx.profile_enable(True)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = run_steps(steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ctx.profile_enable(False)
    ctx.profile_filter("")
    if world > 1:
        te = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        elapsed = float(te.item())
    # ---- verify the LAST timed batch against the closed form (sum_i s_i * dlog_i) * G — no MSM implementation involved
    mine = [closed_form_dlog(scal_cols_h[j], K0, D, first_index=rank * n) for j in range(last["cols"])]
    if world > 1:
        allv = [None] * world
        dist.all_gather_object(allv, mine)
        mine = [sum(v[j] for v in allv) % R for j in range(last["cols"])]
    verified = all(jac_to_affine(result[j]) == _g1_mul(mine[j]) for j in range(last["cols"]))
    if not verified:
        raise RuntimeError("the timed MSM results do not match the closed form")
    blk = None
    if rank == 0:
        c, W = window_for(ctx, n)
        # G1 additions actually performed (SURVEY.md §8d's definition, specialised to the kernel's structure): one mixed addition per
        # (scalar, window) pair, plus the running-sum reduction of ONE bucket set with precomputed 2^(c*w) tables (all windows share
        # it) or of W bucket sets with plain bases
        adds_per_msm = n * W + 2 * (1 if args.precompute else W) * (1 << (c - 1))
        units = world * steps * adds_per_msm
        ms_per_msm = elapsed / steps * 1e3
        k_ms, k_cnt = ctx.profile_get("msm_accum_kernel")
        k_avg_s = (k_ms / max(k_cnt, 1)) * 1e-3
        k_busy_s = ctx.profile_get_busy("msm_accum_kernel") / max(k_cnt, 1) * 1e-3   # union of the launch spans / launches
        alg_bytes = 96.0 * n
        # the per-kernel breakdown: a further 16 MSMs with every launch bracketed (outside the timed region; one GPU only: with N > 1 the batches
        # hold collectives that rank 0 must not enter alone)
        breakdown = {"msm_accum_kernel": round(k_ms / steps, 4)}
        if world == 1:
            ctx.profile_reset()
            ctx.profile_enable(True)
            run_steps(16)
            ctx.profile_enable(False)
            breakdown = {name: round(v[0] / 16, 4) for name, v in ctx.profile_dump().items()}
            ctx.profile_reset()
        # single synchronous MSM (no pipelining): latency, and the dominant kernel's duration without overlap
        ctx.profile_reset()
        ctx.timer_start()
        for _ in range(4):
            ctx.msm_dev(bases, scal_d.data_ptr(), n)
        sync_ms = ctx.timer_stop() / 4
        ctx.profile_enable(True)
        for _ in range(3):
            ctx.msm_dev(bases, scal_d.data_ptr(), n)
        iso_ms, iso_cnt = ctx.profile_get("msm_accum_kernel")
        ctx.profile_enable(False)
        iso_avg_s = iso_ms / max(iso_cnt, 1) * 1e-3
        mm_ms, mm_n = ctx.bench_modmul(16384, 256, 2, unsaturated=True)
        modmul_peak = mm_n / (mm_ms * 1e-3)
        alg_modmul = 10.0 * n * W   # XYZZ mixed add = 8M + 2S per (scalar, window) pair
        blk = {"workload": "BASELINE configs[1]: 2^%d-point BN254 G1 MSM, uniform random scalars (distinct column per MSM of a batch), 2^%d distinct random-looking bases "
                           "(known-dlog multiples of G built on the GPU) resident in HBM, Jacobian result returned to the host" % (args.log_n, args.log_n),
               "value": units / elapsed, "unit": "G1-adds/s", "ms_per_msm": ms_per_msm, "steps": steps, "batch": args.batch, "pairs_per_sec": world * steps * n / elapsed,
               "points_per_gpu": n, "bases": "precomputed 2^(c*w) tables" if args.precompute else "plain", "window_bits": c, "windows": W, "adds_per_msm": adds_per_msm,
               "scaling": args.scaling if world > 1 else None,
               "result_verified": "last timed batch == (sum_i s_i*dlog_i)*G for every column (closed form, known-dlog bases)", "sync_ms_per_msm": sync_ms,
               "kernel_ms_per_msm": breakdown,
               "roofline": {"bound": "hbm", "kernel": "msm_accum_kernel", "achieved": alg_bytes / k_avg_s / 1e9 if k_avg_s > 0 else 0.0, "peak": 8000.0, "unit": "GB/s",
                            "frac": alg_bytes / k_avg_s / 8e12 if k_avg_s > 0 else 0.0, "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": k_avg_s * 1e3,
                            "launches": int(k_cnt), "avg_launch_ms_isolated": iso_avg_s * 1e3, "busy_ms_per_launch": k_busy_s * 1e3},
               "roofline_int": {"kernel": "msm_accum_kernel", "achieved": alg_modmul / k_avg_s if k_avg_s > 0 else 0.0, "peak": modmul_peak, "unit": "modmul/s",
                                "frac": (alg_modmul / k_avg_s / modmul_peak) if k_avg_s > 0 else 0.0,
                                "frac_whole_msm": alg_modmul / (ms_per_msm * 1e-3) / modmul_peak,
                                "frac_isolated": (alg_modmul / iso_avg_s / modmul_peak) if iso_avg_s > 0 else 0.0}}
        if world == 1 and not args.no_cpu_baseline:
            blk["cpu_baseline"] = cpu_baseline(ctx.bases_download(bases), scal_h, adds_per_msm)
    bases.free()
    return blk


def _fr_from_ints(vals):
    """canonical integers -> (n,4) u64 Montgomery limbs"""
    R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
    out = np.empty((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = (v << 256) % R_MOD
        out[i] = [(m >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
    return out


class _PreDrawnRng:
    """the prover's Fr::random stream as a pre-drawn array: the HIP prover (fill_into) and the oracle prover (fill / next_fr) consume the
    same values in the same order"""

    def __init__(self, values):
        self.values, self.pos = values, 0

    def fill(self, m):
        if self.pos + m > len(self.values):
            raise RuntimeError("pre-drawn RNG exhausted")
        out = self.values[self.pos:self.pos + m]
        self.pos += m
        return out

    def next_fr(self):
        row = [int(v) for v in self.fill(1)[0]]
        return (row[0] | row[1] << 64 | row[2] << 128 | row[3] << 192) * pow(1 << 256, -1, R) % R

    def fill_into(self, dst, m):
        import ctypes

        a = self.fill(m)
        ctypes.memmove(dst, a.ctypes.data, 32 * m)


class _ShapeView:
    """the attributes halo2_lib_amd.testing.build_circuit reads, from h2hip_plonk_shape_of"""

    def __init__(self, bp, sh):
        self.k, self.n, self.usable_rows, self.num_advice = bp.k, 1 << bp.k, sh.usable_rows, bp.num_advice
        self.lookup_bits = None if bp.lookup_bits < 0 else bp.lookup_bits
        self.gate_advice = list(range(bp.num_advice))
        self.lookup_advice = list(range(bp.num_advice, sh.num_advice_total))
        self.table_col = sh.table_col if sh.table_col >= 0 else None
        self.constant_cols = list(range(sh.first_constant_col, sh.first_constant_col + bp.num_fixed)) if bp.num_fixed else []
        self.q_lookup_col = sh.q_lookup_col if sh.q_lookup_col >= 0 else None
        self.q_enable_cols = list(range(sh.first_q_enable_col, sh.first_q_enable_col + bp.num_advice))
        self.num_fixed_total, self.num_instance = sh.num_fixed_total, bp.num_instance


def create_proof_k19(ctx, with_cpu_baseline: bool, reps: int = 10):
    """BASELINE.json configs[3]: a REAL create_proof (h2hip_plonk_create_proof: Blake2b transcript, 12 MSMs of 2^19, the lookup sort, grand
    products, h(X) over the 2^21 extended domain, evaluations, SHPLONK; proof bytes out) for the k = 19 secp256k1-ECDSA configuration
    (halo2-ecc/configs/secp256k1/bench_ecdsa.config:1: 1 advice column with the lookup behind q_lookup, 1 constants column, lookup_bits 18,
    no instances), as the reference times it at halo2-base/src/utils/testing.rs:233-238 minus the witness generation: the advice column is a
    synthetic circuit-like one (halo2_lib_amd/testing.py), handed over in host memory like the Vec the Rust prover holds.  `seconds` is host
    wall clock around the whole call, INCLUDING the host->device staging of the advice column and of the 2^19 + ~60 RNG-drawn scalars.
    The cpu_baseline leg runs the oracle's restatement of the same prover (identical step list, C kernels on the box's cores), compares
    the proof BYTES and verifies the HIP proof with the oracle verifier (real pairing)."""
    from halo2_lib_amd import halo2_proofs as HP
    from halo2_lib_amd import plonk as PL
    from halo2_lib_amd import testing as T

    k = 19
    s_toxic = 0x1D0C0FFEE1234567890ABCDEF
    kzg = HP.ParamsKZG.setup(ctx, k, s_toxic, precompute=True)
    bp = PL.BaseCircuitParams.new(k, 1, 1, 1, 0, 18)
    sh = PL.shape_of(ctx, bp)
    n = 1 << k

    class Backend:   # the synthetic witness is computed through the K8 batch kernels
        mul = staticmethod(ctx.fr_mul)
        add = staticmethod(ctx.fr_add)

    circ = T.build_circuit(_ShapeView(bp, sh), 19, Backend)
    t0 = time.perf_counter()
    pk = PL.keygen(kzg, bp, circ.fixed, circ.copies)
    keygen_s = time.perf_counter() - t0
    draws = synthetic_scalars(n + 4096, 4242)
    PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(draws))            # warm-up (allocates the key's buffer pool)
    ctx.sync()
    each = []
    t0 = time.perf_counter()
    for _ in range(reps):
        t1 = time.perf_counter()
        proof = PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(draws))   # returns after the proof bytes are on the host
        each.append(time.perf_counter() - t1)
    seconds = (time.perf_counter() - t0) / reps
    stages = {}
    PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(draws), stages)    # per-stage laps (adds a stream sync per stage)
    t0 = time.perf_counter()
    verified = PL.verify_proof(pk, circ.instances, proof)     # libh2hip's own verifier (host code): the reference's check_proof
    verify_s = time.perf_counter() - t0
    cells = 4 * (sh.usable_rows // 4)    # assigned advice cells: `constraints` of SURVEY.md §8d (total_advice of the circuit)
    out = {"what": "h2hip_plonk_create_proof, k=19 ECDSA configuration (bench_ecdsa.config:1), synthetic circuit-like witness; wall clock incl. "
                   "host staging of the advice column (16 MiB) and of the RNG-drawn scalars (16 MiB); witness generation (CPU gadgets) excluded",
           "seconds": seconds, "reps": reps, "proof_bytes": len(proof), "constraints": cells, "constraints_per_sec": cells / seconds,
           "msm_count": sh.num_commitments, "msm_size": n, "extended_k": sh.extended_k, "degree": sh.degree,
           "stage_ms": {k_: round(v, 3) for k_, v in stages.items()}, "stage_ms_sum": round(sum(stages.values()), 3), "keygen_seconds": keygen_s,
           "verified_by_h2hip_plonk_verify_proof": bool(verified), "verify_seconds": verify_s,
           "reference_published_total_proof_time_s": 7.6,
           "reference_source": "/root/reference/README.md:242 (32 vCPU r6a / M2 Max, end-to-end incl. witness generation; other hardware)"}
    if with_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_create_proof(ctx, kzg, pk, circ, draws, proof, k, s_toxic)
        out["speedup_vs_cpu_port"] = out["cpu_baseline"]["seconds"] / seconds
    pk.free()
    kzg.free()
    return out


def _golden_entry(name):
    """the committed oracle-prover digest of a reference shape (tests/golden/reference_shapes_proof_digests.json: written by the ORACLE prover alone,
    tests/golden/make_proof_goldens.py) with the generator's toxic scalar and seeds — plain data, nothing of oracle/ is imported or run here"""
    try:
        with open(os.path.join(ROOT, "tests", "golden", "reference_shapes_proof_digests.json")) as f:
            doc = json.load(f)
        return {"name": name, "toxic_s": int(doc["toxic_s"], 16), "circuit_seed": doc["circuit_seed"], "rng_seed": doc["rng_seed"], **doc["shapes"][name]}
    except Exception:
        return None


def _predrawn_stream(count, seed):
    """tests/util.py:rand_fr — the pre-drawn Fr::random stream the golden generator hands both provers"""
    a = np.random.default_rng(seed).integers(0, 2**63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + \
        np.random.default_rng(seed + 1).integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def create_proof_shape(ctx, k, na, nl, nf, ni, lb, reps, what, modmul_peak=None, account_proofs=0, sharding=None, golden=None):
    """create_proof for another BaseCircuitParams shape (no CPU leg): seconds per proof, stages, verified by libh2hip's verifier.
    modmul_peak: adds `roofline_proof` (the shape's algorithmic products / bytes over its wall time, SURVEY.md §8d's formulas);
    account_proofs: that many further proofs with every launch bracketed -> `kernel_ms_per_proof`;
    sharding = {"comm", "dist", "torch", "dev", "backend", "shard_ntt_columns", "world", "rank"}: ALL ranks call this together — the same key is put on
    the sharded path, ONE proof per step over the N GPUs is timed between barriers (max over ranks), the exchange schedule is read
    back, and the sharded bytes are compared with the unsharded proof of the same key and with every other rank's.
    golden = _golden_entry(name): the SRS, the synthetic circuit and the RNG stream are the golden generator's, so that sha256(proof) can be compared
    with the digest the oracle prover alone produced for this shape (`equals_committed_oracle_prover_digest`)."""
    from halo2_lib_amd import halo2_proofs as HP
    from halo2_lib_amd import plonk as PL
    from halo2_lib_amd import testing as T

    kzg = HP.ParamsKZG.setup(ctx, k, golden["toxic_s"] if golden else 0x1D0C0FFEE1234567890ABCDEF, precompute=True)
    bp = PL.BaseCircuitParams.new(k, na, nl, nf, ni, lb)
    sh = PL.shape_of(ctx, bp)

    class Backend:
        mul = staticmethod(ctx.fr_mul)
        add = staticmethod(ctx.fr_add)

    circ = T.build_circuit(_ShapeView(bp, sh), golden["circuit_seed"] + k if golden else k, Backend)
    pk = PL.keygen(kzg, bp, circ.fixed, circ.copies)
    if golden:   # tests/golden/make_proof_goldens.py:rng_budget — the stream's length does not change its prefix, the seed does
        bf = (1 << k) - sh.usable_rows - 1
        budget = sh.num_advice_total * (bf + 2) + sh.num_lookups * (2 * (bf + 1) + 2 + bf + 1) + sh.num_perm_sets * (bf + 1) + (1 << k) + 1 + (sh.degree - 1) + 16
        draws = _predrawn_stream(budget, golden["rng_seed"] + k)
    else:
        draws = synthetic_scalars((1 << k) + 65536, 4243)
    # r06: like the headline, the block times the call with the advice columns RESIDENT IN HBM (the bench contract: inputs on the device when the
    # timed region starts); the same call with the columns in host memory — at k = 21 three 64 MiB uploads, ~3.6 ms of PCIe — is `seconds_host_advice`
    adv_dev = [ctx.to_device(np.ascontiguousarray(c)) for c in circ.advice]
    PL.create_proof(pk, adv_dev, circ.instances, PL.ArrayRng(draws), advice_on_device=True)
    ctx.sync()
    each = []
    t0 = time.perf_counter()
    for _ in range(reps):
        t1 = time.perf_counter()
        proof = PL.create_proof(pk, adv_dev, circ.instances, PL.ArrayRng(draws), advice_on_device=True)   # returns after the proof bytes are on the host
        each.append(time.perf_counter() - t1)
    seconds = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        proof_host = PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(draws))
    seconds_host = (time.perf_counter() - t0) / reps
    if proof_host != proof:
        raise RuntimeError("create_proof_shape: host-resident and device-resident advice columns gave different proofs")
    stages = {}
    PL.create_proof(pk, adv_dev, circ.instances, PL.ArrayRng(draws), stages, advice_on_device=True)
    for d in adv_dev:
        ctx.free(d)
    ok = PL.verify_proof(pk, circ.instances, proof)
    cells = 4 * (sh.usable_rows // 4) * na
    out = {"what": what, "seconds": seconds, "seconds_median": sorted(each)[len(each) // 2], "seconds_min": min(each), "reps": reps, "seconds_host_advice": seconds_host,
           "seconds_is": "advice columns resident in HBM (as the headline); seconds_host_advice: the same call with the columns staged from host memory inside it",
           "proof_bytes": len(proof), "constraints": cells, "constraints_per_sec": cells / seconds,
           "msm_count": sh.num_commitments, "msm_size": 1 << k, "extended_k": sh.extended_k, "stage_ms": {k_: round(v, 3) for k_, v in stages.items()},
           "verified_by_h2hip_plonk_verify_proof": bool(ok)}
    if golden:
        import hashlib

        out["proof_sha256"] = hashlib.sha256(proof).hexdigest()
        out["golden"] = {"entry": "tests/golden/reference_shapes_proof_digests.json:" + golden["name"], "oracle_prover_proof_sha256": golden["proof_sha256"],
                         "verifying_keys_equal": hex(pk.transcript_repr) == golden["transcript_repr"]}
        out["equals_committed_oracle_prover_digest"] = out["proof_sha256"] == golden["proof_sha256"]
    if modmul_peak:
        work = proof_algorithmic_work(ctx, bp, sh)
        med = out["seconds_median"]
        out["roofline_proof"] = {"algorithmic": work,
                                 "int": {"achieved": work["products"] / med, "peak": modmul_peak, "unit": "modmul/s", "frac": work["products"] / med / modmul_peak,
                                         "ideal_ms": work["products"] / modmul_peak * 1e3},
                                 "hbm": {"achieved": work["bytes"] / med / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": work["bytes"] / med / 8e12},
                                 "note": "over seconds_median (advice columns resident in HBM); same formulas as the headline's roofline_proof"}
    if account_proofs:
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(account_proofs):
            PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(draws))
        ctx.profile_enable(False)
        out["kernel_ms_per_proof"] = kernel_account(ctx, account_proofs)
        out["gpu_busy_ms_per_proof"] = ctx.profile_get_busy("") / account_proofs
    if sharding is not None:
        import ctypes as _C
        import hashlib

        from halo2_lib_amd.multi_gpu import shard_proving_key

        dist, torch, world, rank = sharding["dist"], sharding["torch"], sharding["world"], sharding["rank"]
        sk = shard_proving_key(pk, ctx.bases_download(kzg.g), ctx.bases_download(kzg.g_lagrange), device=sharding["xdev"], precompute=True, comm=sharding["comm"],
                               shard_ntt_columns=sharding["shard_ntt_columns"])
        prove = lambda st=None: PL.create_proof(pk, circ.advice, circ.instances, PL.ArrayRng(draws), st)
        sproof = prove()
        steps = max(reps, 3)
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sproof = prove()
        torch.cuda.synchronize()
        dist.barrier()
        te = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=sharding["dev"] if sharding["backend"] == "nccl" else "cpu")
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        sstages = {}
        prove(sstages)
        cnt, sizes = _C.c_size_t(0), (_C.c_size_t * 32)()
        ctx._chk(ctx.lib.h2hip_plonk_pk_last_exchanges(pk.handle, sizes, 32, _C.byref(cnt)))
        digests = [None] * world
        dist.all_gather_object(digests, hashlib.sha256(sproof).hexdigest())
        nprod, rows = sh.num_perm_sets + sh.num_lookups, -(-(1 << k) // world)
        out["sharded"] = {"what": "the same key on the sharded path: ONE proof per step over %d GPUs (commitments by point range, 2^%d / %d points per GPU; cosets, row "
                                  "ranges, coefficient ranges: DESIGN.md §6), advice columns in host memory on every rank" % (world, k, world),
                          "seconds": float(te.item()) / steps, "steps": steps, "speedup_vs_one_gpu_same_run": seconds / (float(te.item()) / steps),
                          "stage_ms_rank0": {k_: round(v, 3) for k_, v in sstages.items()},
                          "sharded_bytes_equal_unsharded": sproof == proof, "ranks_emit_identical_bytes": len(set(digests)) == 1, "proof_sha256": digests[0],
                          "equals_committed_oracle_prover_digest": (digests[0] == golden["proof_sha256"]) if golden else None,
                          "lagrange_to_coeff_by_column": sk.shard_ntt_columns, "lagrange_to_coeff_by_column_decision": sk.ntt_decision,
                          "host_allgather_payload_bytes_per_rank": [int(sizes[i]) for i in range(cnt.value)],
                          "device_allgathers_bytes_per_rank": {"grand product columns, this rank's rows": 32 * nprod * (rows + 1),
                                                               "h(X)'s numerator, this rank's cosets": 32 * (1 << k) * (-(-(1 << (sh.extended_k - k)) // world))}}
        sk.free()
    pk.free()
    kzg.free()
    return out


def witness_distribution(ctx, k, reps: int = 5):
    """How much of the headline depends on the SYNTHETIC witness (VERDICT r04 missing 6): the advice commitment and the two permuted-lookup
    commitments skip zero digits, so their cost follows the column's cell statistics.  The k = 19 ECDSA shape is proved with the default column
    (halo2_lib_amd/testing.py), with a column of 0 / 1 / 2 cells only ("all_bits") and with full-width cells everywhere except the range-checked
    ones ("all_uniform"); a real halo2-ecc column (secp256k1/tests/ecdsa.rs:104-146: bits, lookup-sized and 88-bit CRT limbs, few full-width
    cells) lies between the first two.  Same key shape, same RNG stream, every proof verified."""
    from halo2_lib_amd import halo2_proofs as HP
    from halo2_lib_amd import plonk as PL
    from halo2_lib_amd import testing as T

    kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF, precompute=True)
    bp = PL.BaseCircuitParams.new(k, 1, 1, 1, 0, k - 1)
    sh = PL.shape_of(ctx, bp)

    class Backend:
        mul = staticmethod(ctx.fr_mul)
        add = staticmethod(ctx.fr_add)

    out = {}
    for name, kw in (("default", {}), ("all_bits", {"cell_mix": (0.5, 0.5, 0.0, 0.0), "range_checked_bits": 1}), ("all_uniform", {"cell_mix": (0.0, 0.0, 0.0, 1.0)})):
        circ = T.build_circuit(_ShapeView(bp, sh), 19, Backend, **kw)
        pk = PL.keygen(kzg, bp, circ.fixed, circ.copies)
        adv = [ctx.to_device(np.ascontiguousarray(c)) for c in circ.advice]
        prove = lambda: PL.create_proof(pk, adv, circ.instances, PL.ChaChaRng(ctx.lib, 0, 12), advice_on_device=True)
        prove()
        each = []
        for _ in range(reps):
            t0 = time.perf_counter()
            proof = prove()
            each.append(time.perf_counter() - t0)
        out[name] = {"ms_per_proof_median": sorted(each)[len(each) // 2] * 1e3, "ms_per_proof_min": min(each) * 1e3,
                     "verified": bool(PL.verify_proof(pk, circ.instances, proof)),
                     "cells": {k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in T.cell_statistics(circ.advice[0], sh.usable_rows, k - 1).items()}}
        for d in adv:
            ctx.free(d)
        pk.free()
    kzg.free()
    out["what"] = ("k=%d ECDSA shape, advice resident in HBM, %d proofs each: the headline's dependence on the synthetic column's statistics, bracketed "
                   "(cells: fractions of the advice column that are 0, 1, below 2^lookup_bits, below 2^88, wider)" % (k, reps))
    return out


def create_proof_in_flight(device, k, threads: int = 3, proofs: int = 10):
    """THROUGHPUT with several proofs in flight (tools/two_in_flight.py): `threads` host threads, each with its own libh2hip context, window tables and
    proving key of the k = 19 ECDSA shape, call create_proof in a loop at the same time (ctypes releases the GIL inside the call).  ms per proof =
    wall / proofs, for 1 .. threads threads; every proof must have the same bytes.  NOT the headline (that is one proof at a time, as the reference
    times it): the figure says how much of the chip a single proof's Fiat-Shamir chain leaves unused — DESIGN.md §3a."""
    import hashlib
    import threading

    import halo2_lib_amd as H
    from halo2_lib_amd import halo2_proofs as HP
    from halo2_lib_amd import plonk as PL
    from halo2_lib_amd import testing as T

    class Prover:
        def __init__(self):
            self.ctx = ctx = H.Context(device)
            self.kzg = HP.ParamsKZG.setup(ctx, k, 0x1D0C0FFEE1234567890ABCDEF, precompute=True)
            bp = PL.BaseCircuitParams.new(k, 1, 1, 1, 0, k - 1)
            sh = PL.shape_of(ctx, bp)

            class Backend:
                mul = staticmethod(ctx.fr_mul)
                add = staticmethod(ctx.fr_add)

            self.circ = T.build_circuit(_ShapeView(bp, sh), 5, Backend)
            self.pk = PL.keygen(self.kzg, bp, self.circ.fixed, self.circ.copies)
            self.adv = [ctx.to_device(np.ascontiguousarray(c)) for c in self.circ.advice]
            self.digests = set()

        def prove(self):
            p = PL.create_proof(self.pk, self.adv, self.circ.instances, PL.ChaChaRng(self.ctx.lib, 0, 12), advice_on_device=True)
            self.digests.add(hashlib.sha256(bytes(p)).hexdigest())

        def close(self):
            for d in self.adv:
                self.ctx.free(d)
            self.pk.free()
            self.kzg.free()
            self.ctx.close()

    provers = []
    try:
        for _ in range(threads):
            provers.append(Prover())
        for p in provers:
            p.prove()
            p.prove()

        def run(nt):
            gate = threading.Barrier(nt + 1)

            def work(p):
                gate.wait()
                for _ in range(proofs):
                    p.prove()

            ths = [threading.Thread(target=work, args=(provers[i],)) for i in range(nt)]
            for t in ths:
                t.start()
            gate.wait()
            t0 = time.perf_counter()
            for t in ths:
                t.join()
            return (time.perf_counter() - t0) * 1e3 / (nt * proofs)

        per = {}
        for nt in range(1, threads + 1):
            per[str(nt)] = min(run(nt) for _ in range(2))
        digests = set().union(*[p.digests for p in provers])
        return {"what": "k=%d ECDSA shape, advice resident in HBM, %d proofs per thread, best of 2 rounds: ms per proof (wall / proofs) with 1 .. %d proofs in "
                        "flight, one host thread + context + tables + key each" % (k, proofs, threads),
                "ms_per_proof_by_proofs_in_flight": per, "all_proofs_byte_identical": len(digests) == 1,
                "throughput_gain_over_one_at_a_time": per["1"] / min(per.values())}
    finally:
        for p in provers:
            p.close()


# the reference's two benchmark sweeps: (degree, num_advice, num_lookup_advice, num_fixed, lookup_bits) of every line of
# halo2-ecc/configs/bn254/bench_pairing.config and halo2-ecc/configs/secp256k1/bench_ecdsa.config
PAIRING_SHAPES = [(14, 211, 27, 1, 13), (15, 105, 14, 1, 14), (16, 50, 6, 1, 15), (17, 25, 3, 1, 16), (18, 13, 2, 1, 17), (19, 6, 1, 1, 18),
                  (20, 3, 1, 1, 19), (21, 2, 1, 1, 20), (22, 1, 1, 1, 21)]
ECDSA_SHAPES = [(19, 1, 1, 1, 18), (18, 2, 1, 1, 17), (17, 4, 1, 1, 16), (16, 8, 2, 1, 15), (15, 17, 3, 1, 14), (14, 34, 6, 1, 13),
                (13, 68, 12, 1, 12), (12, 139, 24, 2, 11), (11, 291, 53, 4, 10)]


def create_proof_config_sweep(ctx, reps: int = 5):
    """create_proof over synthetic halo2-base circuits of all 18 shapes the reference benchmarks (the same cell budget laid out from 1 column of
    2^22 rows to 291 + 53 columns of 2^11): ms per proof (median of `reps` individually timed proofs: the small shapes are partly host-bound and
    a shared box's CPU noise shows in a mean of three), each proof checked by libh2hip's verifier"""
    out = {}
    for name, shapes in (("bench_ecdsa.config", ECDSA_SHAPES), ("bench_pairing.config", PAIRING_SHAPES)):
        rows = []
        for k, na, nl, nf, lb in shapes:
            try:
                r = create_proof_shape(ctx, k, na, nl, nf, 0, lb, reps, "")
                rows.append({"k": k, "num_advice": na, "num_lookup_advice": nl, "num_fixed": nf, "lookup_bits": lb, "ms": round(r["seconds_median"] * 1e3, 2), "ms_mean": round(r["seconds"] * 1e3, 2),
                             "proof_bytes": r["proof_bytes"], "verified": r["verified_by_h2hip_plonk_verify_proof"]})
            except Exception as e:
                rows.append({"k": k, "num_advice": na, "error": repr(e)})
        out[name] = rows
    return out


def _cpu_threads():
    hw = os.cpu_count() or 1
    cores = min(hw, len(os.sched_getaffinity(0)))
    note = ""
    try:   # the GPU box's container may have a CPU quota far below its hardware threads (cgroup v2 cpu.max)
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            cores = max(1, min(cores, int(round(int(q) / int(period)))))
            note = "; cgroup cpu.max = %s/%s -> %d of the host's %d hardware threads usable" % (q, period, cores, hw)
    except Exception:
        pass
    return cores, note


def cpu_baseline_create_proof(ctx, kzg, pk, circ, draws, gpu_proof, k, s_toxic):
    """the oracle's create_proof (oracle/plonk.py over oracle/h2_oracle.c: same step list as the HIP prover) on the box's host cores"""
    from oracle import bn254 as O
    from oracle import plonk as P

    cores, note = _cpu_threads()
    threads = min(2 * cores, 64)
    sh = P.Shape(k, 1, 1, 1, 0, k - 1)
    params = P.Params.setup(k, s_toxic, g=ctx.bases_download(kzg.g), g_lagrange=ctx.bases_download(kzg.g_lagrange))
    asm = P.PermutationAssembly(sh)
    for l, r in circ.copies:
        asm.copy(l, r)
    opk = P.keygen(params, sh, circ.fixed, asm, threads)
    vk_equal = opk.vk.transcript_repr == pk.transcript_repr
    stages = {}
    t0 = time.perf_counter()
    want = P.create_proof(params, opk, circ.advice, [], _PreDrawnRng(draws), threads, stages)
    sec = time.perf_counter() - t0
    return {"seconds": sec, "cores": cores, "threads": threads, "kind": "port",
            "sample": "one full k=19 create_proof by the oracle restatement (C kernels: best_multiexp with ceil(ln n)-bit windows, radix-2 best_fft, "
                      "sort-based permute_expression_pair, ...) on %d threads%s" % (threads, note),
            "stage_s": {k_: round(v, 3) for k_, v in stages.items()},
            "verifying_keys_equal": bool(vk_equal), "proof_bytes_equal_to_gpu": want == gpu_proof,
            "gpu_proof_verified_by_oracle": bool(P.verify_proof(params, opk.vk, [], gpu_proof))}


def ntt_config3(ctx, torch, dev, modmul_peak):
    """BASELINE configs[2]: 2^22-length NTT + iNTT over F_r on resident data (extra field; the headline stays the MSM)."""
    from halo2_lib_amd import halo2_proofs as HP

    log_n = 22
    n = 1 << log_n
    dom = HP.EvaluationDomain(ctx, 2, log_n)
    a = torch.from_numpy(synthetic_scalars(n, 77).view(np.int64)).to(dev)
    ref = a.clone()
    ctx.best_fft_dev(a.data_ptr(), dom.omega, log_n)
    ctx.ifft_dev(a.data_ptr(), dom.omega_inv, log_n, dom.ifft_divisor)
    torch.cuda.synchronize()
    roundtrip_ok = bool(torch.equal(a, ref))
    reps = 10

    def timed(fn, rounds=3):   # the block follows host-side setup (the clocks have dropped): 2 * reps untimed, then the best of `rounds` loops of `reps`
        for _ in range(2 * reps):
            fn()
        best = []
        for _ in range(rounds):
            ctx.timer_start()   # (timed WITHOUT the per-launch event brackets: r04 timed this loop with them and reported 0.63-0.65 ms for a 0.58 ms transform)
            for _ in range(reps):
                fn()
            best.append(ctx.timer_stop() / reps)
        return min(best), sorted(best)[len(best) // 2]

    fwd_ms, fwd_med = timed(lambda: ctx.best_fft_dev(a.data_ptr(), dom.omega, log_n))
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(reps):
        ctx.best_fft_dev(a.data_ptr(), dom.omega, log_n)
    k_ms, k_cnt = ctx.profile_get("ntt_pass_kernel")
    ctx.profile_enable(False)
    inv_ms, inv_med = timed(lambda: ctx.ifft_dev(a.data_ptr(), dom.omega_inv, log_n, dom.ifft_divisor))
    alg_bytes = 64.0 * n
    alg_mul = (n / 2) * log_n
    # the transforms create_proof actually runs at k = 19: lagrange_to_coeff (iNTT 2^19), coeff_to_extended (coset NTT 2^19 -> 2^21),
    # extended_to_coeff (coset iNTT 2^21)
    d19, d21 = HP.EvaluationDomain(ctx, 5, 19), None
    src = torch.from_numpy(synthetic_scalars(1 << 19, 78).view(np.int64)).to(dev)
    ext = torch.empty((1 << 21) * 4, dtype=torch.int64, device=dev)
    work = {}
    for name, fn in (("intt_2_19", lambda: ctx.ifft_dev(src.data_ptr(), d19.omega_inv, 19, d19.ifft_divisor)),
                     ("coset_ntt_2_19_to_2_21", lambda: ctx.coeff_to_extended_dev(src.data_ptr(), 19, ext.data_ptr(), 21, d19.extended_omega, d19.g_coset)),
                     ("coset_intt_2_21", lambda: ctx.extended_to_coeff_dev(ext.data_ptr(), 21, d19.extended_omega_inv, d19.extended_ifft_divisor, d19.g_coset_inv))):
        ms, _ = timed(fn, rounds=2)
        out_n, lg = (1 << 19, 19) if name == "intt_2_19" else (1 << 21, 21)
        in_n = 1 << 19 if name != "coset_intt_2_21" else 1 << 21
        work[name] = {"ms": ms, "hbm_frac": 32.0 * (in_n + out_n) / (ms * 1e-3) / 8e12, "int_frac": (out_n / 2) * lg / (ms * 1e-3) / modmul_peak}
    return {"workload": "BASELINE configs[2]: 2^22-length radix-2 NTT and iNTT over F_r, data resident in HBM", "ntt_ms": fwd_ms, "intt_ms": inv_ms,
            "ntt_ms_median": fwd_med, "intt_ms_median": inv_med, "timing": "per transform: best (and median) of 3 loops of 10 after 20 untimed",
            "k19_workhorses": work,
            "roundtrip_bit_exact": roundtrip_ok, "passes": int(k_cnt // reps), "avg_pass_kernel_ms": k_ms / max(k_cnt, 1),
            "roofline": {"bound": "hbm", "kernel": "ntt_pass_kernel (3 launches per transform)", "achieved": alg_bytes / (fwd_ms * 1e-3) / 1e9, "peak": 8000.0,
                         "unit": "GB/s", "frac": alg_bytes / (fwd_ms * 1e-3) / 8e12, "algorithmic_bytes_per_transform": alg_bytes},
            "roofline_int": {"achieved": alg_mul / (fwd_ms * 1e-3), "peak": modmul_peak, "unit": "modmul/s", "frac": alg_mul / (fwd_ms * 1e-3) / modmul_peak,
                             "note": "algorithmic products = (n/2)*log2(n)"}}


def k8_batches(ctx, torch, dev, modmul_peak_sat, modmul_peak):
    """north_star's K8: witness-column Montgomery multiplications and Poseidon permutation batches through the same
    kernel layer (halo2-base GateInstructions::mul, PoseidonState::permutation).  Synthetic operands and synthetic round
    constants (the timing does not depend on their values; parity against the reference's KATs is in the tests)."""
    n = 1 << 22
    a = torch.from_numpy(synthetic_scalars(n, 31).view(np.int64)).to(dev)
    b = torch.from_numpy(synthetic_scalars(n, 32).view(np.int64)).to(dev)
    o = torch.empty_like(a)
    mul = lambda: ctx._chk(ctx.lib.h2hip_fr_mul_batch_dev(ctx.handle, o.data_ptr(), a.data_ptr(), b.data_ptr(), n))
    mul()
    ctx.timer_start()
    for _ in range(10):
        mul()
    mul_ms = ctx.timer_stop() / 10
    t, r_f, r_p, m = 3, 8, 57, 1 << 18          # the reference's t = 3, rate 2 spec shape (hasher/tests/state.rs)
    ctx.poseidon_set_spec(t, r_f, r_p, synthetic_scalars((r_f + r_p) * t, 33), synthetic_scalars(t * t, 34))
    st = torch.from_numpy(synthetic_scalars(m * t, 35).view(np.int64)).to(dev)
    inp = torch.from_numpy(synthetic_scalars(m * 2, 36).view(np.int64)).to(dev)
    perm = lambda: ctx._chk(ctx.lib.h2hip_poseidon_permute_batch_dev(ctx.handle, st.data_ptr(), inp.data_ptr(), 2, m))
    perm()
    ctx.timer_start()
    for _ in range(5):
        perm()
    pos_ms = ctx.timer_stop() / 5
    # multiplications of one permutation: full rounds t S-boxes (3 mul each) + t*t MDS; partial rounds 1 S-box + t*t MDS (dense form)
    muls = r_f * (3 * t + t * t) + r_p * (3 + t * t)
    return {"fr_mul_batch": {"elements": n, "ms": mul_ms, "GB_per_s": 96.0 * n / (mul_ms * 1e-3) / 1e9, "hbm_frac": 96.0 * n / (mul_ms * 1e-3) / 8e12,
                             "modmul_per_s": n / (mul_ms * 1e-3)},
            "poseidon_t3_batch": {"permutations": m, "ms": pos_ms, "permutations_per_s": m / (pos_ms * 1e-3),
                                  "algorithmic_modmul_per_s": muls * m / (pos_ms * 1e-3),
                                  "frac_of_unsaturated_multiplier_peak": muls * m / (pos_ms * 1e-3) / modmul_peak,
                                  "frac_of_saturated_multiplier_peak": muls * m / (pos_ms * 1e-3) / modmul_peak_sat,
                                  "note": "algorithmic products = t S-box products x3 + t^2 MDS products per full round, 3 + t^2 per partial round; the kernel "
                                          "reduces an MDS row once (one Montgomery reduction per t products), hence > 1 against the per-product peaks"}}


def cpu_baseline(bases_h, scal_h, adds_per_msm):
    """oracle/ restatement of upstream best_multiexp (thread-chunked multiexp_serial), all host cores."""
    from oracle import c_oracle as CO

    cores, quota_note = _cpu_threads()
    threads = 2 * cores   # measured best on the box (tools/cpu_scaling.py): 32 threads on the 16-CPU quota
    try:
        lib = CO.lib(native=True)
    except Exception:
        lib = CO.lib()
    n = len(scal_h)
    CO.best_multiexp(scal_h[:4096], bases_h[:4096], threads=threads, l=lib)   # warm up
    reps, t_total = 0, 0.0
    while t_total < 5.0 and reps < 20:
        t0 = time.perf_counter()
        CO.best_multiexp(scal_h, bases_h, threads=threads, l=lib)
        t_total += time.perf_counter() - t0
        reps += 1
    per = t_total / reps
    return {"value": adds_per_msm / per, "unit": "G1-adds/s", "cores": cores, "kind": "port", "threads": threads,
            "sample": "full 2^%d-point MSM x %d reps (%.3f s each), C restatement of best_multiexp (chunk = n/threads, c = ceil(ln chunk)) on %d "
                      "threads%s; value uses the SAME adds-per-MSM constant as the GPU line so the ratio equals the pairs/s ratio"
                      % (int(np.log2(n)), reps, per, threads, quota_note),
            "pairs_per_sec": n / per, "seconds_per_msm": per}


if __name__ == "__main__":
    main()
