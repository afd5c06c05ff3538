"""CPU-only: bench.py --dump-outputs writes what the timed path returned as DIR/<name>.npy in float32, exactly, and never more than 64 MB."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_proof_bytes_round_trip_exactly(tmp_path):
    proof = bytes(range(256)) * 5 + b"\x00\xff"
    d = tmp_path / "new" / "dir"
    bench.dump_outputs(str(d), {"proof": np.frombuffer(proof, dtype=np.uint8)})
    got = np.load(d / "proof.npy")
    assert got.dtype == np.float32 and got.shape == (len(proof),)
    assert bytes(got.astype(np.uint8)) == proof and np.array_equal(got, np.frombuffer(proof, dtype=np.uint8))


def test_refuses_more_than_64_mb(tmp_path):
    with pytest.raises(ValueError, match="limit"):
        bench.dump_outputs(str(tmp_path), {"a": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, dtype=np.uint8)})
    assert not os.listdir(tmp_path)


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, r.stderr
