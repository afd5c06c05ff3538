"""A caller-owned transcript through the C++ host mirror: halo2-lib_amd/host/transcript_selftest.cpp implements a Blake2b transcript natively
behind the callbacks (it keeps the absorbed bytes and calls h2hip_blake2b on every squeeze) and proves selftest.cpp's small circuit.  Over the
emulated kernels on CPU, over the real libh2hip.so on the GPU; its proof must be selftest's, byte for byte."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "halo2-lib_amd", "host")


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_native_transcript_over_emulated_kernels(tmp_path):
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu

    lib = build_emu.build()
    exes = {}
    for name in ("transcript_selftest", "selftest"):
        exes[name] = str(tmp_path / (name + "_emu"))
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exes[name], os.path.join(HOST, name + ".cpp"), "-L" + os.path.dirname(lib),
                               "-lh2hip_emu", "-Wl,-rpath," + os.path.dirname(lib), "-lpthread"])
    assert "transcript selftest OK" in _run(exes["transcript_selftest"], "7")
    got = _run(exes["transcript_selftest"], "7", "--dump-proof").strip()
    assert len(got) > 64 and got == _run(exes["selftest"], "7", "--dump-proof").strip()


@pytest.mark.gpu
def test_native_transcript_on_gpu():
    exes = [os.path.join(HOST, "transcript_selftest"), os.path.join(HOST, "selftest")]
    if not all(os.path.exists(e) for e in exes):   # normally prebuilt by __graft_entry__.build()
        import __graft_entry__ as g

        g.build()
    assert "transcript selftest OK" in _run(exes[0], "11")
    got = _run(exes[0], "11", "--dump-proof").strip()
    assert len(got) > 64 and got == _run(exes[1], "11", "--dump-proof").strip()
