"""Host logic: the LDS maps of the fused FFN's two-stage weight ring (layout_dm_amd/csrc/ldm_stream_sched.h FfnRingLinear /
FfnRingInterleaved) replayed byte by byte on the CPU — DMA destinations against fragment reads, stage disjointness, the
16-bit immediates, and the interleaved map as a bijection of the linear one (tests/cpu_ffn_ring_check.cpp; no GPU, no HIP)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ffn_ring_maps(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "cpu_ffn_ring_check.cpp")
    exe = tmp_path / "cpu_ffn_ring_check"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0 and "sanitize" in r.stderr:
        r = subprocess.run([cxx, "-O1", "-std=c++17", src, "-o", str(exe)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK:" in out.stdout, out.stdout + out.stderr
