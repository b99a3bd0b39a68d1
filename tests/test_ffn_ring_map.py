"""Host logic: the LDS maps of the fused FFN's two-stage weight ring (layout_dm_amd/csrc/ldm_stream_sched.h FfnRingLinear /
FfnRingInterleaved) replayed byte by byte on the CPU — DMA destinations against fragment reads, stage disjointness, the
16-bit immediates, and the interleaved map as a bijection of the linear one (tests/cpu_ffn_ring_check.cpp, ASan + UBSan build;
no GPU, no HIP)."""
import _hostbuild as HB


def test_ffn_ring_maps():
    out = HB.run_host(HB.host_program("cpu_ffn_ring_check", sanitize=True), timeout=120)
    assert out.returncode == 0 and "OK:" in out.stdout, out.stdout + out.stderr
