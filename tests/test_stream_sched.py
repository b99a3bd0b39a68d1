"""Host logic: the lgkmcnt bookkeeping of the fused kernels' continuous LDS-read / MFMA pipelines
(layout_dm_amd/csrc/ldm_stream_sched.h) against an independent replay of the issue order with an in-order LDS queue,
compiled (ASan + UBSan build) and run on the CPU (no GPU, no HIP)."""
import _hostbuild as HB


def test_head_stream_counted_waits():
    out = HB.run_host(HB.host_program("cpu_sched_check", sanitize=True), timeout=120)
    assert out.returncode == 0 and "OK:" in out.stdout, out.stdout + out.stderr
