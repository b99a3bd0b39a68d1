"""Host logic: the LDS-image weight packers (layout_dm_amd/csrc/ldm_pack.h) against the fused kernels' LDS read
formulas, compiled and run on the CPU (no GPU, no HIP)."""
import pytest

import _hostbuild as HB


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_weight_images_match_kernel_read_formulas(sanitize):
    """sanitize=True is the ASan/UBSan build of the pure-host part of the C-ABI layer: the packers
    index four differently padded arrays with three index maps each; an out-of-bounds write aborts the test."""
    out = HB.run_host(HB.host_program("cpu_pack_check", sanitize=sanitize), timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
