"""Static checks (no GPU: hipcc cross-compiles) on the gfx950 code of the stack kernel after the step-0 shortcut and
the removal of the FFN stream's wrap-around prefetch:

* every instantiation of stack_stream_k still lives inside the register file: no scratch, no VGPR spill, and the
  register counts hipcc reported before the change (the report tools/kernel_resources.py prints);
* the odd last iteration of the FFN chunk stream (the basic block with exactly 59 MFMAs: 29 GEMM1 + 30 GEMM2) issues
  no LDS-DMA any more — its "next chunk" was chunk 0 again, 64 KiB per layer into a ring stage nobody reads;
* the double iteration (the 118-MFMA block) still issues its 2 x 16 pieces.
"""
import re

import pytest

import _hostbuild as HB

SYM = "_ZN3ldm14stack_stream_kILb{tm}ELi{head}ELb{rel}EEEvNS_9StackArgsE"
# (VGPRs, AGPRs) per instantiation <TM, HEAD, REL>, as reported for the tree before the change
PARENT_REGS = {(0, 1, 0): (256, 245), (0, 2, 0): (256, 251), (0, 2, 1): (256, 250)}


@pytest.fixture(scope="module")
def compiled():
    asm, report, _ = HB.kernel_asm("kernels_stack.hip", resource_report=True)
    return asm, report


def _resources(report):
    """mangled kernel name -> {vgpr, agpr, scratch, vspill} (the fields of tools/kernel_resources.py)"""
    out, cur = {}, None
    for line in report.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("vspill", r"VGPRs? Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def _blocks(asm, symbol):
    """The kernel's basic blocks as lists of instructions (tests/test_loop_kernel_static.py reads them the same way)."""
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], []
    for l in lines[start + 1:end]:
        if re.match(r"^\.LBB\d+_\d+:", l):
            blocks.append(cur)
            cur = []
            continue
        t = l.strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        cur.append(t.split(";")[0].strip())
    blocks.append(cur)
    return blocks


@pytest.mark.parametrize("inst", sorted(PARENT_REGS))
def test_no_scratch_and_the_register_counts_of_the_parent(compiled, inst):
    res = _resources(compiled[1])[SYM.format(tm=inst[0], head=inst[1], rel=inst[2])]
    print(inst, res)
    assert res["scratch"] == 0 and res["vspill"] == 0, res
    assert (res["vgpr"], res["agpr"]) == PARENT_REGS[inst], res
    assert res["vgpr"] <= 256 and res["agpr"] <= 256


@pytest.mark.parametrize("head", [1, 2])
def test_odd_last_ffn_iteration_issues_no_dma(compiled, head):
    blocks = _blocks(compiled[0], SYM.format(tm=0, head=head, rel=0))
    n_mfma = [sum(t.startswith("v_mfma") for t in b) for b in blocks]
    odd = [b for b, n in zip(blocks, n_mfma) if n == 59]
    double = [b for b, n in zip(blocks, n_mfma) if n == 118]
    assert len(odd) == 1 and len(double) == 1, sorted(n for n in n_mfma if n)
    assert sum(t.startswith("global_load_lds") for t in odd[0]) == 0
    assert sum(t.startswith("global_load_lds") for t in double[0]) == 2 * 16
