"""Static checks on the gfx950 code of the stack kernel's FFN chunk loop and of the work around it that the loop kernel
repeats per reverse step (no GPU needed: hipcc cross-compiles).

The FFN ring of the stack kernel uses the interleaved LDS map (ldm_stream_sched.h FfnRingInterleaved): both ring stages
are within the ds_read offset field of one per-lane address, the chunk loop runs two iterations per trip with the stage
as a compile-time argument, and the GEMM2 operand fragments swap roles between the halves instead of being copied.  On
the assembly of the one-pass kernel (HEAD 1) and of the loop kernel (HEAD 2):

* the loop body holds 118 MFMAs (2 x (29 GEMM1 + 30 GEMM2));
* between its first and last MFMA there is no v_xor_b32 (the stage toggle of the linear map: 10 per chunk) and no
  v_mov_b32 (the fragment copy: 8 per chunk), and at most 2 x 33 + 2 other VALU instructions (per chunk: 16 adds, 8 casts,
  8 packed max of the bias / ReLU / cast, one bias address);
* its LDS reads carry the stage in the immediate: offsets of both stages appear on the same address registers;
* no block of v_accvgpr_mov_b32 follows the row gather in front of the first layer (hipcc used to define the residual
  accumulators element-wise in one AGPR range and move all 232 of them into the range the layers use);
* the dynamic VALU count per wavefront and reverse step (tools/instruction_mix.py) is at least 4 800 below the 52 700
  of the tree before the change (profiles/r04_instruction_mix_fast_loop.txt).
"""
import collections
import os
import re
import sys

import pytest

import _hostbuild as HB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = {"HEAD1": "_ZN3ldm14stack_stream_kILb0ELi1ELb0EEEvNS_9StackArgsE",
           "HEAD2": "_ZN3ldm14stack_stream_kILb0ELi2ELb0EEEvNS_9StackArgsE"}
PARENT_VALU_PER_STEP = 52700


@pytest.fixture(scope="module")
def asm_path():
    return HB.kernel_asm("kernels_stack.hip")[2]   # (the compile test_kernel_asm_lint.py reads, too)


def _instructions(asm_path, symbol):
    """The kernel's instructions in text order, and the index ranges of its basic blocks."""
    lines = open(asm_path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    ins, blocks = [], [0]
    for l in lines[start + 1:end]:
        if re.match(r"^\.LBB\d+_\d+:", l):
            blocks.append(len(ins))
            continue
        t = l.strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        ins.append(t.split(";")[0].strip())
    blocks.append(len(ins))
    return ins, list(zip(blocks, blocks[1:]))


def _ffn_loop_body(ins, blocks):
    bodies = [ins[a:b] for a, b in blocks if sum(t.startswith("v_mfma") for t in ins[a:b]) == 118]
    assert len(bodies) == 1, "no basic block with 118 MFMAs: the FFN chunk loop does not run two iterations per trip"
    body = bodies[0]
    mf = [i for i, t in enumerate(body) if t.startswith("v_mfma")]
    return body[mf[0]:mf[-1] + 1]


@pytest.mark.parametrize("head", ["HEAD1", "HEAD2"])
def test_ffn_loop_double_iteration_without_bookkeeping(asm_path, head):
    ins, blocks = _instructions(asm_path, KERNELS[head])
    body = _ffn_loop_body(ins, blocks)
    valu = collections.Counter(t.split()[0] for t in body if t.startswith("v_") and not t.startswith("v_mfma"))
    print(head, dict(valu))
    assert not [op for op in valu if op.startswith("v_xor_b32")], valu
    assert not [op for op in valu if op.startswith("v_mov_b32")], valu
    assert sum(valu.values()) <= 2 * 33 + 2, valu
    # the stage is in the immediate: every fragment address register is read at offsets of BOTH stages (W1: stage 1 at
    # 0x8000 + row group, W2: 0x8000 + tile), and no offset leaves the 16-bit field
    by_reg = collections.defaultdict(set)
    for t in body:
        m = re.match(r"ds_read_b128 \S+ (v\d+)(?: offset:(\S+))?", t)
        if m:
            by_reg[m.group(1)].add(int(m.group(2) or "0", 0))
    frag = {r: o for r, o in by_reg.items() if max(o) >= 0x8000}
    assert len(frag) == 10, by_reg  # 8 W1 columns + 2 W2 k16-steps (the eleventh register is the bias address)
    for r, offs in frag.items():
        assert max(offs) < 65536 and {o & 0x8000 for o in offs} == {0, 0x8000}, (r, sorted(offs))
        # within a stage: W1 row groups of 256 bytes, W2 tiles of 2 KiB (the first and last reads of the block lie outside
        # the span between its first and last MFMA, so not every offset shows up for both stages)
        low = {o & 0x7fff for o in offs}
        assert low <= {0, 256, 512, 768} or low <= {2048 * t for t in range(15)}, (r, sorted(offs))


@pytest.mark.parametrize("head", ["HEAD1", "HEAD2"])
def test_no_agpr_copy_block_behind_the_gather(asm_path, head):
    ins, _ = _instructions(asm_path, KERNELS[head])
    first_mfma = next(i for i, t in enumerate(ins) if t.startswith("v_mfma"))
    movs = [i for i in range(first_mfma) if ins[i].startswith("v_accvgpr_mov_b32")]
    # a handful of single moves may stay (hipcc's own spill slots in AGPRs); a relocation of the residual set is 232
    assert len(movs) < 32, f"{len(movs)} v_accvgpr_mov_b32 in front of the first layer"


def test_valu_per_step_below_parent(asm_path):
    import instruction_mix as IM

    _, total = IM.mix(asm_path)
    valu = IM.valu_total(total)
    print(f"VALU per wavefront-step: {valu:.0f} (parent {PARENT_VALU_PER_STEP}); per MFMA {valu / total['mfma']:.3f}")
    assert valu <= PARENT_VALU_PER_STEP - 4800, valu
