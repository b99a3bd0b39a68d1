"""Static checks on the per-layout-timestep forms of the row-resident LayerNorm + GEMM kernel (kernels_lngemm.hip, the LG_PLT bit
of lngemm16x3_k's variant argument; no GPU needed: hipcc cross-compiles).

These forms read their AdaLN parameters per lane from global memory at the one place of the kernel where the register file is
full (58 float4 of raw row values live, one wave per SIMD).  Checked on the ISA: the seven in_proj forms exist, none uses scratch,
and each passes EVERYTHING tests/test_kernel_asm_lint.py holds its single-t twin to — that test is run on an assembly in which
every in_proj form carries the code of its per-layout form (MFMA counts, the schedule of every step statement, the counted
vmcnt waits of the GEMM prologue, the wait states behind the last MFMAs, no early read of an accumulator)."""
import re

import test_kernel_asm_lint as LINT

PLT = re.compile(r"lngemm16x3_kILb1ELi([02])ELb0ELi256ELb([01])ELi([23])ELi([123])EEEvNS_10LnGemmArgsE$")
FORMS = {(2, 0, 3, 3), (2, 1, 3, 3), (0, 0, 3, 3), (0, 1, 3, 3), (2, 0, 2, 2), (2, 1, 2, 2), (2, 1, 2, 1)}   # <OUT, PRE, NPM, NPP>


def test_the_seven_in_proj_forms_exist_without_scratch():
    asm = LINT._compile("kernels_lngemm.hip")
    kernels = {k: v for k, v in LINT._kernels(asm).items() if PLT.search(k)}
    assert {tuple(int(x) for x in PLT.search(k).groups()) for k in kernels} == FORMS and len(kernels) == 7, list(kernels)
    sizes = dict(re.findall(r"\.amdhsa_kernel\s+(\S+)[\s\S]*?\.amdhsa_private_segment_fixed_size\s+(\d+)", asm))
    for name, instr in kernels.items():
        assert int(sizes[name]) == 0 and not [i for i in instr if i.startswith("scratch_")], name
        # the parameters come from global memory per lane: 58 groups x (scale, shift) float4 loads that the twin does not have
        twin = LINT._kernels(asm)[name.replace("ELi256E", "ELi0E")]
        loads = lambda ins: len([i for i in ins if i.startswith("global_load_dwordx4")])   # noqa: E731
        assert loads(instr) - loads(twin) == 2 * 58, (name, loads(instr), loads(twin))


def test_the_per_layout_forms_pass_the_lint_of_their_twins(monkeypatch):
    asm = LINT._compile("kernels_lngemm.hip")
    names = [k for k in LINT._kernels(asm) if PLT.search(k)]
    assert len(names) == 7
    swapped = asm
    for name in names:   # the twin leaves under another name, the per-layout form takes the twin's
        twin = name.replace("ELi256E", "ELi0E")
        swapped = swapped.replace(twin, twin.replace("lngemm16x3_k", "lngemm16x3_single_t"))
        swapped = swapped.replace(name, twin)
    assert swapped != asm and not [k for k in LINT._kernels(swapped) if PLT.search(k)]
    monkeypatch.setattr(LINT, "_compile", lambda src: swapped)
    LINT.test_lngemm_reachable_forms_no_scratch_and_mfma_hazards()
