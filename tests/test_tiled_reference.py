"""CPU: the inputs of tests/test_tiled_kernels_gpu.py pinned without a device (tests/_tiled_cases.py) — for every case the GPU test runs,

  * every yardstick (operands rounded to fp16, the last K tile left out, the hi-only product of the fp16 x 3 kernels, an unbiased variance, a
    gather one position on) lies at least 100 x above the distance of the CPU emulation of that case from float64: a dropped term cannot
    hide under the bar, which is min(4 x that distance, 1e-2 x the smallest yardstick);
  * the bars of the fp16-product kernels (gemm16, attention16) are 3 x the emulation's distance and stay under what their formats allow;
  * the case lists reach every instantiation the issue names, every K-tile count against the ring depth, every epilogue form, the XCD
    remap's remainders and both sides of every switch of the dispatchers.

Also: the operands are what the issue asks (weights with max |w| in [1, 2), lo = fp16(x - fp16(x)), whole-tile buffers with large finite
padding rows, three layouts of different amplitude, flat and peaked scores, the LayerNorm edge rows)."""
import numpy as np
import pytest

import _tiled_cases as TC

GEMM_CASES = TC.exact_gemm_cases() + TC.x3_gemm_cases() + TC.f16_gemm_cases()
ATTN_CASES = TC.attention_cases() + TC.attention16_cases()
LN_CASES = TC.layernorm_cases()


def test_the_case_list_reaches_every_instantiation():
    got = {c.instantiation for c in GEMM_CASES} | {c.kernel for c in ATTN_CASES} | {f"ln_rows<{c.nv}>" for c in LN_CASES}
    assert got == TC.ALL_INSTANTIATIONS and len(got) == 21, sorted(TC.ALL_INSTANTIATIONS ^ got)
    for cases in (GEMM_CASES, ATTN_CASES, LN_CASES):
        assert len({c.id for c in cases}) == len(cases)


def test_gemm_cases_reach_the_edges_the_issue_lists():
    ex = TC.exact_gemm_cases()
    assert {c.K for c in ex} == {16, 32, 48, 464} and {c.nk for c in ex} == {1, 2, 3, 29}
    assert {1, 127, 128, 129, 257} <= {c.M for c in ex} and {1, 129, 155, 283, 464} <= {c.N for c in ex}
    assert {1, 3, 7} <= {c.n_tiles % 8 for c in ex}
    assert {c.form for c in ex} == set(TC.EXACT_FORMS)
    assert all(c.ldc > c.N and c.ldres != c.ldc and c.lda > c.K for c in ex)
    assert {(c.N, c.ldc) for c in ex if c.N in (155, 283)} == {(155, 160), (283, 288)}
    w = TC.exact_wrap_case(256)
    assert w.n_tiles > 6 * 256 and w.M % 128 and w.N % 128 and w.K == 32
    x3 = TC.x3_gemm_cases()
    assert {c.tag for c in x3} == {0, 1, 2, 3, 4} and len({(c.M, c.N, c.K) for c in x3 if c.tag in (0, 1, 2, 3) and c.M == 257 and c.N == 464 and c.K == 64}) == 1
    for tag, stages in ((0, 2), (4, 3)):
        t = [c for c in x3 if c.tag == tag]
        assert {c.K for c in t} == {32, 64, 96, 512} and {c.tile[3] for c in t} == {stages}
        assert {np.sign(c.nk - stages) for c in t} == {-1, 0, 1}        # fewer, equal and more K tiles than ring stages
        assert {c.M for c in t} == {1, 255, 256, 257} and {c.N for c in t} == {155, 283, 256, 257, 464}
        assert {"bias", "bias_res", "relu_hilo"} <= {c.form for c in t}
    f = TC.f16_gemm_cases()
    assert {c.tag for c in f} == {0, 1, 2, 3, 4} and {c.K for c in f} == {64, 128, 512}
    assert {c.M for c in f} == {1, 127, 128, 129} and {c.N for c in f} == {155, 283, 128, 129, 464}
    assert {"c16", "bias_res"} <= {c.form for c in f}


def test_attention_cases_reach_the_kernels_the_issue_assigns():
    by = {}
    for c in TC.attention_cases():
        by.setdefault(c.kernel, []).append(c)
    x3 = by["attention16x3"]
    assert all(c.split and c.dh == 58 for c in x3) and {c.S for c in x3 if c.H == 8} == {1, 31, 32, 33, 64, 97, 125, 128}
    assert any(c.H == 16 and c.D == 928 for c in x3)
    assert {c.S for c in by["attn32_direct_k"]} == {97, 125, 128} and not any(c.split for c in by["attn32_direct_k"])
    m = by["attn32_mfma_k"]
    assert {(c.S, c.H, c.dh, c.D) for c in m} == {(97, 16, 57, 912), (128, 16, 57, 912)} and {c.split for c in m} == {False, True}
    r60 = by["attn_rows<float,60>"]
    assert {c.S for c in r60 if c.dh == 58 and not c.split} == {1, 50, 96, 129, 150} and {c.S for c in r60 if c.dh == 58 and c.split} == {129}
    assert {c.split for c in r60 if c.dh == 36} == {False, True}
    assert {c.dh for c in by["attn_rows<float,32>"]} == {32, 24} and {c.dh for c in by["attn_rows<float,64>"]} == {64, 62}
    for k in ("attn_rows<float,32>", "attn_rows<float,64>"):
        assert {(c.dh, c.split) for c in by[k]} == {(d, s) for d in {c.dh for c in by[k]} for s in (False, True)}
    assert any(c.D == 496 for c in by["attn_rows<float,64>"])
    assert {c.amp for c in TC.attention_cases()} == {0.3, 2.5}
    # what no whole pass reaches comes last
    firsts = [c.first_run for c in TC.attention_cases()]
    assert firsts == sorted(firsts)
    assert {c.kernel for c in TC.attention_cases() if c.first_run} == {"attn32_mfma_k", "attn_rows<float,32>", "attn_rows<float,60>"}
    assert all(c.dh == 36 for c in r60 if c.first_run)
    a16 = TC.attention16_cases()
    assert {(c.dh, c.S) for c in a16} == {(d, s) for d in (58, 64, 32) for s in (1, 33, 125, 128)} and all(c.kernel == "attn_mfma_k" for c in a16)


def test_layernorm_cases_reach_both_sides_of_each_switch():
    assert {(c.D, c.nv) for c in LN_CASES} == {(16, 1), (256, 1), (260, 2), (464, 2), (512, 2), (516, 4), (1024, 4)}
    assert {c.M for c in LN_CASES} == {1, 3, 4, 5, 129}
    for nv in (1, 2, 4):
        assert {(c.form, c.outs) for c in LN_CASES if c.nv == nv} >= {(f, o) for f in ("ada", "affine", "gather") for o in TC.LN_OUTS} | {("raw", "y32")}
    assert all(c.ld16 > c.D for c in LN_CASES)
    firsts = [c.first_run for c in LN_CASES]
    assert firsts == sorted(firsts)
    x = TC.layernorm_operands(TC.LnCase(464, 129, "ada", "y32_y16_lo", edge=True))["x"]
    assert x[0].std() == 0 and np.count_nonzero(x[1]) == 1 and x[2].std() < 2e-3 and x[3].std() > 5e2 and abs(x[4].mean() / x[4].std()) > 3.5


def test_operands_are_what_the_issue_asks():
    c = TC.GemmCase(TC.X3, 255, 283, 64, "relu_hilo", 0)
    op = TC.gemm_operands(c)
    assert op.A_hi.shape == (256, 64) and op.W_hi.shape == (512, 64) and op.scale == 2.0 ** -3
    assert 1.0 <= np.abs(op.W).max() < 2.0
    assert (op.A_hi[255:] == TC.PAD_VALUE).all() and (op.W_hi[283:] == TC.PAD_VALUE).all() and (op.W_lo[283:] == 0.5).all()
    for x32, hi, lo, n in ((op.A32, op.A_hi, op.A_lo, 255), (op.W32, op.W_hi, op.W_lo, 283)):
        h = x32.astype(np.float16)
        assert np.array_equal(h, hi[:n]) and np.array_equal((x32 - h.astype(np.float32)).astype(np.float16), lo[:n])      # lo = fp16(x - fp16(x))
    q, k, v = TC.attention_operands(TC.AttnCase(125, 8, 58))
    amp = [float(v[b].std()) for b in range(3)]
    assert amp[1] > 3 * amp[0] > 9 * amp[2]
    for want in (0.3, 2.5):
        q, k, _ = TC.attention_operands(TC.AttnCase(125, 8, 58, amp=want))
        s = (q.astype(np.float64) @ np.swapaxes(k.astype(np.float64), -1, -2) / np.sqrt(58)).std()
        assert 0.9 * want < s < 1.1 * want
    rows = TC.attention_rows(TC.AttnCase(33, 8, 58, f16=True), *TC.attention_operands(TC.AttnCase(33, 8, 58, f16=True)))
    assert rows.shape == (99, 1536) and not rows.reshape(99, 24, 64)[..., 58:].any()


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c.id for c in GEMM_CASES])
def test_gemm_yardsticks_100_times_above_the_emulation(case):
    bar, emu, ys, binds = TC.gemm_figures(case)
    print(f"{case.id:44s} {case.instantiation:34s} emulation {emu:.2e}  bar {bar:.2e} ({binds})  " + "  ".join(f"{k} {v:.1e}" for k, v in ys.items()))
    assert emu > 0
    if case.kind == TC.F16:
        c16 = not TC.FORMS[case.form][3]
        assert bar < (3 * 2.0 ** -11 if c16 else 2e-5)      # its own output rounding | fp32 accumulation of exact fp16 products
        return
    assert ys and all(v >= 100 * emu for v in ys.values()), (emu, ys)
    assert bar <= 4 * emu and bar <= 1e-2 * min(ys.values())


@pytest.mark.parametrize("case", ATTN_CASES, ids=[c.id for c in ATTN_CASES])
def test_attention_yardsticks_100_times_above_the_emulation(case):
    bar, emu, ys, binds = TC.attention_figures(case)
    print(f"{case.id:34s} {case.kernel:22s} emulation {emu:.2e}  bar {bar:.2e} ({binds})  " + "  ".join(f"{k} {v:.1e}" for k, v in ys.items()))
    assert emu > 0 or (case.S == 1 and not case.split)      # (one key: p = 1 and the output IS v, bit for bit — the bar is 0)
    if case.f16:
        assert bar < 3 * 2.0 ** -10        # P and the output rounded to fp16 once each
        return
    assert ys and all(v >= 100 * emu for v in ys.values()), (emu, ys)
    assert bar <= 4 * emu and bar <= 1e-2 * min(ys.values())


@pytest.mark.parametrize("case", LN_CASES, ids=[c.id for c in LN_CASES])
def test_layernorm_yardsticks_100_times_above_the_emulation(case):
    bar, emu, ys, binds, bar_stats = TC.layernorm_figures(case)
    print(f"{case.id:40s} ln_rows<{case.nv}> emulation {emu:.2e}  bar {bar:.2e} ({binds})  statistics' bar {bar_stats:.2e}  " +
          "  ".join(f"{k} {v:.1e}" for k, v in ys.items()))
    assert ys and all(v >= 100 * emu for v in ys.values()), (emu, ys)
    assert 0 < bar <= 4 * emu and bar <= 1e-2 * min(ys.values())
    if case.form == "raw":      # y32 = emb + pos: the float32 sum, bit for bit
        ye, _ = TC.layernorm_emulate(case)
        op = TC.layernorm_operands(case)
        assert np.array_equal(ye.astype(np.float32), op["emb"][op["tokens"]] + op["pos"][np.arange(case.M) % TC.LN_S])


def test_hi_within_one_ulp_helper():
    ref = np.array([1.0, 1e-3, 300.0, 0.0])
    assert TC.hi_within_one_ulp(ref.astype(np.float16), ref, 0.0)
    assert TC.hi_within_one_ulp(np.nextafter(ref.astype(np.float16), np.float16(np.inf)), ref, 0.0)
    bad = ref.astype(np.float16).copy()
    bad[2] = np.float16(300.75)     # three ulps at 300
    assert not TC.hi_within_one_ulp(bad, ref, 0.0)


def test_the_library_exports_the_three_hooks():
    """Development hooks (csrc/ldm_dev.cpp), like ldm_dev_lngemm_run outside include/ldm_hip.h and binding.EXPORTS: the GPU test declares them itself"""
    import ctypes

    from layout_dm_amd import build

    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("ldm_dev_layernorm_run", "ldm_dev_gemm_run", "ldm_dev_attention_run"):
        assert hasattr(lib, name), name
    for fn in (lib.ldm_dev_layernorm_run, lib.ldm_dev_gemm_run, lib.ldm_dev_attention_run):
        fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
        assert fn(None) == -1       # (a null io is refused before anything touches a device)
