"""CPU: the inputs of tests/test_lngemm_gpu.py pinned without a device (tests/_lngemm_cases.py) — for every case the GPU test runs,

  * a float32 numpy emulation of the kernel's arithmetic (two-pass fp32 statistics, fp16 hi / lo split, the form's products summed in
    float64 and rounded to fp32 once) stays inside ONE QUARTER of the bar the case is given: the float64 reference describes the launch the
    kernel computes, and the bar leaves room for nothing but fp32 accumulation order;
  * every yardstick — W_lo / x_lo dropped in the main product, W_lo / the lo half of the hidden activations dropped in the prologue, the
    last k16-step missing, rows r and r ^ 32 exchanged, the columns rotated by one 32-wide tile — exceeds that bar at least 30 times: no
    case is vacuous; and the bar is at most 1e-2 of the smallest lo-dropped yardstick of the case (the ratio tests/test_attnout_gpu.py uses);
  * the bars of the one-product forms (hybrid: y rounded to fp16 once) are derived HERE: 3 x the difference between the emulation and the
    float64 reference, which rounds the float64 y where the kernel rounds the float32 y.  (The quarter rule cannot apply to them: their bar
    IS the emulation's distance.)

Also: the cases reach the 14 instantiations of launch_lngemm16x3, the panel unpackers invert the packers, and the restated pre-scale rule."""
import numpy as np
import pytest

import _lngemm_cases as LC

CASES = LC.all_cases()


def test_cases_reach_the_14_instantiations():
    got = {c.instantiation for c in LC.form_cases()}
    assert got == LC.INSTANTIATIONS and len(got) == 14
    assert len({c.id for c in CASES}) == len(CASES)
    assert {c.M % 128 for c in LC.form_cases()} == {119}


def test_prescale_rule_and_split():
    for mx, k in ((1.0, 1.0), (1.999, 1.0), (2.0, 0.5), (0.26, 4.0), (0.25, 4.0), (0.2499, 8.0), (7.3, 0.25)):
        assert LC.prescale(np.array([0.01, -mx], np.float32)) == k, mx
    w = (np.random.default_rng(0).standard_normal((64, LC.D)) * 0.06).astype(np.float32)
    hi, lo, k = LC.split_w(w)
    assert 1.0 <= np.abs(w * k).max() < 2.0
    assert np.abs((hi + lo) / k - w).max() <= 2.0 ** -22 * np.abs(w).max() + 2.0 ** -25 / k     # hi + lo carries 22 bits (or fp16's denormal spacing)


def test_panel_unpackers_invert_the_layout():
    rng = np.random.default_rng(1)
    M, P, halves = 37, 5, (37 + 3) * 32
    rows = rng.integers(1, 60000, (M, P * 32)).astype(np.uint16)
    flat = LC.pack_panels(rows, P, halves)
    for r, c in ((0, 0), (36, 159), (17, 33), (5, 95)):
        assert flat[(c // 32) * halves + (r * 64 + (c % 32) * 2) // 2] == rows[r, c]      # ldm_kernels.h: panel c / 32, byte r * 64 + (c % 32) * 2
    back = LC.unpack_panels(flat, P, halves)
    assert np.array_equal(back[:M], rows) and not back[M:].any()
    idx = LC.qkv_row(np.arange(3 * LC.D))
    assert idx[0] == 0 and idx[57] == 57 and idx[58] == 64 and idx[LC.D] == 8 * 64 and idx[-1] == 23 * 64 + 57 and len(set(idx.tolist())) == 3 * LC.D
    padded = np.arange(2 * 1536, dtype=np.float64).reshape(2, 1536)
    logical, pad = LC.qkv_logical(padded)
    assert logical.shape == (2, 3 * LC.D) and pad.shape == (2, 144) and logical[1, 58] == 1536 + 64 and pad[0, 0] == 58


def test_operands_are_what_the_issue_asks():
    c = LC.Case("split", LC.HEAD, prologue=True)
    op = LC.operands(c)
    h = op.hid_hi.astype(np.float64) + op.hid_lo.astype(np.float64)
    assert (h >= 0).all() and 0.45 < (op.hid_hi == 0).mean() < 0.55 and not op.hid_lo[op.hid_hi == 0].any()
    assert 1.8 < op.res.std() < 2.2
    x = LC.operands(LC.Case("split", LC.LINEAR1, layer=1)).x
    sd = x.std(-1)
    assert 0.25 < sd.min() and sd.max() < 3.5 and (np.abs(x.mean(-1)) <= 1.2 * sd).all()
    assert len(np.unique(x, axis=0)) == x.shape[0] and len(np.unique(x, axis=1).T) == x.shape[1]
    ln = LC.operands(LC.layernorm_cases()[0]).x
    assert ln[0].std() == 0 and np.count_nonzero(ln[1]) == 1 and ln[2].std() < 2e-3 and ln[3].std() > 5e2 and abs(ln[4].mean() / ln[4].std()) > 3.5


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_emulation_inside_a_quarter_of_the_bar_and_yardsticks_30_times_above(case):
    y, ref = LC.reference(case)
    ye, emu = LC.emulate(case)
    bar = LC.bar(case)
    e = LC.rel_err(emu, ref)
    op = LC.operands(case)
    ys = {w: LC.rel_err(LC.reference(case, w)[1], ref) for w in LC.applicable(case)}
    print(f"{case.id:48s} <{','.join(map(str, case.instantiation))}> bar {bar:.2e}  emulation {e:.2e}  " + "  ".join(f"{k} {v:.1e}" for k, v in ys.items()))
    if case.family == "one":
        assert 5e-6 < bar < 3e-4, bar      # a handful of fp16 roundings of y on the other side, each 2^-11 of ONE of 464 terms
        if case.out_form == 3:
            assert (np.abs(emu - ref) <= LC.HI_ONLY_REL * np.abs(ref) + bar * np.abs(ref).max()).all()
        else:
            assert e <= bar
    else:
        assert e <= bar / 4, (e, bar)
    if op.ada:
        ey = LC.rel_err(ye, y)
        assert ey <= LC.bar_y32(case) / 4, ey
    for k, v in ys.items():
        assert v >= 30 * bar, (k, v, bar)
    lo = [ys[k] for k in LC.LO_DROPPED if k in ys]
    if case.family != "one":
        assert lo and bar <= 1e-2 * min(lo), (bar, lo)
