"""GPU: ONE launch of the row-resident LayerNorm + GEMM kernel (layout_dm_amd/csrc/kernels_lngemm.hip lngemm16x3_k) of a live engine on the
test's rows (csrc/ldm_dev.cpp ldm_dev_lngemm_run: the product's own LnGemmArgs — images, pre-scales, parameter tables, mode — with the
workspace pointers and M swapped) against the float64 reference of that launch (tests/_lngemm_cases.py) — the kernel alone, without the
denoiser around it.  The logits of a whole pass are held to 2e-5 .. 1e-3 (tests/test_hip_parity.py, test_split_shapes_gpu.py,
test_mixed_gpu.py); a lo term dropped in one k16-step, one column tile, one accumulator chain or the prologue only, or a stale fragment in
the last row block, fits under that.  Here the bar is two orders of magnitude under a dropped lo term (tests/test_lngemm_reference.py pins
bars, operands and yardsticks on the CPU).

  * every one of the 14 instantiations launch_lngemm16x3 can pick (split, mixed, hybrid, hybrid with the two-launch FFN, split with fp32
    q / k / v rows) at M = 375; M in {1, 125, 128, 129, 255} for in_proj on tokens, in_proj and the head behind the linear2 prologue;
  * every output buffer larger than the launch needs and pre-filled with a NaN pattern: rows >= M, row-major columns >= N, panel rows
    beyond M and the bytes behind the last panel come back bit for bit (the EXEC row / column masks);
  * exact zeros in the logits' padding columns and in the head padding d = 58 .. 63 of every q / k / v panel; y32 in place (the product's
    own use) == y32 into a buffer of its own, bit for bit; LayerNorm edge rows (constant, one non-zero element, scale 1e-3 / 1e3, offset 4
    sigma); d_ff = 1840 / 1824 at d_model 464 (partly / wholly masked last tile), whole pass and the launches alone.

Reference: Block.forward / CategoricalTransformer.forward (oracle/restatement.py denoiser_logits restates them).

Measured on the MI355X, max |out - ref| / max |ref| (the printed table: profiles/lngemm_alone_check.txt):

  family                           cases   measured             bar
  three products (split)              28   3.1e-7 .. 6.4e-7     min(2.6e-6 = 4 x measured, 1e-2 x the case's smallest lo-dropped yardstick) = 1.3e-6 .. 2.2e-6
  two products (mixed, in_proj)       12   3.8e-7 .. 6.6e-7     min(2.7e-6, the same cap) = 1.9e-6 .. 2.3e-6
  one product, fp32 out (head)         2   3.8e-5, 6.7e-5       1.9e-4, 8.8e-5   (3 x the CPU emulation's distance)
  one product, fp16 out (linear1)      1   2.8e-5 beyond 2^-11 |ref|            5.5e-5
  LayerNorm edge rows                  2   5.3e-7, 7.9e-7       min(3.2e-6, cap) = 2.1e-6
  y32, rows read or gathered          11   1.6e-7 .. 3.9e-7     1.6e-6
  y32 behind the linear2 prologue     10   5.7e-7 .. 1.2e-6     4.7e-6
  d_ff 1840 / 1824, whole pass         4   split 3.7e-7, mixed 6.8e-4            LOGIT_REL_TOL (5e-5 / 1e-3)

4 x measured lies ABOVE the cap for the three- and two-product forms: the cap binds, the margin over the measured values is 2 - 4, not 4.  The
values are bit-repeatable (seeded operands, a deterministic kernel); what they consist of is the fp32 accumulation order (tests/_lngemm_cases.py,
tolerances).  Mutation check, by hand: with the W_lo x_hi MFMA of k16-step 13 of lg_step removed, the three-product cases here measure 4.9e-5 ..
6.2e-5 (25 - 30 x their bars; the two-product cases do not move), the logits of a whole pass 4.3e-5 .. 6.1e-5.
"""
import ctypes

import numpy as np
import pytest
import torch

import _lngemm_cases as LC
from oracle import restatement as R

pytestmark = pytest.mark.gpu

D = LC.D
VP = ctypes.c_void_p


class Io(ctypes.Structure):   # csrc/ldm_dev.cpp ldm_dev_lngemm_io
    _fields_ = [("launch", ctypes.c_int32), ("layer", ctypes.c_int32), ("t", ctypes.c_int32), ("prologue", ctypes.c_int32), ("M", ctypes.c_int32),
                ("pre_lda", ctypes.c_int32), ("tokens", VP), ("x", VP), ("hid_hi", VP), ("hid_lo", VP), ("res", VP), ("y32", VP), ("C32", VP),
                ("C16", VP), ("C16lo", VP), ("ldc32", ctypes.c_int64), ("ldc16", ctypes.c_int64), ("panel_stride", ctypes.c_uint64),
                ("pre_panel_stride", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def engines():
    """One engine per (mode, d_ff), built on first use; knob engines are created under a patched environment (the knobs are read at create)."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from layout_dm_amd.binding import Engine

    cache = {}

    def get(mode, d_ff=1856):
        if (mode, d_ff) not in cache:
            m = LC.MODES[mode]
            with pytest.MonkeyPatch.context() as mp:
                for k, v in m.env:
                    mp.setenv(k, v)
                e = Engine(n_category=25, precision=m.precision, max_batch=4, d_ff=d_ff)
            e.load_state_dict(LC.state_dict(m.point, d_ff))
            fn = e.lib.ldm_dev_lngemm_run
            fn.argtypes, fn.restype = [VP, ctypes.POINTER(Io)], ctypes.c_int
            cache[(mode, d_ff)] = e
        return cache[(mode, d_ff)]

    yield get
    for e in cache.values():
        e.close()


MEASURED = {}   # family -> {case id: error}, printed by the last test


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint16, np.float16):
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def run_launch(e, case, alias_y=False):
    """The launch of `case` on engine e -> dict: out_hi / out_lo (fp16 forms, [M, N] in the image's column order) or out (fp32), y, and
    `guards`: a list of (name, ok) for every band that must come back untouched."""
    op, M = LC.operands(case), case.M
    F, Fp = case.d_ff, (case.d_ff + 63) // 64 * 64
    io = Io(launch=case.launch, layer=case.layer, t=case.t, prologue=int(case.prologue), M=M)
    keep = []

    def dev(a):
        t = _dev(a)
        keep.append(t)
        return t

    if case.prologue:
        cols = Fp
        hh, hl = (np.zeros((M, cols), np.uint16) for _ in range(2))
        hh[:, :F], hl[:, :F] = op.hid_hi.view(np.uint16), op.hid_lo.view(np.uint16)
        if case.hid_panels:
            halves = (M + 1) * 32
            io.pre_panel_stride = halves * 2
            hh, hl = LC.pack_panels(hh, cols // 32, halves), LC.pack_panels(hl, cols // 32, halves)
        else:
            io.pre_lda = cols + 8
            hh, hl = (np.concatenate([a, np.zeros((M, 8), np.uint16)], 1) for a in (hh, hl))
        io.hid_hi, io.res = dev(hh).data_ptr(), dev(op.res).data_ptr()
        if case.np_pre > 1:
            io.hid_lo = dev(hl).data_ptr()
    elif case.tokens:
        io.tokens = dev(op.tokens).data_ptr()
    ROWS = M + 3
    y = None
    if op.ada:
        if alias_y:
            assert op.x is not None
            ybuf = np.full((ROWS, D), LC.NAN32, np.uint32)
            ybuf[:M] = op.x.view(np.uint32)
            y = dev(ybuf)
            io.x = io.y32 = y.data_ptr()
        else:
            y = dev(np.full((ROWS, D), LC.NAN32, np.uint32))
            io.y32 = y.data_ptr()
    if op.x is not None and not io.x:
        io.x = dev(op.x).data_ptr()
    form = case.out_form
    N = {LC.IN_PROJ: 1536 if form == 2 else 3 * D, LC.LINEAR1: F, LC.HEAD: 160}[case.launch]
    panels = form in (2, 3) or (form == 1 and case.hid_panels)
    if form == 0:
        ld = N + 8
        io.ldc32 = ld
        c32 = dev(np.full((ROWS, ld), LC.NAN32, np.uint32))
        io.C32 = c32.data_ptr()
    elif panels:
        n_panels = (N + 31) // 32 + (1 if N % 64 else 0)       # (d_ff 1824: the 58th, wholly masked tile owns a panel the launch must not touch)
        prow = M + 5
        io.panel_stride = prow * 64
        total = n_panels * prow * 32 + 128
        c16 = dev(np.full(total, LC.NAN16, np.uint16))
        io.C16 = c16.data_ptr()
        if form != 3:
            c16lo = dev(np.full(total, LC.NAN16, np.uint16))
            io.C16lo = c16lo.data_ptr()
    else:
        ld = Fp + 8
        io.ldc16 = ld
        c16, c16lo = (dev(np.full((ROWS, ld), LC.NAN16, np.uint16)) for _ in range(2))
        io.C16, io.C16lo = c16.data_ptr(), c16lo.data_ptr()
    torch.cuda.synchronize()
    rc = e.lib.ldm_dev_lngemm_run(e._h, ctypes.byref(io))
    if rc == -2:    # a HIP error: nothing more runs on this device from this module
        pytest.exit(f"{case.id}: {e.lib.ldm_last_error(e._h).decode()}", returncode=3)
    assert rc == 0, (case.id, rc, e.lib.ldm_last_error(e._h).decode())
    res, guards = {}, []
    if y is not None:
        yb = _host(y, np.uint32)
        res["y"] = yb[:M].view(np.float32)
        guards.append(("y32 rows >= M", bool((yb[M:] == LC.NAN32).all())))
    if form == 0:
        cb = _host(c32, np.uint32)
        res["out"] = cb[:M, :N].view(np.float32)
        guards += [("C32 rows >= M", bool((cb[M:] == LC.NAN32).all())), ("C32 columns >= N", bool((cb[:M, N:] == LC.NAN32).all()))]
    elif panels:
        for name, buf in (("hi", c16),) + ((("lo", c16lo),) if form != 3 else ()):
            b = _host(buf, np.uint16)
            full = LC.unpack_panels(b, n_panels, prow * 32)
            res["out_" + name] = full[:M, :N].view(np.float16)
            guards += [(f"{name} panel rows >= M", bool((full[M:] == LC.NAN16).all())), (f"{name} columns >= N", bool((full[:M, N:] == LC.NAN16).all())),
                       (f"{name} bytes behind the last panel", bool((b[n_panels * prow * 32:] == LC.NAN16).all()))]
    else:
        for name, buf in (("hi", c16), ("lo", c16lo)):
            b = _host(buf, np.uint16)
            res["out_" + name] = b[:M, :N].view(np.float16)
            guards += [(f"{name} rows >= M", bool((b[M:] == LC.NAN16).all())), (f"{name} columns >= N", bool((b[:M, N:] == LC.NAN16).all()))]
    res["guards"] = guards
    return res


def check(case, res, note=""):
    """Every figure printed before it is asserted; returns the launch's error."""
    y_ref, ref = LC.reference(case)
    bar, form = LC.bar(case), case.out_form
    hi = res["out"] if form == 0 else res["out_hi"]
    out = hi.astype(np.float64) + (res["out_lo"].astype(np.float64) if form in (1, 2) else 0.0)
    zeros_ok = True
    if case.launch == LC.HEAD:
        zeros_ok = bool((out[:, 155:] == 0).all())
        out = out[:, :155]
    elif form == 2:
        out = LC.qkv_logical(out)[0]
        zeros_ok = bool((LC.qkv_logical(res["out_hi"])[1] == 0).all() and (LC.qkv_logical(res["out_lo"])[1] == 0).all())
    err = LC.rel_err(out, ref)
    r, c, wave, tile = LC.worst_location(out, ref)
    if form == 3:   # plain fp16 out: what exceeds its own rounding 2^-11 |ref| is held to the bar
        excess = np.maximum(np.abs(out - ref) - LC.HI_ONLY_REL * np.abs(ref), 0.0)
        err = float(excess.max() / np.abs(ref).max())
        r, c, wave, tile = LC.worst_location(excess, np.zeros_like(excess))
    line = (f"{case.id:42s} <{','.join(map(str, case.instantiation))}> err {err:.2e} (bar {bar:.2e}) at row {r} col {c} wave {wave} tile {tile}")
    ey = None
    if "y" in res:
        ey = LC.rel_err(res["y"], y_ref)
        line += f"  y32 {ey:.2e}"
    bad = [n for n, ok in res["guards"] if not ok]
    print(line + note + ("" if not bad else f"  GUARDS TOUCHED: {bad}") + ("" if zeros_ok else "  PADDING NOT ZERO"), flush=True)
    fam = "ln_rows" if case.rows == "layernorm" else case.family
    MEASURED.setdefault(fam, {})[case.id] = err
    if ey is not None:
        MEASURED.setdefault("ln_rows_y32" if case.rows == "layernorm" else "y32", {})[case.id] = ey
    assert not bad, bad
    assert zeros_ok
    assert err <= bar, (case.id, err, bar, (r, c, wave, tile))
    if ey is not None:
        assert ey <= LC.bar_y32(case), (case.id, ey)
    return err


FORM_CASES = LC.form_cases()
RAN = set()


@pytest.mark.parametrize("case", FORM_CASES, ids=[c.id for c in FORM_CASES])
def test_every_instantiation_against_float64(engines, case):
    e = engines(case.mode)
    d = e.describe()
    assert d["precision"] == LC.MODES[case.mode].precision + "_f16"
    check(case, run_launch(e, case))
    RAN.add((case.mode, case.launch, case.prologue, case.instantiation))


def test_the_cases_ran_reach_all_14_instantiations():
    assert {i for _, _, _, i in RAN} == LC.INSTANTIATIONS, sorted(LC.INSTANTIATIONS - {i for _, _, _, i in RAN})
    assert {(m, l, p) for m, l, p, _ in RAN} == {(c.mode, c.launch, c.prologue) for c in FORM_CASES}


ROW_CASES = LC.row_cases()


@pytest.mark.parametrize("case", ROW_CASES, ids=[c.id for c in ROW_CASES])
def test_row_counts_around_the_128_row_block(engines, case):
    check(case, run_launch(engines(case.mode), case))


@pytest.mark.parametrize("case", LC.layernorm_cases(), ids=[c.id for c in LC.layernorm_cases()])
def test_layernorm_edge_rows(engines, case):
    check(case, run_launch(engines(case.mode), case))


def test_y32_in_place_is_y32_into_its_own_buffer(engines):
    """The product's own use: a.x = a.y32 = ws.P"""
    case = LC.Case("split", LC.IN_PROJ, layer=3, M=255, seed=5)
    e = engines("split")
    a, b = run_launch(e, case), run_launch(e, case, alias_y=True)
    check(case, a)
    check(case, b, note="  (in place)")
    for k in ("y", "out_hi", "out_lo"):
        assert np.array_equal(a[k].view(np.uint16 if k != "y" else np.uint32), b[k].view(np.uint16 if k != "y" else np.uint32)), k


def test_the_hook_refuses_what_the_handle_does_not_run(engines):
    e = engines("hybrid")      # FFN behind the attention: no linear1 launch, no prologue
    for case in (LC.Case("hybrid", LC.LINEAR1, layer=1, M=8), LC.Case("hybrid", LC.HEAD, prologue=True, M=8)):
        io = Io(launch=case.launch, layer=case.layer, t=0, prologue=int(case.prologue), M=8)
        assert e.lib.ldm_dev_lngemm_run(e._h, ctypes.byref(io)) == -1
    s = engines("split")
    io = Io(launch=LC.IN_PROJ, layer=0, t=0, prologue=1, M=8)      # nothing in front of layer 0
    assert s.lib.ldm_dev_lngemm_run(s._h, ctypes.byref(io)) == -1
    from layout_dm_amd.binding import Engine
    x = Engine(n_category=25, precision="exact", max_batch=4)
    x.load_state_dict(LC.state_dict("perturb"))
    assert x.lib.ldm_dev_lngemm_run(x._h, ctypes.byref(Io(launch=LC.HEAD, M=8))) == -1
    x.close()


# ---------------------------------------------------------------------------------------------------------------- other d_ff at d_model 464
DFF_CASES = LC.dff_cases()


@pytest.mark.parametrize("case", DFF_CASES, ids=[c.id for c in DFF_CASES])
def test_other_d_ff_launches_alone(engines, case):
    check(case, run_launch(engines(case.mode, case.d_ff), case))


@pytest.mark.parametrize("mode", ["split", "mixed"])
@pytest.mark.parametrize("d_ff", LC.DFF_GEOMETRIES)
def test_other_d_ff_whole_pass_against_the_oracle(engines, mode, d_ff):
    from test_hip_parity import LOGIT_REL_TOL

    e = engines(mode, d_ff)
    spec = LC.spec_for(d_ff)
    W = R.as_torch_weights(LC.state_dict(LC.MODES[mode].point, d_ff), torch.float64)
    tokens = torch.randint(0, spec.n_class, (2, spec.seq_len), generator=torch.Generator().manual_seed(d_ff))
    ref = R.denoiser_logits(W, spec, tokens, 41, dtype=torch.float64)
    out = e.denoise_logits(tokens.int(), 41).cpu()[..., :spec.n_class].double()
    err = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"d_ff {d_ff} {mode}: logits of a whole pass vs float64 {err:.2e} (hidden activations: {'panels' if d_ff % 32 == 0 else 'rows'})")
    assert err <= LOGIT_REL_TOL[mode]


def test_hybrid_at_d_ff_1840_is_refused_at_create():
    """Its plain-fp16 hidden activations exist as 32-column panels only: d_ff % 32 != 0 is refused with a message, not at the first pass."""
    from layout_dm_amd.binding import Engine

    with pytest.raises(RuntimeError, match="precision hybrid: d_ff must be a multiple of 32"):
        Engine(n_category=25, precision="hybrid", max_batch=4, d_ff=1840)


def test_print_the_measured_table():
    """(last: what profiles/lngemm_alone_check.txt holds)"""
    print("\nfamily            cases   largest error   at")
    for fam in sorted(MEASURED):
        worst = max(MEASURED[fam], key=MEASURED[fam].get)
        print(f"{fam:16s}  {len(MEASURED[fam]):5d}   {MEASURED[fam][worst]:.2e}        {worst}")
    assert MEASURED
