"""GPU: ONE launch of the fused attention + out_proj (+ LayerNorm-2 + plain-fp16 FFN) kernel (layout_dm_amd/csrc/kernels_attnout.hip
attnout16x3_k) of a live engine on the test's panels (csrc/ldm_dev.cpp ldm_dev_attnout_run: the product's own AttnOutArgs of a layer — out_proj's
k-step image, bias and pre-scale, the two-product flag, the FFN's chunk image and parameters — with the panels, their stride, res, out, B and S
swapped) against the float64 reference of that launch (tests/_attnout_cases.py) — the kernel alone, without the denoiser around it.  The logits of
a whole mixed / hybrid pass are held to 1e-3, and a dropped lo product in one out_proj stage or a skipped FFN chunk fits under that; here the bars
are derived on the CPU from an emulation of the kernel's number formats and from wrong references on the same operands
(tests/test_attnout_reference.py pins them; nothing in a bar comes from the device).

  * the three instantiations launch_attnout16x3 picks (split <false>, mixed <false, W2>, hybrid <false, W2, FFN>) at B = 3, S = 125 on the
    first and on the last layer; S in {1, 31, 32, 33, 50, 64, 65, 96, 97, 127, 128} at B = 2 (and B = 1 at S = 1, 128) for each: waves without
    rows, with one row, with all of them; key tiles wholly masked, partly masked, unmasked; layout starts that are only 64-byte aligned;
  * q / k amplitudes 0.3, 1, 2.5, q = 0 (P = 1 / S: also against the mean of V through Wo) and a peaked case (largest scaled score 41: one key
    carries the row, the others' 2^10 p are fp16 denormals or zero); V with another amplitude per layout; the panel rows behind the last
    layout, up to the 128-row reach = the END of every panel, hold 1000.0 (the kernel's contract: finite values, masked);
  * hybrid at d_ff 1856, 1824, 2048 and 32 (58, 57, 64 chunks and one), and in place (ffn_out == res, the product's own use) == out of place
    bit for bit;
  * the output buffer is 3 rows and a tail longer than the launch needs and pre-filled with a NaN pattern: rows >= B S and the tail come back bit
    for bit (the m < nrow / r < nrow store masks, waves with nrow <= 0 included), no NaN in the real rows, res unchanged by an out-of-place launch;
  * the hook's refusals, each -1 with the output untouched.

Reference: torch.nn.MultiheadAttention and the FFN inside Block.forward (oracle/restatement.py denoiser_logits restates them).

Measured on the MI355X, max |out - ref| / max |ref - res| (the printed table: profiles/attnout_alone_check.txt):

  family                         cases   measured             bar
  three products (split)            20   3.0e-7 .. 9.0e-7     min(4 x the emulation's distance, 1e-2 x the case's smallest yardstick) = 5.0e-7 .. 2.1e-6
  two-product out_proj (mixed)      20   9.7e-8 .. 8.1e-7     the same rule = 4.9e-7 .. 2.7e-6
  out_proj + FFN (hybrid), 31+ rows 18   3.4e-5 .. 1.35e-4    3 x the emulation's distance = 1.6e-4 .. 4.1e-4
  out_proj + FFN, S = 1              2   2.9e-7, 4.8e-7       4.8e-7, 9.7e-7
  in place == out of place           1   bit for bit
  q = 0 against the mean of V        2   5.0e-7, 3.2e-7       the case's bar (1.3e-6, 1.0e-6)

Closest to its bar: mixed-L2-B1-S1 at 0.87 of it, split-L2-B1-S128 at 0.78 (there 4 x the emulation binds; the cap binds where Wo's dropped lo half
is the smallest yardstick); the values are bit-repeatable (seeded operands, a deterministic kernel).  The emulation follows the kernel's order of
accumulation, and four FFN cases (B = 3 on layers 0 and 3, S = 50, S = 97) measure its distance to three digits: what the FFN form's error consists of is fp16 roundings of the
LayerNorm-2 output and of hidden activations that the fp32 kernel and the float64 reference take to different neighbours.  With one row a single
such rounding IS the figure: on operands with a hidden pre-activation 0.6 fp32 ulps from a rounding boundary (seed 1 of the B = 1, S = 1 case)
the device took the other neighbour — 4.5e-6 where the emulation, which sums the 16 products of an MFMA exactly, had 2.5e-7 — so the FFN cases
at S = 1 use operands without a rounding decided by less than 8 fp32 ulps (tests/_attnout_cases.py near_ties, TIE_FREE_SEED).
No case faulted or touched a guard row: the d_ff geometries (58, 57, 64 chunks and one), waves with nrow <= 0 in the FFN path and the half == 1
clamp of dma_prow at small S are as the kernel's comments state them; the kernel and its launcher are unchanged.
Mutation check, by hand (profiles/attnout_alone_check.txt): with the Wo_lo · O_hi MFMA of out_proj stage 2 removed the split cases here measure
2.5e-5 .. 1.2e-4 (40 - 100 x their bars; the logits of a whole split pass 1.5e-5 against 4.2e-7, inside that test's 5e-5); with the last
iteration of the FFN chunk loop removed the hybrid cases measure 9.4e-2 .. 1.0 (500 x their bars and more; a whole hybrid pass 2.1e-1).
"""
import ctypes

import numpy as np
import pytest
import torch

import _attnout_cases as AC
import _lngemm_cases as LC

pytestmark = pytest.mark.gpu

D = AC.D
VP = ctypes.c_void_p
TAIL = 96      # uint32 words behind the output's last row


class Io(ctypes.Structure):   # csrc/ldm_dev.cpp ldm_dev_attnout_io
    _fields_ = [("layer", ctypes.c_int32), ("B", ctypes.c_int32), ("S", ctypes.c_int32), ("pad_", ctypes.c_int32), ("qkv_hi", VP), ("qkv_lo", VP),
                ("panel_stride", ctypes.c_uint64), ("res", VP), ("out", VP), ("panel_rows", ctypes.c_int64), ("res_rows", ctypes.c_int64),
                ("out_rows", ctypes.c_int64)]


def _bind(e):
    fn = e.lib.ldm_dev_attnout_run
    fn.argtypes, fn.restype = [VP, ctypes.POINTER(Io)], ctypes.c_int
    return e


@pytest.fixture(scope="module")
def engines():
    """One engine per (mode, d_ff), built on first use"""
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
            cache[(mode, d_ff)] = _bind(e)
        return cache[(mode, d_ff)]

    yield get
    for e in cache.values():
        e.close()


MEASURED = {}   # family -> {case id: (error, bar)}, printed by the last test


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint16, np.float16):
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _buffers(case, in_place=False):
    """-> (io, tensors): panels of exactly the launch's reach, res of exactly B S rows, the output 3 rows and a tail longer, NaN-filled"""
    op, M, rows = AC.operands(case), case.M, case.panel_rows
    hi, lo = AC.pack_qkv_panels(op.q, op.k, op.v, rows)
    out = np.full((M + 3) * D + TAIL, AC.NAN32, np.uint32)
    if in_place:
        out[: M * D] = op.res.view(np.uint32).reshape(-1)
    t = dict(hi=_dev(hi), lo=_dev(lo), out=_dev(out))
    t["res"] = t["out"] if in_place else _dev(op.res)
    io = Io(layer=case.layer, B=case.B, S=case.S, qkv_hi=t["hi"].data_ptr(), qkv_lo=t["lo"].data_ptr(), panel_stride=rows * 64,
            res=t["res"].data_ptr(), out=t["out"].data_ptr(), panel_rows=rows, res_rows=M, out_rows=M + 3)
    return io, t


def run_launch(e, case, in_place=False):
    """The launch of `case` on engine e -> (out [M, 464] float32, guards: a list of (name, ok))"""
    op, M = AC.operands(case), case.M
    io, t = _buffers(case, in_place)
    torch.cuda.synchronize()
    rc = e.lib.ldm_dev_attnout_run(e._h, ctypes.byref(io))
    if rc == -2:    # a HIP error: nothing more runs on this device from this module
        pytest.exit(f"{case.id}: {e.lib.ldm_last_error(e._h).decode()}", returncode=3)
    assert rc == 0, (case.id, rc, e.lib.ldm_last_error(e._h).decode())
    ob = t["out"].cpu().numpy().view(np.uint32)
    guards = [("rows >= B S", bool((ob[M * D: (M + 3) * D] == AC.NAN32).all())), ("tail", bool((ob[(M + 3) * D:] == AC.NAN32).all()))]
    if not in_place:
        guards.append(("res unchanged", bool(np.array_equal(t["res"].cpu().numpy().view(np.uint32), op.res.view(np.uint32)))))
        assert t["out"].data_ptr() != t["res"].data_ptr()
    return ob[: M * D].reshape(M, D).view(np.float32), guards


def check(case, out, guards, note="", ref=None, record=True):
    """Every figure printed before it is asserted; returns the launch's error."""
    res = AC.operands(case).res
    ref = AC.reference(case) if ref is None else ref
    bar = AC.bar(case)
    nan = int(np.isnan(out).sum())
    err = AC.rel_err(np.nan_to_num(out), ref, res)
    r, c = AC.worst_location(np.nan_to_num(out), ref)
    bad = [n for n, ok in guards if not ok]
    print(f"{case.id:38s} <{','.join(str(int(x)) for x in case.instantiation)}> err {err:.2e} (bar {bar:.2e}, emulation {AC.figures(case)['emu']:.2e}) at layout "
          f"{r // case.S} row {r % case.S} (wave {r % case.S // 32}) col {c} (tile {c // 32}){note}" + (f"  NaN: {nan}" if nan else "")
          + (f"  GUARDS TOUCHED: {bad}" if bad else ""), flush=True)
    if record:
        MEASURED.setdefault(case.family, {})[case.id] = (err, bar)
    assert not bad, bad
    assert nan == 0
    assert err <= bar, (case.id, err, bar, (r, c))
    return err


RAN = set()


def _case_test(engines, case):
    e = engines(case.mode, case.d_ff)
    d = e.describe()
    assert d["precision"] == LC.MODES[case.mode].precision + "_f16"
    out, guards = run_launch(e, case)
    check(case, out, guards)
    RAN.add(case.instantiation)
    return out


FORM_CASES, S_CASES, SCORE_CASES, DFF_CASES = AC.form_cases(), AC.s_edge_cases(), AC.score_cases(), AC.dff_cases()


@pytest.mark.parametrize("case", FORM_CASES, ids=[c.id for c in FORM_CASES])
def test_every_instantiation_against_float64(engines, case):
    _case_test(engines, case)


def test_the_cases_ran_reach_the_three_instantiations():
    assert RAN == AC.INSTANTIATIONS, sorted(AC.INSTANTIATIONS - RAN)


@pytest.mark.parametrize("case", S_CASES, ids=[c.id for c in S_CASES])
def test_sequence_lengths_around_the_wave_and_key_tile_edges(engines, case):
    _case_test(engines, case)


@pytest.mark.parametrize("case", SCORE_CASES, ids=[c.id for c in SCORE_CASES])
def test_score_range(engines, case):
    out = _case_test(engines, case)
    if case.kind == "q0":      # P = 1 / S exactly: the block is the mean of V through Wo, no softmax in the reference
        check(case, out, [], note="  (against the mean of V)", ref=AC.mean_of_v(case), record=False)


@pytest.mark.parametrize("case", DFF_CASES, ids=[c.id for c in DFF_CASES])
def test_ffn_geometries(engines, case):
    assert engines(case.mode, case.d_ff).cfg.d_ff == case.d_ff
    _case_test(engines, case)


def test_ffn_in_place_is_ffn_out_of_place(engines):
    """The product's own use: a.res = a.ffn_out = ws.P"""
    case = AC.IN_PLACE
    e = engines(case.mode)
    a, ga = run_launch(e, case)
    b, gb = run_launch(e, case, in_place=True)
    check(case, a, ga)
    check(case, b, gb, note="  (in place)", record=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_hook_refuses_what_the_kernel_does_not_take(engines):
    case = AC.Case("mixed", B=2, S=33, layer=1, seed=33)
    e = engines("mixed")
    M, rows = case.M, case.panel_rows

    def refused(handle=e, **kw):
        io, t = _buffers(case)
        for k, v in kw.items():
            setattr(io, k, v(io) if callable(v) else v)
        torch.cuda.synchronize()
        rc = handle.lib.ldm_dev_attnout_run(handle._h, ctypes.byref(io))
        untouched = bool((t["out"].cpu().numpy().view(np.uint32) == AC.NAN32).all())
        print(f"refusal {sorted(kw) or ['handle']}: rc {rc}, output untouched {untouched}: {handle.lib.ldm_last_error(handle._h).decode()}")
        return rc == -1 and untouched

    out, guards = run_launch(e, case)          # (the same buffers are accepted as they stand)
    check(case, out, guards, record=False)
    assert refused(S=0) and refused(S=129) and refused(B=0) and refused(B=2 ** 31 - 1, S=128)
    assert refused(layer=-1) and refused(layer=AC.N_LAYER)
    assert refused(panel_rows=rows - 1)                                     # panels shorter than the last layout's 128-row reach
    assert refused(panel_stride=rows * 64 - 16) and refused(panel_stride=rows * 64 + 8)
    assert refused(out_rows=M - 1) and refused(res_rows=M - 1)
    for p in ("qkv_hi", "qkv_lo", "res", "out"):
        assert refused(**{p: lambda io, p=p: getattr(io, p) + 4}), p        # not 16-byte aligned
        assert refused(**{p: None}), p
    # a handle without the kernel: split with LDM_X3_ATTNOUT off (mixed / hybrid do not exist without it: ldm_create refuses them)
    assert refused(handle=engines("split_qkv32"))
    from layout_dm_amd.binding import Engine

    with pytest.MonkeyPatch.context() as mp:
        for k, v in LC.MODES["split_qkv32"].env:
            mp.setenv(k, v)
        with pytest.raises(RuntimeError, match="two-product kernels"):
            Engine(n_category=25, precision="mixed", max_batch=4)


def test_print_the_measured_table():
    """(last: what profiles/attnout_alone_check.txt holds)"""
    print("\nfamily                  cases   measured               bar                    closest to its bar")
    for fam in sorted(MEASURED):
        m = MEASURED[fam]
        errs, bars = [v[0] for v in m.values()], [v[1] for v in m.values()]
        near = max(m, key=lambda k: m[k][0] / m[k][1])
        print(f"{fam:22s}  {len(m):5d}   {min(errs):.2e} .. {max(errs):.2e}   {min(bars):.2e} .. {max(bars):.2e}   {near} ({m[near][0]:.2e} of {m[near][1]:.2e}: "
              f"{m[near][0] / m[near][1]:.2f})")
    assert MEASURED
