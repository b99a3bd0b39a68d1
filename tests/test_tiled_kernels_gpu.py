"""GPU: ONE launch of each kernel of the tiled engines (layout_dm_amd/csrc/ldm_denoise.cpp denoise_chunk_tiled / denoise_chunk_fast) on the
test's buffers — launch_layernorm, launch_gemm, launch_gemm16x3, launch_gemm16, launch_attention, launch_attention16 through the development
hooks ldm_dev_layernorm_run / ldm_dev_gemm_run / ldm_dev_attention_run (csrc/ldm_dev.cpp) — against the float64 reference of that launch
(tests/_tiled_cases.py).  No engine is created.  The logits of a whole pass are held to 1e-5 .. 2e-3 on five or six geometries; a lo term
dropped in one k-step, a skipped K tile or one wrong column tile fits under that.  tests/test_tiled_reference.py pins cases, yardsticks and bars.

  * every output buffer is larger than the launch needs and pre-filled with a NaN pattern: rows >= M, columns N .. ld and the bytes behind the
    last row come back bit for bit, and no element inside [M, N] keeps the pattern or holds a NaN;
  * operand buffers of the fp16 GEMMs are allocated exactly to whole tiles, the rows past M / N hold large finite values;
  * hi / lo outputs: hi + lo against the reference, hi alone against fp16(reference) within one ulp;
  * LayerNorm in place (y32 == x, the tiled pass's use of its P buffer) == out of place, bit for bit; exact zeros in the padding columns of
    the head-padded attention output.

Bars (none is taken from the device): min(4 x the distance of the CPU emulation of the case from float64, 1e-2 x the case's smallest
yardstick) for the exact and fp16 x 3 kernels and LayerNorm; 3 x the emulation's distance for the fp16-product kernels.

Measured on the MI355X, max |out - ref| / max |ref| (the printed table: profiles/tiled_alone_check.txt):

  family                              cases   measured             bar (all: the emulation term binds; 1e-2 x the smallest yardstick is >= 1.4e-6)
  gemm_f32_tile<2>                       81   6.9e-8 .. 7.6e-7     2.0e-7 .. 2.4e-6   (80 shapes + the wrapping persistent loop: 1 640 tiles at 256 CUs)
  gemm16x3_k 256 x 256, 2 stages         38   5.5e-8 .. 4.3e-7     2.8e-7 .. 1.5e-6   (tags 0 .. 3)
  gemm16x3_k 256 x 128, 3 stages         35   6.9e-8 .. 6.1e-7     2.7e-7 .. 1.2e-6   (tag 4)
  gemm16_k, C32 out                      15   9.9e-8 .. 3.0e-7     1.7e-7 .. 6.7e-7   (3 x emulation)
  gemm16_k, C16 out                      18   2.5e-4 .. 3.8e-4     7.6e-4 .. 1.1e-3   (3 x emulation: its own fp16 rounding)
  attention16x3                          10   0 .. 5.9e-7          2.7e-7 .. 2.6e-6
  attn32_direct_k                         4   4.0e-7 .. 1.2e-6     1.8e-6 .. 2.8e-6
  attn32_mfma_k, fp32 | hi / lo out   2 + 2   4.1e-7 .. 1.0e-6     1.9e-6 .. 3.6e-6   (first run)
  attn_rows<float,32>, both outs      4 + 4   0 .. 7.8e-7          0 .. 3.3e-6        (first run; S = 1: bit for bit)
  attn_rows<float,60>, both outs      7 + 3   0 .. 8.7e-7          0 .. 3.7e-6        (head dim 36: first run)
  attn_rows<float,64>, both outs      4 + 4   2.8e-7 .. 1.0e-6     1.1e-6 .. 3.7e-6
  attn_mfma_k (attention16)              12   0 .. 5.0e-4          0 .. 1.5e-3        (3 x emulation; S = 1: bit for bit)
  ln_rows<1> | <2> | <4>       20 | 24 | 19   0 .. 1.8e-7          1.0e-7 .. 8.6e-7   (<4>: first run)
  ln_rows, raw + statistics       3 | 4 | 3   4.3e-8 .. 4.8e-7     1.7e-7 .. 1.9e-6   (y32 = emb + pos bit for bit)

Closest to a bar: gemm16-t2-M1-N155-K128-bias_res 1.37e-7 of 1.73e-7, x3-t0-M256-N464-K96-bias 3.79e-7 of 5.09e-7, exact-t0-M1-N464-K48-nobias 3.28e-7
of 4.66e-7; the values are bit-repeatable (seeded operands, deterministic kernels).  No case exposed a fault: the four instantiations that ran
for the first time (attn32_mfma_k, attn_rows<float,32>, attn_rows<float,60> at head dim 36, ln_rows<4>) are inside their bars.

Mutation check, by hand: with the Alo x Whi MFMA of gemm16x3_k removed in every k-step all 73 gemm16x3 cases fail at 1.4e-4 .. 2.7e-4 (140 .. 920 x
their bars) while the logits of a whole split pass through gemm16x3_k (LDM_X3_LNGEMM=0 LDM_X3_ATTNOUT=0) measure 2.4e-4; removed in one k-step
(kt 1, ks 0) the 61 cases with K >= 64 fail at 2.4e-5 .. 1.6e-4 (24 .. 340 x) and the whole pass measures 7.2e-5 (unmutated: 6.4e-7) — inside the 1e-3
of the mixed / hybrid / fast passes, 1.4 x over the split pass's own 5e-5.
"""
import ctypes

import numpy as np
import pytest
import torch

import _tiled_cases as TC

pytestmark = pytest.mark.gpu

VP, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
F4, F8 = np.float32, np.float64


class LnIo(ctypes.Structure):      # csrc/ldm_dev.cpp ldm_dev_layernorm_io
    _fields_ = [(n, VP) for n in ("x", "tokens", "emb", "pos", "p0", "p1", "y32", "y16", "y16lo", "stats_out")] + \
               [(n, I32) for n in ("M", "D", "S", "ld16", "ada", "raw")] + \
               [(n, I64) for n in ("x_rows", "n_tokens", "emb_rows", "pos_rows", "n_p", "y32_rows", "y16_rows", "stats_rows")]


class GemmIo(ctypes.Structure):    # ldm_dev_gemm_io
    _fields_ = [(n, VP) for n in ("A", "Alo", "W", "Wlo", "bias", "res", "C32", "C16", "C16lo")] + \
               [(n, I32) for n in ("M", "N", "K", "lda", "ldw", "ldres", "ldc32", "ldc16", "relu", "tag", "kind")] + [("out_scale", ctypes.c_float)] + \
               [(n, I64) for n in ("a_rows", "w_rows", "n_bias", "res_rows", "c32_rows", "c16_rows")]


class AttnIo(ctypes.Structure):    # ldm_dev_attention_io
    _fields_ = [(n, VP) for n in ("qkv", "out32", "out16", "out16lo")] + \
               [(n, I32) for n in ("in_f16", "B", "S", "H", "dh", "D", "ld", "ldo32", "ldo16", "kind")] + \
               [(n, I64) for n in ("qkv_rows", "out32_rows", "out16_rows")]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from layout_dm_amd import binding

    L = binding.load_library()
    for fn, io in ((L.ldm_dev_layernorm_run, LnIo), (L.ldm_dev_gemm_run, GemmIo), (L.ldm_dev_attention_run, AttnIo)):
        fn.argtypes, fn.restype = [ctypes.POINTER(io)], ctypes.c_int
    torch.cuda.set_device(0)
    return L


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint16, np.float16):
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def padded(a, ld):
    """[rows, n] -> [rows, ld] with zeros behind the columns"""
    out = np.zeros((a.shape[0], ld), a.dtype)
    out[:, :a.shape[1]] = a
    return out


class Guarded:
    """An output buffer of `rows` + 3 rows of ld elements and 64 more behind them, filled with a NaN pattern"""
    EXTRA, TAIL = 3, 64

    def __init__(self, rows, ld, bits, init=None):
        self.rows, self.ld = rows, ld
        self.dtype, self.fill = (np.uint32, TC.NAN32) if bits == 32 else (np.uint16, TC.NAN16)
        h = np.full((rows + self.EXTRA) * ld + self.TAIL, self.fill, self.dtype)
        if init is not None:        # (rows that the launch reads and overwrites in place)
            h[:rows * ld].reshape(rows, ld)[:, :init.shape[1]] = init.view(self.dtype)
        self.t = _dev(h)

    @property
    def ptr(self):
        return self.t.data_ptr()

    @property
    def cap_rows(self):
        return self.rows + self.EXTRA

    def read(self, name, n_cols):
        """-> (values [rows, n_cols] as float32 / float16, [(guard, ok)])"""
        b = self.t.cpu().numpy().view(self.dtype)
        body = b[:(self.rows + self.EXTRA) * self.ld].reshape(-1, self.ld)
        vals = body[:self.rows, :n_cols].view(F4 if self.dtype == np.uint32 else np.float16)
        guards = [(f"{name} rows >= M", bool((body[self.rows:] == self.fill).all())),
                  (f"{name} columns >= N", bool((body[:self.rows, n_cols:] == self.fill).all())),
                  (f"{name} bytes behind the last row", bool((b[(self.rows + self.EXTRA) * self.ld:] == self.fill).all())),
                  (f"{name} every element written", bool((body[:self.rows, :n_cols] != self.fill).all() and not np.isnan(vals).any()))]
        return vals, guards


def call(lib, fn, io, cid):
    torch.cuda.synchronize()
    rc = fn(ctypes.byref(io))
    if rc == -2:    # a HIP error: nothing more runs on this device from this module
        pytest.exit(f"{cid}: HIP error", returncode=3)
    assert rc == 0, (cid, rc)


MEASURED = {}   # family -> {case id: (error, bar, the term that binds)}
RAN = set()


def record(family, cid, err, bar, binds, inst):
    MEASURED.setdefault(family, {})[cid] = (err, bar, binds)
    RAN.add(inst)


def finish(cid, inst, err, bar, binds, guards, extra_ok=True, note=""):
    """Every figure printed before it is asserted"""
    bad = [n for n, ok in guards if not ok]
    print(f"{cid:46s} {inst:34s} err {err:.2e} (bar {bar:.2e}, {binds}){note}" + (f"  GUARDS TOUCHED: {bad}" if bad else "") +
          ("" if extra_ok else "  HI / ZERO CHECK FAILED"), flush=True)
    assert not bad, bad
    assert extra_ok
    assert err <= bar, (cid, err, bar)


def hi_lo_err(hi, lo, ref, mag):
    """hi + lo against the reference, beyond what the two-half format itself loses"""
    d = np.abs(hi.astype(F8) + lo.astype(F8) - ref) - TC.hi_lo_slack(ref)
    return float(max(d.max(), 0.0) / mag)


# ================================================================================================================ GEMM
def run_gemm(lib, c, figures=None):
    op = TC.gemm_operands(c)
    bias, relu, res, c32, c16, c16lo = TC.FORMS[c.form]
    io = GemmIo(M=c.M, N=c.N, K=c.K, lda=c.lda, ldw=c.ldw, ldres=c.ldres, ldc32=c.ldc, ldc16=c.ldc, relu=relu, tag=c.tag, kind=c.kind,
                out_scale=op.scale if c.kind == TC.X3 else 0.0, a_rows=c.a_rows, w_rows=c.w_rows)
    keep = []

    def dev(a):
        keep.append(_dev(a))
        return keep[-1].data_ptr()

    if c.kind == TC.EXACT:
        io.A, io.W = dev(padded(op.A, c.lda)), dev(padded(op.W, c.ldw))
    else:
        io.A, io.W = dev(padded(op.A_hi, c.lda)), dev(padded(op.W_hi, c.ldw))
        if c.kind == TC.X3:
            io.Alo, io.Wlo = dev(padded(op.A_lo, c.lda)), dev(padded(op.W_lo, c.ldw))
    if bias:
        io.bias, io.n_bias = dev(op.bias), c.N
    if res:
        io.res, io.res_rows = dev(padded(op.res, c.ldres)), c.M
    outs = {}
    for name, on, bits in (("C32", c32, 32), ("C16", c16, 16), ("C16lo", c16lo, 16)):
        if on:
            outs[name] = Guarded(c.M, c.ldc, bits)
            setattr(io, name, outs[name].ptr)
    io.c32_rows = io.c16_rows = c.M + Guarded.EXTRA
    call(lib, lib.ldm_dev_gemm_run, io, c.id)
    ref, mag = TC.gemm_reference(c)
    bar, emu, ys, binds = figures or TC.gemm_figures(c)
    got, guards = {}, []
    for name, g in outs.items():
        got[name], gs = g.read(name, c.N)
        guards += gs
    err, ok = 0.0, True
    if c32:
        err = TC.rel_err(got["C32"], ref, mag)
    if c16 and c16lo:
        err = max(err, hi_lo_err(got["C16"], got["C16lo"], ref, mag))
        ok = TC.hi_within_one_ulp(got["C16"], ref, bar * mag)
    elif c16:
        err = max(err, TC.rel_err(got["C16"], ref, mag))
    fam = {TC.EXACT: "gemm_f32_tile<2>", TC.X3: "gemm16x3_k 256x256 / 2 stages" if c.tag != 4 else "gemm16x3_k 256x128 / 3 stages",
           TC.F16: "gemm16_k, C16 out" if not c32 else "gemm16_k, C32 out"}[c.kind]
    record(fam, c.id, err, bar, binds, c.instantiation)
    finish(c.id, c.instantiation, err, bar, binds, guards, ok)
    return got


GEMM_CASES = TC.exact_gemm_cases() + TC.x3_gemm_cases() + TC.f16_gemm_cases()


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c.id for c in GEMM_CASES])
def test_gemm_against_float64(lib, case):
    run_gemm(lib, case)


def test_exact_gemm_persistent_loop_wraps(lib):
    """More tiles than the grid: a workgroup walks tiles w, w + grid, ... (launch_gemm: at most 5 per CU)"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = TC.exact_wrap_case(n_cu)
    assert c.n_tiles > 6 * n_cu
    run_gemm(lib, c, figures=TC.gemm_figures(c, 8))


# ================================================================================================================ attention
def run_attention(lib, c):
    q, k, v = TC.attention_operands(c)
    rows = TC.attention_rows(c, q, k, v)
    M = TC.B_LAYOUTS * c.S
    qkv = _dev(rows)
    io = AttnIo(qkv=qkv.data_ptr(), in_f16=int(c.f16), B=TC.B_LAYOUTS, S=c.S, H=c.H, dh=c.dh, D=c.D, ld=rows.shape[1], ldo32=c.D, ldo16=c.ldo16,
                kind=int(c.f16), qkv_rows=M)
    outs = {}
    if c.f16:
        outs["out16"] = Guarded(M, c.ldo16, 16)
    elif c.split:        # attention_out_proj, split: hi / lo out, out32 null
        outs["out16"], outs["out16lo"] = Guarded(M, c.ldo16, 16), Guarded(M, c.ldo16, 16)
    else:                # attention_out_proj, exact: out32 only (ldo16 is passed all the same)
        outs["out32"] = Guarded(M, c.D, 32)
    for name, g in outs.items():
        setattr(io, name, g.ptr)
    io.out32_rows = io.out16_rows = M + Guarded.EXTRA
    call(lib, lib.ldm_dev_attention_run, io, c.id)
    ref, mag = TC.attention_reference(c)
    bar, emu, ys, binds = TC.attention_figures(c)
    n_cols = c.H * 64 if c.f16 else c.D
    got, guards = {}, []
    for name, g in outs.items():
        got[name], gs = g.read(name, n_cols)
        guards += gs
    ok = True
    if c.f16:
        o, pad = TC.attention_heads(c, got["out16"])
        err = TC.rel_err(o, ref, mag)
        ok = pad is None or bool((pad == 0).all())      # exact zeros in the head padding
    elif c.split:
        hi, lo = TC.attention_heads(c, got["out16"])[0], TC.attention_heads(c, got["out16lo"])[0]
        err = hi_lo_err(hi, lo, ref, mag)
        ok = TC.hi_within_one_ulp(hi, ref, bar * mag)
    else:
        err = TC.rel_err(TC.attention_heads(c, got["out32"])[0], ref, mag)
    fam = c.kernel + (", hi / lo out" if c.split and c.kernel != "attention16x3" else "")
    record(fam, c.id, err, bar, binds, c.kernel)
    finish(c.id, c.kernel, err, bar, binds, guards, ok)


ATTN_KNOWN = [c for c in TC.attention_cases() if not c.first_run]
ATTN_FIRST = [c for c in TC.attention_cases() if c.first_run]


@pytest.mark.parametrize("case", ATTN_KNOWN, ids=[c.id for c in ATTN_KNOWN])
def test_attention_against_float64(lib, case):
    run_attention(lib, case)


@pytest.mark.parametrize("case", TC.attention16_cases(), ids=[c.id for c in TC.attention16_cases()])
def test_attention16_against_float64(lib, case):
    run_attention(lib, case)


# ================================================================================================================ LayerNorm
def run_layernorm(lib, c, in_place=False):
    op = TC.layernorm_operands(c)
    M, D = c.M, c.D
    gathered = "tokens" in op
    io = LnIo(M=M, D=D, S=TC.LN_S, ld16=c.ld16, ada=int(c.form in ("ada", "gather")), raw=int(c.form == "raw"), n_p=D)
    keep = []

    def dev(a):
        keep.append(_dev(a))
        return keep[-1].data_ptr()

    if gathered:
        io.tokens, io.emb, io.pos = dev(op["tokens"]), dev(op["emb"]), dev(op["pos"])
        io.n_tokens, io.emb_rows, io.pos_rows = M, TC.LN_CLASSES, TC.LN_S
    io.p0, io.p1 = dev(op["p0"]), dev(op["p1"])
    outs = {}
    want32 = c.outs != "y16" or c.form == "raw"
    if want32:
        outs["y32"] = Guarded(M, D, 32, init=op["x"] if in_place else None)
    if "y16" in c.outs and c.form != "raw":
        outs["y16"] = Guarded(M, c.ld16, 16)
        if c.outs == "y32_y16_lo":
            outs["y16lo"] = Guarded(M, c.ld16, 16)
    if c.form == "raw":
        outs["stats_out"] = Guarded(M, 2, 32)
    for name, g in outs.items():
        setattr(io, name, g.ptr)
    io.y32_rows = io.y16_rows = io.stats_rows = M + Guarded.EXTRA
    if not gathered:
        if in_place:
            io.x, io.x_rows = outs["y32"].ptr, M + Guarded.EXTRA
        else:
            io.x, io.x_rows = dev(op["x"]), M
    call(lib, lib.ldm_dev_layernorm_run, io, c.id)
    got, guards = {}, []
    for name, g in outs.items():
        got[name], gs = g.read(name, 2 if name == "stats_out" else D)
        guards += gs
    return got, guards


def check_layernorm(c, got, guards, note=""):
    y, st, mag = TC.layernorm_reference(c)
    bar, emu, ys, binds, bar_stats = TC.layernorm_figures(c)
    err, ok = 0.0, True
    if c.form == "raw":
        op = TC.layernorm_operands(c)
        ok = np.array_equal(got["y32"], op["emb"][op["tokens"]] + op["pos"][np.arange(c.M) % TC.LN_S])       # one fp32 addition: bit for bit
        err = TC.stats_err(got["stats_out"], st)
    else:
        if "y32" in got:
            err = TC.rel_err(got["y32"], y, mag)
        if "y16lo" in got:
            err = max(err, hi_lo_err(got["y16"], got["y16lo"], y, mag))
        if "y16" in got:
            ok = TC.hi_within_one_ulp(got["y16"], y, bar * mag)
            if len(got) == 1:       # fp16 out alone: what exceeds its own rounding 2^-11 |ref| is held to the bar
                err = float(np.maximum(np.abs(got["y16"].astype(F8) - y) - 2.0 ** -11 * np.abs(y), 0.0).max() / mag)
            if "y32" in got:
                ok = ok and np.array_equal(got["y16"], got["y32"].astype(np.float16))      # y16 IS fp16(y32)
    inst = f"ln_rows<{c.nv}>"
    record(inst + (", raw + statistics" if c.form == "raw" else ""), c.id + note, err, bar, binds, inst)
    finish(c.id, inst, err, bar, binds, guards, ok, note)


LN_KNOWN = [c for c in TC.layernorm_cases() if not c.first_run]
LN_FIRST = [c for c in TC.layernorm_cases() if c.first_run]


@pytest.mark.parametrize("case", LN_KNOWN, ids=[c.id for c in LN_KNOWN])
def test_layernorm_against_float64(lib, case):
    check_layernorm(case, *run_layernorm(lib, case))


@pytest.mark.parametrize("D", [464, 256])
def test_layernorm_in_place_is_out_of_place(lib, D):
    """The tiled pass's own use: a.x = a.y32 = ws.P"""
    c = TC.LnCase(D, 129, "ada", "y32_y16_lo", edge=True)
    a, ga = run_layernorm(lib, c)
    b, gb = run_layernorm(lib, c, in_place=True)
    check_layernorm(c, a, ga)
    check_layernorm(c, b, gb, note="  (in place)")
    for k in ("y32", "y16", "y16lo"):
        assert np.array_equal(a[k].view(np.uint32 if k == "y32" else np.uint16), b[k].view(np.uint32 if k == "y32" else np.uint16)), k


# ================================================================================================================ refusals
def test_the_hooks_refuse_what_the_kernels_forbid(lib):
    """-1 before any launch: the pointers are real, only the stated precondition is broken"""
    buf = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    w, o = p + (1 << 20), p + (1 << 21)      # a second operand and the output: 1 MiB apart

    def gemm(**kw):
        d = dict(A=p, W=w, C32=o, M=8, N=8, K=64, lda=64, ldw=64, ldc32=8, kind=0, a_rows=8, w_rows=8, c32_rows=8)
        d.update(kw)
        return lib.ldm_dev_gemm_run(ctypes.byref(GemmIo(**d)))

    assert gemm(K=24, lda=24, ldw=24) == -1 and gemm(lda=66) == -1 and gemm(A=p + 4) == -1 and gemm(a_rows=7) == -1 and gemm(c32_rows=7) == -1
    assert gemm(out_scale=0.125) == -1 and gemm(ldc32=4) == -1 and gemm(C32=None) == -1
    x3 = dict(kind=1, Alo=p, Wlo=p, a_rows=256, w_rows=256, out_scale=0.125)
    assert gemm(**{**x3, "K": 48, "lda": 48, "ldw": 48}) == -1 and gemm(**{**x3, "a_rows": 255}) == -1 and gemm(**{**x3, "w_rows": 128}) == -1
    assert gemm(**{**x3, "Alo": None}) == -1 and gemm(**{**x3, "lda": 68}) == -1 and gemm(**{**x3, "C32": o + 8}) == -1 and gemm(**{**x3, "tag": 5}) == -1
    f16 = dict(kind=2, a_rows=128, w_rows=128)
    assert gemm(**{**f16, "K": 96, "lda": 96, "ldw": 96}) == -1 and gemm(**{**f16, "a_rows": 127}) == -1 and gemm(**{**f16, "C16lo": p, "C16": p}) == -1

    def ln(**kw):
        d = dict(x=p, p0=w, p1=w, y32=o, M=4, D=16, S=1, n_p=16, x_rows=4, y32_rows=4)
        d.update(kw)
        return lib.ldm_dev_layernorm_run(ctypes.byref(LnIo(**d)))

    assert ln(D=18, n_p=18) == -1 and ln(D=1028, n_p=1028) == -1 and ln(x=p + 4) == -1 and ln(x_rows=3) == -1 and ln(y32_rows=3) == -1
    assert ln(n_p=12) == -1 and ln(y32=None) == -1 and ln(y16=p, ld16=18, y16_rows=4) == -1 and ln(y16lo=p) == -1 and ln(raw=1, y32=None) == -1

    def attn(**kw):
        d = dict(qkv=p, out32=o, B=1, S=8, H=2, dh=16, D=32, ld=96, ldo32=32, qkv_rows=8, out32_rows=8)
        d.update(kw)
        return lib.ldm_dev_attention_run(ctypes.byref(AttnIo(**d)))

    assert attn(dh=65, D=130, ld=390, ldo32=130) == -1 and attn(S=0) == -1 and attn(D=30) == -1 and attn(ld=64) == -1 and attn(qkv_rows=7) == -1
    assert attn(S=400, dh=64, D=128, ld=384, ldo32=128, qkv_rows=400, out32_rows=400) == -1      # 2 x 400 x 64 floats > 160 KiB of LDS
    assert attn(out32=None) == -1 and attn(out16lo=p) == -1 and attn(out32_rows=7) == -1
    a16 = dict(kind=1, in_f16=1, out32=None, out16=o, H=2, ld=384, ldo16=128, out16_rows=8)
    assert attn(**{**a16, "S": 129, "qkv_rows": 129, "out16_rows": 129}) == -1 and attn(**{**a16, "ld": 380}) == -1 and attn(**{**a16, "in_f16": 0}) == -1
    assert attn(**{**a16, "ldo16": 120}) == -1 and attn(**a16) == 0 and gemm() == 0 and ln() == 0      # (and the unbroken arguments run)


# ================================================================================================================ first runs
# Instantiations no test of a whole pass reaches — attn32_mfma_k (head dim 57), attn_rows<float, 32>, attn_rows<float, 60> at head dim 36,
# ln_rows<4> (d_model > 512) — behind everything the product already exercises.
@pytest.mark.parametrize("case", LN_FIRST, ids=[c.id for c in LN_FIRST])
def test_layernorm_wide_rows_against_float64(lib, case):
    check_layernorm(case, *run_layernorm(lib, case))


@pytest.mark.parametrize("case", ATTN_FIRST, ids=[c.id for c in ATTN_FIRST])
def test_attention_first_runs_against_float64(lib, case):
    run_attention(lib, case)


def test_the_cases_ran_reach_all_21_instantiations():
    assert RAN == TC.ALL_INSTANTIATIONS, sorted(TC.ALL_INSTANTIATIONS ^ RAN)


def test_print_the_measured_table():
    """(last: what profiles/tiled_alone_check.txt holds)"""
    print("\nfamily                                  cases   measured               bar                    binds")
    for fam in sorted(MEASURED):
        m = MEASURED[fam]
        errs, bars = [v[0] for v in m.values()], [v[1] for v in m.values()]
        binds = sorted({v[2] for v in m.values()})
        worst = max(m, key=lambda k: m[k][0] / m[k][1] if m[k][1] else 0.0)
        print(f"{fam:38s}  {len(m):5d}   {min(errs):.1e} .. {max(errs):.1e}   {min(bars):.1e} .. {max(bars):.1e}   {' | '.join(binds)}"
              f"   closest to its bar: {worst} ({m[worst][0]:.2e} of {m[worst][1]:.2e})")
    assert MEASURED
