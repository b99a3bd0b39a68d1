"""Shared by tests/test_lngemm_reference.py (CPU) and tests/test_lngemm_gpu.py (device): ONE launch of the row-resident LayerNorm + GEMM
kernel (layout_dm_amd/csrc/kernels_lngemm.hip lngemm16x3_k) — the cases, their seeded operands, the float64 reference of the launch, wrong
references on the same operands (the yardsticks: what a dropped lo term, a missing k16-step, exchanged rows or a shifted tile would give), a
float32 emulation of the kernel's arithmetic, and the unpackers of its output layouts.  numpy only.

A launch:   x   = the rows | emb[token] + pos[row % S] | res + b2 + hid · W2^T      (linear2 of the layer in front as the GEMM prologue)
            y   = LayerNorm(x), eps 1e-5, times (1 + scale) plus shift (AdaLN row of (t, layer)) | gamma, beta
            out = y · W^T + bias, ReLU behind linear1
(CategoricalTransformer.forward / Block.forward of the reference: oracle/restatement.py denoiser_logits restates them.)"""
import dataclasses
import functools

import numpy as np

from oracle import spec as SP
from oracle import synth

D, S, EPS = 464, 125, 1e-5
NAN32, NAN16 = 0x7FC01234, 0x7E55          # guard-band fill: quiet NaNs with a payload
IN_PROJ, LINEAR1, HEAD = 0, 1, 2
LAUNCH_NAMES = ("in_proj", "linear1", "head")

# ---------------------------------------------------------------------------------------------------------------- modes
# What ldm_create derives from (precision, knobs): products per k16-step of the attention path's GEMM (in_proj) and of linear1 / linear2 / the
# head, whether q / k / v leave in_proj as head-padded panels, and whether the block's FFN has launches of its own.


@dataclasses.dataclass(frozen=True)
class Mode:
    name: str
    precision: str
    env: tuple            # development knobs the engine is created under
    np_w: int
    np_ffn: int
    qkv_panels: bool = True
    ffn_launches: bool = True
    point: str = "mid"    # the weights: oracle.synth "perturb" (synth_state_dict(perturb=True)) | trained-like "mid"


MODES = {m.name: m for m in (
    Mode("split", "split", (), 3, 3, point="perturb"),
    Mode("mixed", "mixed", (), 2, 2, point="mid"),
    Mode("hybrid", "hybrid", (), 2, 1, ffn_launches=False, point="mid"),
    Mode("hybrid_two_launch", "hybrid", (("LDM_DEV", "1"), ("LDM_HYB_FFN", "0")), 2, 1, point="mid"),
    Mode("split_qkv32", "split", (("LDM_DEV", "1"), ("LDM_X3_ATTNOUT", "0")), 3, 3, qkv_panels=False, point="perturb"),
)}
# Which weights: the "mid" point scales 4 output channels of every linear2 by 8, and make_w16 pre-scales a TENSOR by one power of two — the lo
# halves of the ordinary rows then sit in fp16's denormal range (spacing 2^-24 of the scaled weight, up to 1e-6 of a weight of typical size).
# hi + lo of such a linear2 is the fp32 weight to 5e-7 only: the emulation below (no kernel involved) is 4.7e-7 .. 6.4e-7 away from the float64
# reference for the three-product in_proj behind layer 0's linear2, against 1.5e-7 .. 3e-7 everywhere else — a floor of the weight FORMAT, above
# a quarter of any bar that stays two orders of magnitude under a dropped lo term.  A test of the launch's arithmetic keeps it out of the way:
# the three-product engines run the "perturb" weights, the two- and one-product engines — whose specified weight IS fp16(W 2^k) / 2^k, lo halves
# play no part — the "mid" point.

# the 14 instantiations <ADA, OUT, PRE, NPM, NPP> launch_lngemm16x3 lists above its dispatch (kernels_lngemm.hip)
INSTANTIATIONS = frozenset({
    (1, 2, 0, 3, 3), (1, 2, 1, 3, 3), (1, 0, 0, 3, 3), (1, 0, 1, 3, 3), (0, 1, 0, 3, 3), (0, 0, 1, 3, 3),       # split
    (1, 2, 0, 2, 2), (1, 2, 1, 2, 2), (0, 1, 0, 2, 2), (0, 0, 1, 2, 2),                                         # mixed
    (1, 2, 1, 2, 1), (0, 3, 0, 1, 1), (0, 0, 1, 1, 1), (0, 0, 0, 1, 1),                                         # hybrid
})


@dataclasses.dataclass(frozen=True)
class Case:
    mode: str
    launch: int
    prologue: bool = False
    M: int = 375
    layer: int = 0
    t: int = 37
    tokens: bool = False       # in_proj of layer 0: the launch gathers its rows
    d_ff: int = 1856
    rows: str = "random"       # "random" | "layernorm" (the LayerNorm edge rows)
    seed: int = 0

    @property
    def m(self):
        return MODES[self.mode]

    @property
    def np_main(self):
        return self.m.np_w if self.launch == IN_PROJ else self.m.np_ffn

    @property
    def np_pre(self):
        return self.m.np_ffn if self.prologue else self.np_main

    @property
    def hid_panels(self):
        return self.d_ff % 32 == 0

    @property
    def out_form(self):
        """The kernel's OUT: 0 fp32 rows | 1 ReLU + hi / lo fp16 (rows or panels) | 2 hi / lo q / k / v panels | 3 ReLU + hi-only panels"""
        if self.launch == IN_PROJ:
            return 2 if self.m.qkv_panels else 0
        if self.launch == LINEAR1:
            return 3 if self.m.np_ffn == 1 else 1
        return 0

    @property
    def instantiation(self):
        return (int(self.launch == IN_PROJ), self.out_form, int(self.prologue), self.np_main, self.np_pre)

    @property
    def family(self):
        return {3: "three", 2: "two", 1: "one"}[self.np_main]

    @property
    def id(self):
        s = f"{self.mode}-{LAUNCH_NAMES[self.launch]}{self.layer if self.launch != HEAD else ''}-{'pre' if self.prologue else 'tok' if self.tokens else 'rows'}-M{self.M}"
        return s + (f"-ff{self.d_ff}" if self.d_ff != 1856 else "") + ("-ln" if self.rows != "random" else "")


def form_cases():
    """Every launch form of every mode at M = 375 (three layouts; M % 128 = 119): between them the 14 instantiations."""
    out = []
    for m in MODES.values():
        out.append(Case(m.name, IN_PROJ, tokens=True, layer=0))
        if m.ffn_launches:
            out += [Case(m.name, IN_PROJ, prologue=True, layer=2), Case(m.name, LINEAR1, layer=1), Case(m.name, HEAD, prologue=True)]
        else:
            out += [Case(m.name, IN_PROJ, layer=3, t=81), Case(m.name, HEAD)]
    return out


ROW_COUNTS = (1, 125, 128, 129, 255)   # one row in a lone block, one layout, a full block, a second block of one row, a block lacking one row


def row_cases():
    out = []
    for M in ROW_COUNTS:
        out += [Case("split", IN_PROJ, tokens=True, layer=0, M=M, seed=M), Case("split", IN_PROJ, prologue=True, layer=1, M=M, seed=M),
                Case("split", HEAD, prologue=True, M=M, seed=M)]
    return out


def layernorm_cases():
    return [Case("split", LINEAR1, layer=2, M=128, rows="layernorm"), Case("split", IN_PROJ, layer=1, M=128, rows="layernorm")]


DFF_GEOMETRIES = (1840, 1824)   # d_ff % 32 = 16: a partly masked last tile, row-major hidden rows | 57 tiles rounded up to 58: a wholly masked tile


def dff_cases():
    return [Case(mode, launch, prologue=launch == HEAD, layer=1, M=250, d_ff=F) for F in DFF_GEOMETRIES for mode in ("split", "mixed")
            for launch in (LINEAR1, HEAD)]


def all_cases():
    return form_cases() + row_cases() + layernorm_cases() + dff_cases()


# ---------------------------------------------------------------------------------------------------------------- tolerances
# max |out - ref| / max |ref| over every row and column of a launch.
# Three- and two-product forms, the LayerNorm edge rows: 4 x the largest value measured on the MI355X over the family's cases (the 4 covers
# seed and accumulation-order spread; the measured values: tests/test_lngemm_gpu.py's docstring), but never above 1e-2 of the smallest
# lo-dropped yardstick of the SAME case — lo_cap below, which is what binds: the launches measure 3.1e-7 .. 6.6e-7, 4 x that is 2.6e-6, and
# a dropped lo term sits at 1.3e-4 .. 2.8e-4.  (Where the 6.6e-7 come from: the emulation with every product summed exactly is 1.3e-7 ..
# 3.4e-7 away from float64; the same emulation with the 87 / 348 MFMA results of a tile / of the prologue added one by one in fp32, two
# alternating chains, 2.8e-7 .. 4.4e-7 — the kernel's accumulation order, not a lost term: a lost term is 200 times that.)
# y32: 4 x measured — 3.9e-7 on rows that are read or gathered, 1.2e-6 where the prologue's 348 fp32 accumulations make them.
# One-product forms: one_product_bar below.
BAR = {"three": 2.6e-6, "two": 2.7e-6}
BAR_Y32 = {False: 1.6e-6, True: 4.7e-6}      # [behind the linear2 prologue]
BAR_LN_ROWS = 3.2e-6                         # out (7.9e-7 measured) and y32 (8.1e-7): fp32 statistics lose digits with the row's offset
HI_ONLY_REL = 2.0 ** -11   # plain-fp16 outputs: |hi - ref| <= 2^-11 |ref| + bar * max |ref|


# ---------------------------------------------------------------------------------------------------------------- weights
def spec_for(d_ff=1856):
    return dataclasses.replace(SP.RICO25, d_ff=d_ff)


@functools.lru_cache(maxsize=None)
def state_dict(point, d_ff=1856):
    spec = spec_for(d_ff)
    sd = synth.synth_state_dict(spec, seed=1, perturb=True) if point == "perturb" else synth.trained_like_state_dict(spec, point, seed=3)
    return synth.strip_prefix(sd)


def f16(x):
    """fp16 rounding of float32 / float64 values, as float64"""
    return np.asarray(x).astype(np.float16).astype(np.float64)


def prescale(w):
    """2^k of ldm_weights.cpp make_w16: the exact power of two that brings max |w| into [1, 2) before the hi / lo split"""
    mx = float(np.abs(w).max())
    return 2.0 ** (-int(np.floor(np.log2(mx)))) if mx > 0 and np.isfinite(mx) else 1.0


def split_w(w):
    """(hi, lo, 2^k) of a float32 weight as the split mode keeps it: hi = fp16(w 2^k), lo = fp16(w 2^k - hi), both as float64"""
    k = prescale(w)
    ws = (w.astype(np.float32) * np.float32(k)).astype(np.float32)
    hi = ws.astype(np.float16)
    lo = (ws - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64), k


def split_x(x32):
    """hi / lo fp16 halves of float32 values (kSplitLoScale = 1), as float16 arrays"""
    x32 = np.asarray(x32, np.float32)
    hi = x32.astype(np.float16)
    return hi, (x32 - hi.astype(np.float32)).astype(np.float16)


def qkv_row(n, H=8, dh=58):
    """ldm_pack::qkv_row: in_proj row n = which * D + head * dh + d -> (which * H + head) * 64 + d"""
    n = np.asarray(n)
    return ((n // D) * H + (n % D) // dh) * 64 + (n % D) % dh


def adaln_row(sd, layer, t, dtype=np.float64):
    b = f"transformer.backbone.layers.{layer}.norm1."
    e = sd[b + "emb.weight"][t].astype(dtype)
    e = e / (1.0 + np.exp(-e))     # SiLU
    ss = sd[b + "linear.weight"].astype(dtype) @ e + sd[b + "linear.bias"].astype(dtype)
    return ss[:D], ss[D:]


# ---------------------------------------------------------------------------------------------------------------- operands
@dataclasses.dataclass
class Operands:
    W: np.ndarray            # [N, 464] float32 main weight (logical rows: 3 D | d_ff | C)
    bias: object             # [N] float32 or None
    p0: np.ndarray           # AdaLN scale | gamma   (float64 for AdaLN: the table row computed from the fp32 checkpoint)
    p1: np.ndarray
    ada: bool
    relu: bool
    tokens: object = None    # [M] int32
    emb: object = None
    pos: object = None       # [S, 464] float32 = elem_emb[s // 5] + attr_emb[s % 5], as the engine's table holds it
    x: object = None         # [M, 464] float32 rows
    hid_hi: object = None    # [M, d_ff] float16, >= 0
    hid_lo: object = None
    res: object = None       # [M, 464] float32
    W2: object = None        # [464, d_ff] float32
    b2: object = None


def make_rows(rng, M, kind="random"):
    """Rows with a per-row scale in [0.3, 3] and a per-row offset of at most one row standard deviation; every row and column distinct."""
    x = rng.standard_normal((M, D))
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), (M, 1)))
    off = rng.uniform(-1.0, 1.0, (M, 1)) * scale
    x = x * scale + off
    if kind == "layernorm":     # one 128-row block: the LayerNorm edges in its first rows, ordinary rows behind them
        x[0] = 0.75                                     # constant: variance 0, eps decides
        x[1] = 0.0
        x[1, 77] = 1.5                                  # one non-zero element
        x[2] = rng.standard_normal(D) * 1e-3
        x[3] = rng.standard_normal(D) * 1e3
        x[4] = rng.standard_normal(D) + 4.0             # offset of 4 standard deviations
        x[5] = rng.standard_normal(D) * 0.5 - 2.0
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def operands(case: Case) -> Operands:
    sd = state_dict(case.m.point, case.d_ff)
    rng = np.random.default_rng(1000 + case.seed * 7919 + case.launch * 31 + case.M)
    tr, M = "transformer.", case.M
    if case.launch == IN_PROJ:
        b = f"{tr}backbone.layers.{case.layer}."
        p0, p1 = adaln_row(sd, case.layer, case.t)
        op = Operands(W=sd[b + "self_attn.in_proj_weight"], bias=sd[b + "self_attn.in_proj_bias"], p0=p0, p1=p1, ada=True, relu=False)
    elif case.launch == LINEAR1:
        b = f"{tr}backbone.layers.{case.layer}."
        op = Operands(W=sd[b + "linear1.weight"], bias=sd[b + "linear1.bias"], p0=sd[b + "norm2.weight"], p1=sd[b + "norm2.bias"], ada=False, relu=True)
    else:
        op = Operands(W=sd[tr + "head.1.weight"], bias=None, p0=sd[tr + "head.0.weight"], p1=sd[tr + "head.0.bias"], ada=False, relu=False)
    if case.prologue:
        src = (case.layer - 1) if case.launch == IN_PROJ else SP.RICO25.n_layer - 1
        b = f"{tr}backbone.layers.{src}."
        op.W2, op.b2 = sd[b + "linear2.weight"], sd[b + "linear2.bias"]
        # (amplitude: linear2's sum is a few times the residual rows — a fault of the prologue is not diluted by them)
        h = np.abs(rng.standard_normal((M, case.d_ff))) * 8.0 * np.exp(rng.uniform(-0.7, 0.7, (M, 1)))
        h[rng.random((M, case.d_ff)) < 0.5] = 0.0     # like a ReLU output: about half the entries exactly zero
        op.hid_hi, op.hid_lo = split_x(h.astype(np.float32))
        op.res = (rng.standard_normal((M, D)) * 2.0).astype(np.float32)
    elif case.tokens:
        op.tokens = rng.integers(0, SP.RICO25.n_class, M).astype(np.int32)
        op.emb = sd[tr + "cat_emb.weight"]
        s = np.arange(S)
        op.pos = (sd[tr + "pos_emb.elem_emb"][s // 5] + sd[tr + "pos_emb.attr_emb"][s % 5]).astype(np.float32)
    else:
        op.x = make_rows(rng, M, case.rows)
    return op


# ---------------------------------------------------------------------------------------------------------------- float64 reference
YARDSTICKS = ("w_lo", "x_lo", "pre_w_lo", "hid_lo", "k16", "rows32", "tile")
LO_DROPPED = ("w_lo", "x_lo", "pre_w_lo", "hid_lo")


def applicable(case: Case):
    """The yardsticks that are a DIFFERENT computation for this form (a form that is specified without a lo term has none to drop)"""
    ys = ["k16", "tile"]
    if case.M > 32:
        ys.append("rows32")
    if case.np_main == 3:
        ys.append("w_lo")
    if case.np_main >= 2:
        ys.append("x_lo")
    if case.prologue and case.np_pre == 3:
        ys.append("pre_w_lo")
    if case.prologue and case.np_pre >= 2:
        ys.append("hid_lo")
    return ys


def _rounded_w(w):
    hi, _, k = split_w(w)
    return hi / k


def reference(case: Case, wrong=None):
    """float64 (y, out) of the launch as its form is SPECIFIED: three products = the fp32 weight; two = fp16(W 2^k) / 2^k; one = additionally
    fp16(y), and in the prologue the hi half of the hidden activations only.  out [M, N] in logical columns (N = 3 D | d_ff | C).
    wrong: one of YARDSTICKS — the same launch with that fault."""
    op = operands(case)
    f8 = np.float64
    if case.prologue:
        hid = op.hid_hi.astype(f8)
        if case.np_pre >= 2 and wrong != "hid_lo":
            hid = hid + op.hid_lo.astype(f8)
        W2 = op.W2.astype(f8) if (case.np_pre == 3 and wrong != "pre_w_lo") else _rounded_w(op.W2)
        x = op.res.astype(f8) + op.b2.astype(f8) + hid @ W2.T
    elif case.tokens:
        x = op.emb.astype(f8)[op.tokens] + op.pos.astype(f8)[np.arange(case.M) % S]
    else:
        x = op.x.astype(f8)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    g = (1.0 + op.p0.astype(f8)) if op.ada else op.p0.astype(f8)
    y = (x - mu) / np.sqrt(var + EPS) * g + op.p1.astype(f8)
    ym = f16(y) if (case.np_main == 1 or wrong == "x_lo") else y
    if wrong == "k16":
        ym = ym.copy()
        ym[:, 448:] = 0.0          # the last k16-step missing
    W = op.W.astype(f8) if (case.np_main == 3 and wrong != "w_lo") else _rounded_w(op.W)
    out = ym @ W.T
    if op.bias is not None:
        out = out + op.bias.astype(f8)
    if op.relu:
        out = np.maximum(out, 0.0)
    if wrong == "rows32":
        r = np.arange(case.M)
        src = np.where((r ^ 32) < case.M, r ^ 32, r)
        out = out[src]
    if wrong == "tile":
        out = np.roll(out, 32, axis=1)
    return y, out


def rel_err(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def worst_location(a, ref):
    """(row, column, wave, tile) of the largest |a - ref|"""
    d = np.abs(np.asarray(a, np.float64) - ref)
    r, c = np.unravel_index(int(np.argmax(d)), d.shape)
    return int(r), int(c), int(r % 128) // 32, int(c) // 32


# ---------------------------------------------------------------------------------------------------------------- float32 emulation
def emulate(case: Case):
    """(y32, out) as the kernel's arithmetic gives them: float32 rows, two-pass float32 statistics, fp16 hi / lo split of the LayerNorm output and
    of the pre-scaled weights, the form's products summed in float64 and rounded to float32 ONCE (the kernel's fp32 accumulation order adds its
    own noise on top), float32 epilogue, hi / lo split of the fp16 outputs (returned as hi + lo; the hi-only form as hi)."""
    op = operands(case)
    f4, f8 = np.float32, np.float64
    if case.prologue:
        w2h, w2l, k2 = split_w(op.W2)
        ah, al = op.hid_hi.astype(f8), op.hid_lo.astype(f8)
        acc = ah @ w2h.T
        if case.np_pre >= 2:
            acc = acc + al @ w2h.T
        if case.np_pre == 3:
            acc = acc + ah @ w2l.T
        acc = acc.astype(f4)
        x = (acc * f4(1.0 / k2) + op.b2.astype(f4)) + op.res
    elif case.tokens:
        x = op.emb[op.tokens] + op.pos[np.arange(case.M) % S]
    else:
        x = op.x
    x = x.astype(f4)
    inv_d = f4(1.0) / f4(D)
    mean = x.sum(-1, keepdims=True, dtype=f4) * inv_d
    dx = x - mean
    rstd = f4(1.0) / np.sqrt((dx * dx).sum(-1, keepdims=True, dtype=f4) * inv_d + f4(EPS))
    g = (f4(1.0) + op.p0.astype(f4)) if op.ada else op.p0.astype(f4)
    y = (dx * rstd * g + op.p1.astype(f4)).astype(f4)
    yh, yl = split_x(y)
    wh, wl, k = split_w(op.W)
    acc = yh.astype(f8) @ wh.T
    if case.np_main >= 2:
        acc = acc + yl.astype(f8) @ wh.T
    if case.np_main == 3:
        acc = acc + yh.astype(f8) @ wl.T
    out = acc.astype(f4) * f4(1.0 / k)
    if op.bias is not None:
        out = out + op.bias.astype(f4)
    if op.relu:
        out = np.maximum(out, f4(0.0))
    out = out.astype(f4)
    if case.out_form in (1, 2):
        oh, ol = split_x(out)
        out = oh.astype(f8) + ol.astype(f8)
    elif case.out_form == 3:
        out = out.astype(np.float16).astype(f8)
    return y, out.astype(f8)


@functools.lru_cache(maxsize=None)
def one_product_bar(case: Case):
    """The bar of a one-product form: it rounds y to fp16 ONCE — the float64 reference rounds the float64 y, the kernel the float32 y, and a few
    elements land on the other side of a rounding boundary.  3 x the difference between the float32 emulation and that reference on the same
    operands (for the hi-only output: of what exceeds its own fp16 rounding)."""
    assert case.family == "one"
    _, ref = reference(case)
    _, emu = emulate(case)
    d = np.abs(emu - ref)
    if case.out_form == 3:
        d = np.maximum(d - HI_ONLY_REL * np.abs(ref), 0.0)
    return 3.0 * float(d.max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def lo_cap(case: Case):
    """1e-2 of the smallest lo-dropped yardstick of the case (the ratio tests/test_attnout_gpu.py uses)"""
    _, ref = reference(case)
    return 1e-2 * min(rel_err(reference(case, w)[1], ref) for w in applicable(case) if w in LO_DROPPED)


def bar(case: Case):
    if case.family == "one":
        return one_product_bar(case)
    return min(BAR_LN_ROWS if case.rows == "layernorm" else BAR[case.family], lo_cap(case))


def bar_y32(case: Case):
    return BAR_LN_ROWS if case.rows == "layernorm" else BAR_Y32[case.prologue]


# ---------------------------------------------------------------------------------------------------------------- output layouts
def unpack_panels(buf16, n_panels, panel_halves):
    """Panel-major fp16 output (ldm_kernels.h LnGemmArgs): column c of row r at panel c / 32, byte r * 64 + (c % 32) * 2.
    buf16: flat uint16 / float16 array; panel_halves = panel_stride / 2 -> [rows, 32 n_panels] with rows = panel_halves / 32"""
    rows = panel_halves // 32
    a = np.asarray(buf16)[: n_panels * panel_halves].reshape(n_panels, panel_halves)[:, : rows * 32].reshape(n_panels, rows, 32)
    return a.transpose(1, 0, 2).reshape(rows, n_panels * 32)


def pack_panels(rows16, n_panels, panel_halves):
    """[M, 32 n_panels] -> flat panel-major array of n_panels * panel_halves halves (rows beyond M zero)"""
    M = rows16.shape[0]
    out = np.zeros((n_panels, panel_halves), rows16.dtype)
    out[:, : M * 32] = rows16.reshape(M, n_panels, 32).transpose(1, 0, 2).reshape(n_panels, M * 32)
    return out.reshape(-1)


def qkv_logical(padded):
    """[M, 1536] head-padded q / k / v columns -> ([M, 1392] logical columns, [M, 144] the padding d = 58 .. 63 of every head)"""
    idx = qkv_row(np.arange(3 * D))
    pad = np.setdiff1d(np.arange(1536), idx)
    return padded[:, idx], padded[:, pad]
