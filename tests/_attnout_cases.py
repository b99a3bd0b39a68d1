"""Shared by tests/test_attnout_reference.py (CPU) and tests/test_attnout_kernel_gpu.py (device): ONE launch of the fused attention + out_proj
(+ LayerNorm-2 + plain-fp16 FFN) kernel (layout_dm_amd/csrc/kernels_attnout.hip attnout16x3_k) — the cases, their seeded operands, the
head-padded panel layout q / k / v travel in, the float64 reference of the launch, wrong references on the same operands (the yardsticks),
an emulation of the kernel's arithmetic in its own number formats, and the bars derived from the two.  numpy only.

A launch:   x1  = res + b_out + concat_h softmax(q_h k_h^T / sqrt(58)) v_h · Wo^T                      (torch.nn.MultiheadAttention in Block.forward)
            out = x1                                                                                    split <false>, mixed <false, W2>
            out = x1 + b2 + relu(LayerNorm(x1; g2, be2, eps 1e-5) · W1^T + b1) · W2^T                   hybrid <false, W2, FFN>
(oracle/restatement.py denoiser_logits restates both.)  Weights as the form SPECIFIES them: split the fp32 Wo (three products); mixed and
hybrid fp16(Wo 2^k) / 2^k (ldm_weights.cpp make_w16: the lo half is neither read nor multiplied); hybrid's FFN fp16(W1), fp16(W2), the
LayerNorm output and the hidden activations rounded to fp16 once."""
import dataclasses
import functools
import math

import numpy as np

import _lngemm_cases as LC
from _tiled_cases import PAD_VALUE

D, H, DH, EPS = 464, 8, 58, 1e-5
N_PANELS, REACH = 48, 128                  # (which * 8 + head) * 2 + d / 32 | rows a layout reads from its first one, in every panel
NAN32 = LC.NAN32
N_LAYER = 4
V_AMP = (1.0, 4.0, 0.25)                   # amplitude of V per layout: a read across a layout boundary shows
S_EDGES = (1, 31, 32, 33, 50, 64, 65, 96, 97, 127, 128)
D_FF = (1856, 1824, 2048, 32)              # 58, 57, 64, 1 chunks: even, odd, the sb1 table's limit, a single chunk
QK_AMPS = (0.3, 1.0, 2.5)
PEAK = 40.0                                # largest scaled score of the peaked case (42 on the fitted checkpoint)

# <TM, W2, FFN> of attnout16x3_k that launch_attnout16x3 picks without the phase-timer knob
FORMS = {"split": (False, False, False), "mixed": (False, True, False), "hybrid": (False, True, True)}
INSTANTIATIONS = frozenset(FORMS.values())


@dataclasses.dataclass(frozen=True)
class Case:
    mode: str
    B: int = 3
    S: int = 125
    layer: int = 0
    d_ff: int = 1856
    kind: str = "random"       # "random" | "q0" (q = 0: P = 1 / S exactly) | "peaked" (one key carries the row)
    amp: float = 1.0           # amplitude of q and k
    seed: int = 0

    @property
    def w2(self):
        return FORMS[self.mode][1]

    @property
    def ffn(self):
        return FORMS[self.mode][2]

    @property
    def instantiation(self):
        return FORMS[self.mode]

    @property
    def M(self):
        return self.B * self.S

    @property
    def panel_rows(self):
        return (self.B - 1) * self.S + REACH

    @property
    def family(self):
        return {"split": "three products", "mixed": "two-product out_proj", "hybrid": "out_proj + FFN"}[self.mode]

    @property
    def id(self):
        s = f"{self.mode}-L{self.layer}-B{self.B}-S{self.S}"
        s += f"-ff{self.d_ff}" if self.d_ff != 1856 else ""
        s += f"-{self.kind}" if self.kind != "random" else ""
        return s + (f"-amp{self.amp:g}" if self.amp != 1.0 else "") + (f"-s{self.seed}" if self.seed else "")


def form_cases():
    """The three instantiations at the product's shape, on the first and on the last layer"""
    return [Case(mode, layer=layer) for mode in FORMS for layer in (0, N_LAYER - 1)]


def s_edge_cases():
    """A wave with no rows, one row, all its rows; every key tile wholly masked, partly masked, unmasked; odd S (layout starts 64-byte aligned only)"""
    seed = lambda mode, B, S: TIE_FREE_SEED[B] if (mode, S) == ("hybrid", 1) else S
    out = [Case(mode, B=2, S=S, layer=1, seed=seed(mode, 2, S)) for S in S_EDGES for mode in FORMS]
    return out + [Case(mode, B=1, S=S, layer=2, seed=seed(mode, 1, S)) for S in (1, 128) for mode in FORMS]


# the FFN form at S = 1: the first seed >= 1 for which no fp16 rounding of the reference is decided by less than TIE_ULPS fp32 ulps (near_ties
# below says why; tests/test_attnout_reference.py recomputes both)
TIE_FREE_SEED = {1: 6, 2: 64}


def score_cases():
    out = []
    for mode in ("split", "mixed"):
        out += [Case(mode, layer=1, amp=a, seed=3) for a in QK_AMPS]
        out += [Case(mode, layer=1, kind="q0", seed=4), Case(mode, layer=2, kind="peaked", seed=5)]
    return out


def dff_cases():
    return [Case("hybrid", B=2, layer=1, d_ff=F, seed=6) for F in D_FF]


IN_PLACE = Case("hybrid", B=3, layer=2, seed=11)     # ffn_out == res (the product: ws.P for both) against ffn_out != res


def all_cases():
    return form_cases() + s_edge_cases() + score_cases() + dff_cases() + [IN_PLACE]


# ---------------------------------------------------------------------------------------------------------------- weights
@dataclasses.dataclass
class Weights:
    Wo: np.ndarray       # [464, 464] float32
    bo: np.ndarray
    g2: np.ndarray
    be2: np.ndarray
    W1: np.ndarray       # [F, 464]
    b1: np.ndarray
    W2: np.ndarray       # [464, F]
    b2: np.ndarray


@functools.lru_cache(maxsize=None)
def weights(mode, layer, d_ff):
    sd = LC.state_dict(LC.MODES[mode].point, d_ff)
    b = f"transformer.backbone.layers.{layer}."
    return Weights(Wo=sd[b + "self_attn.out_proj.weight"], bo=sd[b + "self_attn.out_proj.bias"], g2=sd[b + "norm2.weight"], be2=sd[b + "norm2.bias"],
                   W1=sd[b + "linear1.weight"], b1=sd[b + "linear1.bias"], W2=sd[b + "linear2.weight"], b2=sd[b + "linear2.bias"])


def case_weights(case: Case) -> Weights:
    return weights(case.mode, case.layer, case.d_ff)


# ---------------------------------------------------------------------------------------------------------------- operands
@dataclasses.dataclass
class Operands:
    q: np.ndarray        # [B S, 8, 58] float32
    k: np.ndarray
    v: np.ndarray
    res: np.ndarray      # [B S, 464] float32


@functools.lru_cache(maxsize=None)
def operands(case: Case) -> Operands:
    B, S, M = case.B, case.S, case.M
    rng = np.random.default_rng([case.seed, B, S, list(FORMS).index(case.mode), case.layer, case.d_ff, int(case.amp * 10), len(case.kind)])
    q = rng.uniform(-1.0, 1.0, (B, S, H, DH)) * case.amp
    k = rng.uniform(-1.0, 1.0, (B, S, H, DH)) * case.amp
    v = rng.uniform(-1.0, 1.0, (B, S, H, DH)) * np.array([V_AMP[b % 3] for b in range(B)])[:, None, None, None]
    if case.kind == "q0":
        q[:] = 0.0
    elif case.kind == "peaked":
        # per (layout, head) every query lies along u, and ONE key is a u: its scaled score is a^2 58 / sqrt(58) = PEAK for every row, the other
        # keys' below 5.  Head 0's key is the layout's LAST one (the masked-key yardstick bites), the others' are drawn.
        a = math.sqrt(PEAK / math.sqrt(DH))
        for b in range(B):
            for h in range(H):
                u = rng.choice([-1.0, 1.0], DH)
                q[b, :, h] = a * u + rng.uniform(-0.3, 0.3, (S, DH))
                k[b, S - 1 if h == 0 else int(rng.integers(0, S)), h] = a * u
    res = rng.uniform(-2.0, 2.0, (M, D))
    f = lambda x: np.ascontiguousarray(x.reshape(M, H, DH), np.float32)
    return Operands(q=f(q), k=f(k), v=f(v), res=res.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- panels
def pack_qkv_panels(q, k, v, rows):
    """(hi, lo) uint16 [48, rows, 32] of fp32 q / k / v [M, 8, 58] — ldm_kernels.h AttnOutArgs: hi and lo fp16 arrays of 48 panels, panel
    (which * 8 + head) * 2 + d / 32, 64 bytes per row, the head padding d = 58 .. 63 zero; the rows behind M hold PAD_VALUE in every half."""
    M = q.shape[0]
    hi = np.zeros((N_PANELS, rows, 32), np.float16)
    lo = np.zeros((N_PANELS, rows, 32), np.float16)
    ph, pl = LC.split_x(np.float32(PAD_VALUE))
    hi[:, M:], lo[:, M:] = ph, pl
    for which, x in enumerate((q, k, v)):
        xh, xl = LC.split_x(x)
        for h in range(H):
            for half in range(2):
                d0, d1 = 32 * half, min(32 * half + 32, DH)
                p = (which * H + h) * 2 + half
                hi[p, :M, : d1 - d0], lo[p, :M, : d1 - d0] = xh[:, h, d0:d1], xl[:, h, d0:d1]
    return hi.view(np.uint16), lo.view(np.uint16)


def unpack_qkv_panels(hi, lo, M):
    """-> (q, k, v) [M, 8, 58] float64 = hi + lo of the panels' first M rows, and the head padding's halves [2, 24, M, 6] as uint16"""
    full = hi.view(np.float16)[:, :M].astype(np.float64) + lo.view(np.float16)[:, :M].astype(np.float64)      # [48, M, 32]
    x = full.reshape(3, H, 2, M, 32).transpose(0, 3, 1, 2, 4).reshape(3, M, H, 64)
    pad = np.stack([a.reshape(3 * H, 2, -1, 32)[:, 1, :M, DH - 32:] for a in (hi, lo)])
    return x[0, :, :, :DH], x[1, :, :, :DH], x[2, :, :, :DH], pad


def row_behind(case: Case):
    """(k, v) [B, 8, 58] float64 of the panel row behind every layout's rows: the next layout's first row, PAD_VALUE behind the last layout"""
    op = operands(case)
    k = np.full((case.B, H, DH), PAD_VALUE, np.float64)
    v = k.copy()
    for b in range(case.B - 1):
        k[b], v[b] = op.k[(b + 1) * case.S], op.v[(b + 1) * case.S]
    return k, v


# ---------------------------------------------------------------------------------------------------------------- float64 reference
YARDSTICKS = ("act_lo", "wo_lo", "mask_last", "unmask_next", "heads_swapped", "k16", "tile", "ffn_last_chunk", "ffn_b1_shift", "ffn_ln_unbiased")
FFN_YARDSTICKS = ("ffn_last_chunk", "ffn_b1_shift", "ffn_ln_unbiased")
INFORMATIONAL = ("ffn_hid_exact",)         # the hidden activations not rounded to fp16: reported, not part of any bar


def applicable(case: Case):
    """The yardsticks that are a DIFFERENT computation for this case"""
    ys = ["act_lo", "heads_swapped", "k16", "tile"]
    if not case.w2:
        ys.append("wo_lo")                  # (the two-product forms are specified without it)
    if case.S >= 2:
        ys.append("mask_last")              # (S = 1: no key would be left)
    if case.S < REACH:
        ys.append("unmask_next")
    if case.ffn:
        ys += ["ffn_last_chunk", "ffn_ln_unbiased"]
        if case.d_ff > 32:
            ys.append("ffn_b1_shift")       # (one chunk: the shift is the identity)
    return ys


def _f16(x):
    return LC.f16(x)


def _rounded_w(w):
    hi, _, k = LC.split_w(w)
    return hi / k


def reference(case: Case, wrong=None, parts=False):
    """float64 out [M, 464] of the launch as its form is specified.  wrong: one of YARDSTICKS / INFORMATIONAL — the same launch with that fault:
      act_lo           the lo halves of q, k, v, of P (after its 2^10 scaling) and of the attention output dropped
      wo_lo            the lo half of Wo dropped
      mask_last        key S - 1 masked              unmask_next     key S — the panel row behind the layout — not masked
      heads_swapped    heads 2 and 5 multiply each other's out_proj stages
      k16              the second k16-step (d = 16 .. 31) of head 3's out_proj missing
      tile             output columns 64 .. 95 of the attention block taken from the tile behind them
      ffn_last_chunk   the last 32 hidden units missing       ffn_b1_shift   b1 shifted by one chunk
      ffn_ln_unbiased  LayerNorm-2 with the variance over 463     ffn_hid_exact  hidden activations not rounded to fp16
    parts (FFN form): -> (the LayerNorm-2 output, the hidden pre-activations floored at 0), both BEFORE their fp16 rounding"""
    op, w, B, S, M = operands(case), case_weights(case), case.B, case.S, case.M
    f8 = np.float64
    q, k, v = (x.astype(f8).reshape(B, S, H, DH) for x in (op.q, op.k, op.v))
    if wrong == "act_lo":
        q, k, v = _f16(q), _f16(k), _f16(v)
    if wrong == "unmask_next":
        kb, vb = row_behind(case)
        k, v = np.concatenate([k, kb[:, None]], 1), np.concatenate([v, vb[:, None]], 1)
    s = q.transpose(0, 2, 1, 3) @ k.transpose(0, 2, 3, 1) / math.sqrt(DH)      # [B, 8, query, key]
    if wrong == "mask_last":
        s[..., S - 1] = -np.inf
    e = np.exp(s - s.max(-1, keepdims=True))
    den = e.sum(-1, keepdims=True)
    if wrong == "act_lo":
        e = _f16(e * 1024.0) / 1024.0
    att = ((e / den) @ v.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)
    if wrong == "act_lo":
        att = _f16(att)
    att = att.reshape(M, H, DH).copy()
    if wrong == "k16":
        att[:, 3, 16:32] = 0.0
    Wo = w.Wo.astype(f8) if (not case.w2 and wrong != "wo_lo") else _rounded_w(w.Wo)
    Wh = Wo.reshape(D, H, DH)
    if wrong == "heads_swapped":
        Wh = Wh.copy()
        Wh[:, [2, 5]] = Wh[:, [5, 2]]
    y = att.reshape(M, D) @ Wh.reshape(D, D).T
    if wrong == "tile":
        y[:, 64:96] = y[:, 96:128]
    x1 = op.res.astype(f8) + w.bo.astype(f8) + y
    if not case.ffn:
        return x1
    F = case.d_ff
    mu = x1.mean(-1, keepdims=True)
    var = ((x1 - mu) ** 2).sum(-1, keepdims=True) / (D - 1 if wrong == "ffn_ln_unbiased" else D)
    y64 = (x1 - mu) / np.sqrt(var + EPS) * w.g2.astype(f8) + w.be2.astype(f8)
    yn = _f16(y64)
    b1 = w.b1.astype(f8)
    if wrong == "ffn_b1_shift":
        b1 = np.roll(b1, 32)
    hid = np.maximum(yn @ _f16(w.W1).T + b1, 0.0)
    if parts:
        return y64, hid
    if wrong != "ffn_hid_exact":
        hid = _f16(hid)
    if wrong == "ffn_last_chunk":
        hid[:, F - 32:] = 0.0
    return x1 + w.b2.astype(f8) + hid @ _f16(w.W2).T


TIE_ULPS = 8.0


def near_ties(case: Case, ulps=TIE_ULPS):
    """How many fp16 roundings of the FFN form's reference — LayerNorm-2 output, hidden activations — are decided by less than `ulps` fp32 ulps
    of the rounded value.  The kernel rounds fp32 values that differ from the float64 ones by a few ulps (the statistics, 29 accumulations in two
    chains, the summation order inside an MFMA): such an element can land on the other side, and ONE hidden activation on the other side is
    4e-6 .. 2e-5 of the block.  From 62 rows on there are hundreds of them, in the emulation as on the device, and the distance is their
    level; with one or two rows their number is 0 .. 5, and an emulation cannot say which way each goes.  The one- and two-row FFN cases
    therefore use operands WITHOUT such an element (s_edge_cases), so that their bar is not the draw of a tie."""
    n = 0
    for x in reference(case, parts=True):
        h = x.astype(np.float16)
        with np.errstate(over="ignore"):
            mids = [(h.astype(np.float64) + np.nextafter(h, np.float16(d)).astype(np.float64)) / 2 for d in (np.inf, -np.inf)]
        dist = np.minimum(np.abs(x - mids[0]), np.abs(x - mids[1]))
        nz = x != 0                                                                     # (a hidden activation floored at 0 has no tie)
        n += int((dist[nz] < ulps * np.spacing(np.abs(x[nz]).astype(np.float32))).sum())
    return n


def mean_of_v(case: Case):
    """q = 0: every score is 0, P = 1 / S exactly, the block is the mean of V through Wo — the closed form of the launch (no softmax in it)"""
    assert case.kind == "q0" and not case.ffn
    op, w = operands(case), case_weights(case)
    vm = op.v.astype(np.float64).reshape(case.B, case.S, D).mean(1)
    Wo = w.Wo.astype(np.float64) if not case.w2 else _rounded_w(w.Wo)
    return op.res.astype(np.float64) + w.bo.astype(np.float64) + np.repeat(vm @ Wo.T, case.S, axis=0)


def rel_err(out, ref, res):
    """The measure of csrc/ldm_dev.cpp ldm_dev_attnout_check: max |out - ref| / max |ref - res| over every real row and column"""
    return float(np.abs(np.asarray(out, np.float64) - ref).max() / np.abs(ref - res.astype(np.float64)).max())


def worst_location(out, ref):
    """(row, column) of the largest |out - ref|"""
    d = np.abs(np.asarray(out, np.float64) - ref)
    r, c = np.unravel_index(int(np.argmax(d)), d.shape)
    return int(r), int(c)


# ---------------------------------------------------------------------------------------------------------------- emulation
def _pad64(x):
    """[.., 58] -> [.., 64] with the head padding zero"""
    return np.concatenate([x, np.zeros(x.shape[:-1] + (64 - DH,), x.dtype)], -1)


def _key_order(g):
    """keys of lane half g in the order its 64 score registers are summed: tile kt, register r -> 32 kt + (r & 3) + 8 (r >> 2) + 4 g"""
    return np.array([32 * kt + (r & 3) + 8 * (r >> 2) + 4 * g for kt in range(4) for r in range(16)])


def emulate(case: Case):
    """out [M, 464] as the kernel's arithmetic gives it, read off kernels_attnout.hip / ldm_pipes.h FfnStream (not off the device): every
    product as fp16 hi / lo halves, one v_mfma_f32_32x32x16_f16 = the exact sum of its 16 products added to the fp32 accumulator and rounded
    once, in the kernel's order of k16-steps and of products (lo·hi, hi·lo, hi·hi for the scores and P V; hi·hi, hi·lo, lo·hi for out_proj,
    hi·hi, hi·lo under W2); softmax in fp32 with p = exp2(fma(s, c, 10 - mx c)), the row sum in register order; P and O split to hi / lo; the
    epilogue (acc out_scale + b) + res; for the FFN form two-pass fp32 statistics, fp16 LayerNorm output, fp16 W1 / W2, two GEMM1 chains with
    b1 in the first, fp16 hidden activations, ReLU, GEMM2 on the tile that already holds x1 + b2."""
    op, w, B, S, M = operands(case), case_weights(case), case.B, case.S, case.M
    f4, f8 = np.float32, np.float64

    def halves(x):      # [M, 8, 58] fp32 -> hi, lo float64 [B, 8, S, 64]
        hi, lo = LC.split_x(x)
        return tuple(_pad64(a.astype(f8)).reshape(B, S, H, 64).transpose(0, 2, 1, 3) for a in (hi, lo))

    (qh, ql), (kh, kl), (vh, vl) = halves(op.q), halves(op.k), halves(op.v)
    sc = np.zeros((B, H, S, S), f4)                                     # [query, key]
    for ks in range(4):
        d = slice(16 * ks, 16 * ks + 16)
        for a, b in ((kl, qh), (kh, ql), (kh, qh)):
            sc = (sc + b[..., d] @ np.swapaxes(a[..., d], -1, -2)).astype(f4)      # (fp32 + float64 -> float64, rounded once)
    mx = sc.max(-1, keepdims=True)
    c = f4((f4(1.0) / np.sqrt(f4(DH))) * f4(1.4426950408889634))      # scale = 1.0f / sqrtf(58.0f), times log2(e), both in fp32
    nb = (10.0 - mx.astype(f8) * f8(c)).astype(f4)
    p = np.exp2((sc.astype(f8) * f8(c) + nb.astype(f8)).astype(f4).astype(f8)).astype(f4)
    p128 = np.zeros((B, H, S, REACH), f4)                               # (masked keys: exp2(-inf) = 0)
    p128[..., :S] = p
    part = [np.add.accumulate(p128[..., _key_order(g)], axis=-1, dtype=f4)[..., -1] for g in (0, 1)]
    inv = (f4(1.0) / (part[0] + part[1]).astype(f4)).astype(f4)[..., None]
    ph, pl = (a.astype(f8) for a in LC.split_x(p))
    o = np.zeros((B, H, S, 64), f4)
    for j0 in range(0, S, 16):
        j = slice(j0, min(j0 + 16, S))                                  # (keys >= S: P = 0 times a finite V)
        for a, b in ((vl, ph), (vh, pl), (vh, ph)):
            o = (o + b[..., j] @ a[:, :, j]).astype(f4)
    oh, ol = (a.astype(f8).transpose(0, 2, 1, 3).reshape(M, H, 64) for a in LC.split_x((o * inv).astype(f4)))
    wh, wl, kw = LC.split_w(w.Wo)
    wh, wl = (_pad64(a.reshape(D, H, DH)) for a in (wh, wl))
    acc = np.zeros((M, D), f4)
    for h in range(H):
        for st in range(4):
            d = slice(16 * st, 16 * st + 16)
            for a, b in ((wh, oh), (wh, ol)) + (() if case.w2 else ((wl, oh),)):
                acc = (acc + b[:, h, d] @ a[:, h, d].T).astype(f4)
    x1 = ((acc.astype(f8) * (1.0 / kw) + w.bo.astype(f8)).astype(f4) + op.res).astype(f4)
    if not case.ffn:
        return x1.astype(f8)
    F = case.d_ff
    # LayerNorm-2 as the lanes do it: a row lives in two lanes (g = 0, 1), each sums ITS 232 columns one by one in tile / register order, the halves
    # meet through one __shfl_xor; a * b + c is one fma (hipcc's default contraction); 1.0f / sqrtf() correctly rounded, one rounding each.
    # (A row sum taken in another order is a few fp32 ulps elsewhere, which puts some elements of the fp16 LayerNorm output on the other side of
    #  a rounding boundary: at one row, or 32 hidden units, where the float64 reference has no such element at all, that IS the whole distance.)
    halves = [np.array([t * 32 + (i >> 2) * 8 + g * 4 + (i & 3) for t in range(15) for i in range(16) if t * 4 + (i >> 2) < 58]) for g in (0, 1)]
    inv_d = f4(f4(1.0) / f4(D))
    s1 = [np.add.accumulate(x1[:, c], axis=-1, dtype=f4)[:, -1] for c in halves]
    mean = ((s1[0] + s1[1]).astype(f4) * inv_d).astype(f4)[:, None]
    dx = (x1 - mean).astype(f4)
    s2 = []
    for c in halves:
        a = np.zeros(M, f4)
        for j in c:
            a = (a + dx[:, j].astype(f8) * dx[:, j].astype(f8)).astype(f4)
        s2.append(a)
    var = ((s2[0] + s2[1]).astype(f4).astype(f8) * f8(inv_d) + f8(f4(EPS))).astype(f4)
    rstd = (f4(1.0) / np.sqrt(var).astype(f4)).astype(f4)[:, None]
    yn = ((dx * rstd).astype(f4).astype(f8) * w.g2.astype(f8) + w.be2.astype(f8)).astype(f4).astype(np.float16).astype(f8)
    W1, W2 = _f16(w.W1), _f16(w.W2)
    ha = hb = None
    for it in range(D // 16):
        d = slice(16 * it, 16 * it + 16)
        t = yn[:, d] @ W1[:, d].T
        if it == 0:
            ha = (w.b1.astype(f8) + t).astype(f4)
        elif it == 1:
            hb = t.astype(f4)
        elif it % 2 == 0:
            ha = (ha + t).astype(f4)
        else:
            hb = (hb + t).astype(f4)
    hid = np.maximum((ha + hb).astype(f4).astype(np.float16), np.float16(0)).astype(f8)
    out = (x1 + w.b2.astype(f4)).astype(f4)
    for j0 in range(0, F, 16):
        j = slice(j0, j0 + 16)
        out = (out + hid[:, j] @ W2[:, j].T).astype(f4)
    return out.astype(f8)


# ---------------------------------------------------------------------------------------------------------------- figures and bars
@functools.lru_cache(maxsize=None)
def figures(case: Case):
    """-> dict: emu (the emulation's distance from the float64 reference), ys {yardstick: its distance}, info {...}, bar.  Nothing here
    comes from a device.
      split and two-product forms: bar = min(4 x emu, 1e-2 x the case's smallest applicable yardstick)
      FFN form:                    bar = 3 x emu — a format that rounds activations to plain fp16 cannot be matched more tightly than its own
                                   error level (the reference rounds the float64 LayerNorm output, the kernel the fp32 one: a few elements land
                                   on the other side of a rounding boundary); no yardstick cap"""
    res, ref = operands(case).res, reference(case)
    emu = rel_err(emulate(case), ref, res)
    ys = {y: rel_err(reference(case, y), ref, res) for y in applicable(case)}
    info = {y: rel_err(reference(case, y), ref, res) for y in INFORMATIONAL} if case.ffn else {}
    bar = 3.0 * emu if case.ffn else min(4.0 * emu, 1e-2 * min(ys.values()))
    return dict(emu=emu, ys=ys, info=info, bar=bar)


def bar(case: Case):
    return figures(case)["bar"]
