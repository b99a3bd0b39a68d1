"""Shared by tests/test_tiled_reference.py (CPU) and tests/test_tiled_kernels_gpu.py (device): ONE launch of a kernel of the tiled engines
(layout_dm_amd/csrc/ldm_denoise.cpp denoise_chunk_tiled / denoise_chunk_fast) — launch_layernorm, launch_gemm, launch_gemm16x3, launch_gemm16,
launch_attention, launch_attention16 — on seeded operands: the cases, the float64 reference of each, wrong references on the same operands (the
yardsticks: what a subtly wrong kernel would measure), a CPU emulation of the kernel's arithmetic in its number formats, and the bars.  numpy only.

    GEMM        C = act(scale * A W^T + bias) + res        (ReLU before the residual, as the epilogues do it)
    attention   softmax(q k^T / sqrt(dh)) v per (layout, head)
    LayerNorm   (x - mean) / sqrt(var + 1e-5) * (1 + scale) + shift  |  * gamma + beta;  x = emb[token] + pos[row % S] when gathered

Every error is max |out - ref| / mag with mag = max |ref| of the launch (GEMM with a residual: of the part in front of it, so that the
residual does not dilute a fault of the product).

Bars.  exact and fp16 x 3 kernels, LayerNorm: min(4 x the emulation's distance from float64, 1e-2 x the case's smallest yardstick) — the 4
covers accumulation order (the emulation adds a k-step at a time, rounding to fp32 after each; the MFMA chains, the wave reductions and
contracted multiply-adds round elsewhere).  fp16-product kernels (gemm16, attention16): 3 x the emulation's distance, as the one-product
rows of tests/_lngemm_cases.py.  Nothing here is taken from a device."""
import dataclasses
import functools
import zlib

import numpy as np

NAN32, NAN16 = 0x7FC01234, 0x7E55          # guard-band fill: quiet NaNs with a payload
EPS = 1e-5
F4, F8 = np.float32, np.float64
PAD_VALUE = 1000.0                          # operand rows past M / N of the whole-tile buffers: large and finite (a stored product of one shows)
OUT_SCALE = 2.0 ** -3


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def round_up(n, m):
    return (n + m - 1) // m * m


def f16(x):
    """fp16 rounding, as float64"""
    return np.asarray(x).astype(np.float16).astype(F8)


def split_x(x32):
    """hi / lo fp16 halves as the producers make them: lo = fp16(x - fp16(x)); float16 arrays"""
    x32 = np.asarray(x32, F4)
    hi = x32.astype(np.float16)
    return hi, (x32 - hi.astype(F4)).astype(np.float16)


def chain(terms, step, acc=None):
    """sum_k a[..., k] b[..., k] the way a matrix pipe accumulates it: `step` k values per instruction — their products summed exactly
    (float64) — then ONE rounding of accumulator + sum to float32; the instruction's `terms` (pairs a [..., M, K], b [..., N, K]) one after the
    other.  -> float32 [..., M, N]"""
    K = terms[0][0].shape[-1]
    a0, b0 = terms[0]
    if acc is None:
        acc = np.zeros(np.broadcast_shapes(a0.shape[:-2], b0.shape[:-2]) + (a0.shape[-2], b0.shape[-2]), F4)
    for k in range(0, K, step):
        for a, b in terms:
            acc = (acc.astype(F8) + a[..., k:k + step].astype(F8) @ np.swapaxes(b[..., k:k + step].astype(F8), -1, -2)).astype(F4)
    return acc


def rel_err(a, ref, mag):
    return float(np.abs(np.asarray(a, F8) - ref).max() / mag)


# ================================================================================================================ GEMM
EXACT, X3, F16 = 0, 1, 2
KIND_NAMES = ("exact", "x3", "gemm16")
# epilogue forms of the call sites (ldm_denoise.cpp): name -> (bias, relu, res, C32, C16, C16lo)
FORMS = {
    "bias": (1, 0, 0, 1, 0, 0),         # in_proj
    "bias_res": (1, 0, 1, 1, 0, 0),     # out_proj, linear2 (ldres != ldc32 here)
    "relu": (1, 1, 0, 1, 0, 0),         # linear1, exact
    "nobias": (0, 0, 0, 1, 0, 0),       # the head: ldc32 > N
    "relu_hilo": (1, 1, 0, 1, 1, 1),    # linear1, split: C32 + C16 + C16lo, ldc16 > N
    "c16": (1, 0, 0, 0, 1, 0),          # in_proj, fast
    "relu_c16": (1, 1, 0, 0, 1, 0),     # linear1, fast
}


@dataclasses.dataclass(frozen=True)
class GemmCase:
    kind: int
    M: int
    N: int
    K: int
    form: str
    tag: int = 0

    @property
    def id(self):
        return f"{KIND_NAMES[self.kind]}-t{self.tag}-M{self.M}-N{self.N}-K{self.K}-{self.form}"

    @property
    def tile(self):
        """(BM, BN, BK, ring stages) of the kernel the launch picks"""
        if self.kind == EXACT:
            return (128, 128, 16, 2)
        if self.kind == F16:
            return (128, 128, 64, 2)
        return (256, 128, 32, 3) if self.tag == 4 else (256, 256, 32, 2)

    @property
    def instantiation(self):
        if self.kind == EXACT:
            return "gemm_f32_tile<2>"
        bm, bn, bk, st = self.tile
        return f"{'gemm16x3_k' if self.kind == X3 else 'gemm16_k'}<{bm},{bn},{bk},{st},tag {self.tag}>"

    @property
    def n_tiles(self):
        bm, bn, _, _ = self.tile
        return ((self.M + bm - 1) // bm) * ((self.N + bn - 1) // bn)

    @property
    def nk(self):
        return self.K // self.tile[2]

    # leading dimensions: every one wider than what it holds, the residual's different from the output's
    @property
    def lda(self):
        return self.K + (4 if self.kind == EXACT else 8)

    @property
    def ldw(self):
        return self.K + (8 if self.kind == EXACT else 0)

    @property
    def ldc(self):
        r = round_up(self.N, 32)
        return r if r > self.N else self.N + 8      # 155 -> 160, 283 -> 288

    @property
    def ldres(self):
        return round_up(self.N, 4) + 12

    @property
    def a_rows(self):
        return self.M if self.kind == EXACT else round_up(self.M, 256 if self.kind == X3 else 128)

    @property
    def w_rows(self):
        return self.N if self.kind == EXACT else round_up(self.N, 256 if self.kind == X3 else 128)


def _cycle(seq, i):
    return seq[i % len(seq)]


EXACT_FORMS = ("bias", "bias_res", "relu", "nobias")
X3_FORMS = ("bias", "bias_res", "relu_hilo")
F16_FORMS = ("c16", "bias_res", "relu_c16")


def exact_gemm_cases():
    """K = 16 / 32 / 48: nk = 1 / even / odd, every M x N edge; K = 464: the product's 29 tiles; 7 column tiles for the XCD remap"""
    out, i = [], 0
    for K in (16, 32, 48):
        for M in (1, 127, 128, 129, 257):
            for N in (1, 129, 155, 283, 464):
                if M == 1 and N == 1:
                    continue            # (one element: nothing for a maximum to run over)
                out.append(GemmCase(EXACT, M, N, K, _cycle(EXACT_FORMS, i)))
                i += 1
    out += [GemmCase(EXACT, M, N, 464, f) for M, N, f in ((1, 464, "bias"), (127, 155, "nobias"), (128, 283, "nobias"), (129, 129, "bias_res"),
                                                           (257, 464, "relu"), (257, 1, "bias_res"))]
    out += [GemmCase(EXACT, 3, 893, 16, "nobias"), GemmCase(EXACT, 770, 100, 32, "bias_res")]      # 7 tiles in a row / in a column
    return out


def exact_wrap_case(n_cu):
    """K = 32, more tiles than 6 x the CU count (the persistent grid is at most 5 workgroups per CU), M and N no multiples of 128"""
    t = int(np.ceil(np.sqrt(6 * n_cu + 1)))
    return GemmCase(EXACT, 128 * t + 5, 128 * t - 5, 32, "bias_res")


def x3_gemm_cases():
    """256 x 256 / 2 stages (tags 0 .. 3) and 256 x 128 / 3 stages (tag 4): K = 32, 64, 96, 512 -> 1, 2, 3, 16 K tiles"""
    Ms, Ns = (1, 255, 256, 257), (155, 283, 256, 257, 464)
    out, i = [], 0
    for tag in (0, 4):
        for K in (32, 64, 96):
            for M in Ms:
                for N in Ns:
                    if K != 64 and (Ms.index(M) + Ns.index(N) + K // 32) % 3:
                        continue        # (the full M x N cross at K = 64; a third of it at the other K)
                    out.append(GemmCase(X3, M, N, K, "nobias" if (tag == 4 and i % 2) else _cycle(X3_FORMS, i), tag))
                    i += 1
        out += [GemmCase(X3, 257, 464, 512, "relu_hilo", tag), GemmCase(X3, 255, 155, 512, "nobias" if tag == 4 else "bias_res", tag)]
    out += [GemmCase(X3, 257, 464, 64, _cycle(X3_FORMS, tag), tag) for tag in (1, 2, 3)]
    return out


def f16_gemm_cases():
    Ms, Ns = (1, 127, 128, 129), (155, 283, 128, 129, 464)
    out, i = [], 0
    for K in (64, 128, 512):
        for M in Ms:
            for N in Ns:
                if K != 128 and (Ms.index(M) + Ns.index(N)) % 3 != K // 256:
                    continue
                out.append(GemmCase(F16, M, N, K, "nobias" if i % 5 == 4 else _cycle(F16_FORMS, i), i % 5))
                i += 1
    return out


@dataclasses.dataclass
class GemmOperands:
    A: np.ndarray            # exact: float32 [M, K]; fp16 kernels: the VALUE of the operand as float64 (hi + lo | the fp16 number)
    W: np.ndarray
    A_hi: object = None      # float16 [a_rows, K] whole-tile buffers, rows past M = PAD_VALUE
    A_lo: object = None
    W_hi: object = None
    W_lo: object = None
    bias: object = None      # float32 [N]
    res: object = None       # float32 [M, N]
    scale: float = 1.0
    A32: object = None       # the float32 values the fp16 forms were made from
    W32: object = None


@functools.lru_cache(maxsize=4)
def gemm_operands(c: GemmCase) -> GemmOperands:
    rng = _rng("gemm", c.id)
    a = (rng.standard_normal((c.M, c.K)) * np.exp(rng.uniform(-0.7, 0.7, (c.M, 1)))).astype(F4)
    w = rng.uniform(-1.0, 1.0, (c.N, c.K))
    w = (w * (1.9 / np.abs(w).max())).astype(F4)       # max |w| = 1.9: what make_w16's power-of-two pre-scale leaves
    bias, relu, res, _, _, _ = FORMS[c.form]
    op = GemmOperands(A=a, W=w, A32=a, W32=w)
    if c.kind == EXACT:
        op.W = (w * F4(OUT_SCALE)).astype(F4)           # (launch_gemm has no out_scale: the weights carry it, exactly)
    else:
        def whole(x, rows, lo):
            hi, l = split_x(x)
            buf = np.full((rows, x.shape[1]), 0.5 if lo else PAD_VALUE, np.float16)
            buf[:x.shape[0]] = l if lo else hi
            return buf
        op.A_hi, op.W_hi = whole(a, c.a_rows, False), whole(w, c.w_rows, False)
        op.A, op.W = op.A_hi[:c.M].astype(F8), op.W_hi[:c.N].astype(F8)
        if c.kind == X3:
            op.A_lo, op.W_lo = whole(a, c.a_rows, True), whole(w, c.w_rows, True)
            op.A, op.W = op.A + op.A_lo[:c.M].astype(F8), op.W + op.W_lo[:c.N].astype(F8)
            op.scale = OUT_SCALE
    if bias:
        op.bias = (rng.standard_normal(c.N) * 0.5).astype(F4)
    if res:
        op.res = (rng.standard_normal((c.M, c.N)) * 2.0).astype(F4)
    return op


GEMM_YARDSTICKS = {EXACT: ("hi_only", "last_k"), X3: ("hi_only",), F16: ()}


def gemm_reference(c: GemmCase, wrong=None, rows=slice(None)):
    """float64 (out, mag) of the launch (rows: a subset of them); wrong = "hi_only": operands rounded to fp16 | "last_k": the last K tile left out"""
    op = gemm_operands(c)
    a, w = op.A[rows].astype(F8), op.W.astype(F8)
    if wrong == "hi_only":
        a, w = (f16(op.A_hi[:c.M][rows]), f16(op.W_hi[:c.N])) if c.kind == X3 else (f16(a), f16(w * (1 / OUT_SCALE)) * OUT_SCALE)
    if wrong == "last_k":
        a = a[:, :c.K - c.tile[2]]
        w = w[:, :c.K - c.tile[2]]
    out = op.scale * (a @ w.T)
    if op.bias is not None:
        out = out + op.bias.astype(F8)
    if FORMS[c.form][1]:
        out = np.maximum(out, 0.0)
    mag = float(np.abs(out).max())
    if op.res is not None:
        out = out + op.res[rows].astype(F8)
    return out, mag


def gemm_emulate(c: GemmCase, rows=slice(None)):
    """The launch in the kernel's number formats -> float64 of what it stores in C32 (C16 alone: the fp16 value); rows: a subset of them"""
    op = gemm_operands(c)
    if c.kind == EXACT:
        acc = chain([(op.A[rows], op.W)], 2)                             # v_mfma_f32_32x32x2_f32
    elif c.kind == X3:
        ah, al, wh, wl = op.A_hi[:c.M][rows], op.A_lo[:c.M][rows], op.W_hi[:c.N], op.W_lo[:c.N]
        acc = chain([(ah, wl), (al, wh), (ah, wh)], 16)                  # v_mfma_f32_32x32x16_f16, the kernel's order of the three
        acc = acc * F4(op.scale)
    else:
        acc = chain([(op.A_hi[:c.M][rows], op.W_hi[:c.N])], 16)
    bias, relu, res, c32, c16, c16lo = FORMS[c.form]
    v = acc
    if bias:
        v = v + op.bias
    if relu:
        v = np.maximum(v, F4(0))
    if res:
        v = v + op.res[rows]
    v = v.astype(F4)
    if c16 and not c32:
        return v.astype(np.float16).astype(F8)
    return v.astype(F8)


@functools.lru_cache(maxsize=None)
def gemm_figures(c: GemmCase, row_stride=1):
    """(bar, emulation's distance, {yardstick: distance}, which term binds); row_stride: the figures are taken over every n-th row (the one large
    case: every 8th — maxima over fewer elements, so if anything a smaller bar)"""
    emu_rows = slice(None, None, row_stride)
    ref, mag = gemm_reference(c, rows=emu_rows)
    emu = rel_err(gemm_emulate(c, emu_rows), ref, mag)
    ys = {w: rel_err(gemm_reference(c, w, emu_rows)[0], ref, mag) for w in GEMM_YARDSTICKS[c.kind]}
    if c.kind == F16:
        return 3.0 * emu, emu, ys, "3 x emulation"
    cap = 1e-2 * min(ys.values())
    return min(4.0 * emu, cap), emu, ys, "4 x emulation" if 4.0 * emu <= cap else "1e-2 x yardstick"


# ================================================================================================================ attention
B_LAYOUTS = 3
V_AMP = (1.0, 4.0, 0.25)       # per layout: a read across a layout boundary shows


@dataclasses.dataclass(frozen=True)
class AttnCase:
    S: int
    H: int
    dh: int
    split: bool = False        # the split engine's form: out16 + out16lo, out32 null (else the exact engine's: out32 only)
    amp: float = 2.5           # standard deviation of the scores: 0.3 a flat softmax, 2.5 a peaked one
    f16: bool = False          # launch_attention16 on the head-padded fp16 layout
    first_run: bool = False    # an instantiation no test of a whole pass reaches

    @property
    def D(self):
        return self.H * self.dh

    @property
    def id(self):
        return f"{'attn16' if self.f16 else 'split' if self.split else 'exact'}-S{self.S}-H{self.H}-dh{self.dh}-amp{self.amp}"

    @property
    def ldo16(self):
        return self.H * 64 + 8 if self.f16 else round_up(self.D, 64 if self.split else 32)      # ldm_create: Dp

    @property
    def kernel(self):
        """launch_attention's dispatch (kernels_attn.hip), restated"""
        S, dh, D = self.S, self.dh, self.D
        ld, ldo32, ldo16 = 3 * D, D, self.ldo16
        if self.f16:
            return "attn_mfma_k"
        if self.split and 1 <= S <= 128 and dh == 58 and D % 2 == 0 and ld % 2 == 0 and ldo16 % 2 == 0:
            return "attention16x3"
        if 96 < S <= 128 and dh == 58 and D % 2 == 0 and ld % 2 == 0 and ldo32 % 2 == 0 and ldo16 % 2 == 0:
            return "attn32_direct_k"
        if 96 < S <= 128 and 56 < dh <= 58:
            return "attn32_mfma_k"
        dhp = round_up(dh, 4)
        return f"attn_rows<float,{32 if dhp <= 32 else 60 if dhp <= 60 else 64}>"


def attention_cases():
    out = []
    for i, S in enumerate((1, 31, 32, 33, 64, 97, 125, 128)):
        out.append(AttnCase(S, 8, 58, split=True, amp=(0.3, 2.5)[i % 2]))
    out += [AttnCase(125, 8, 58, split=True, amp=2.5), AttnCase(125, 16, 58, split=True)]
    out += [AttnCase(97, 8, 58, amp=0.3), AttnCase(125, 8, 58), AttnCase(128, 8, 58, amp=0.3), AttnCase(128, 8, 58)]
    for i, S in enumerate((1, 50, 96, 129, 150)):
        out.append(AttnCase(S, 8, 58, amp=(2.5, 0.3)[i % 2]))
    out.append(AttnCase(129, 8, 58, split=True))
    for dh, S in ((64, 125), (62, 125), (64, 33), (62, 129)):
        out += [AttnCase(S, 8, dh, amp=0.3 if S == 33 else 2.5), AttnCase(S, 8, dh, split=True)]
    # first runs, after everything a whole pass already reaches
    for S in (97, 128):
        out += [AttnCase(S, 16, 57, amp=0.3 if S == 97 else 2.5, first_run=True), AttnCase(S, 16, 57, split=True, first_run=True)]
    for dh, S in ((36, 125), (36, 50), (32, 125), (32, 33), (24, 125), (24, 1)):
        out += [AttnCase(S, 8, dh, amp=0.3 if S == 125 else 2.5, first_run=True), AttnCase(S, 8, dh, split=True, first_run=True)]
    return out


def attention16_cases():
    return [AttnCase(S, 8, dh, f16=True, amp=(0.3, 2.5)[(i + j) % 2]) for i, dh in enumerate((58, 64, 32)) for j, S in enumerate((1, 33, 125, 128))]


ATTN_INSTANTIATIONS = frozenset({"attention16x3", "attn32_direct_k", "attn32_mfma_k", "attn_rows<float,32>", "attn_rows<float,60>",
                                 "attn_rows<float,64>", "attn_mfma_k"})


@functools.lru_cache(maxsize=4)
def attention_operands(c: AttnCase):
    """q, k, v float32 [B, H, S, dh] (attention16: fp16 values)"""
    rng = _rng("attn", c.id)
    sh = (B_LAYOUTS, c.H, c.S, c.dh)
    a = np.sqrt(c.amp)          # q . k / sqrt(dh) then has the standard deviation amp
    q, k = (rng.standard_normal(sh) * a).astype(F4), (rng.standard_normal(sh) * a).astype(F4)
    v = (rng.standard_normal(sh) * np.asarray(V_AMP).reshape(-1, 1, 1, 1)).astype(F4)
    if c.f16:
        q, k, v = (x.astype(np.float16).astype(F4) for x in (q, k, v))
    return q, k, v


def attention_rows(c: AttnCase, q, k, v):
    """[B, H, S, dh] each -> the launch's qkv rows [B S, ld]: q | k | v, head h at columns h * dh (attention16: h * 64, zero padding)"""
    w = 64 if c.f16 else c.dh
    out = np.zeros((B_LAYOUTS * c.S, 3 * c.H * w), np.float16 if c.f16 else F4)
    for i, x in enumerate((q, k, v)):
        for h in range(c.H):
            out[:, (i * c.H + h) * w:(i * c.H + h) * w + c.dh] = x[:, h].reshape(-1, c.dh)
    return out


def attention_heads(c: AttnCase, rows):
    """[B S, >= H w] output rows -> ([B, H, S, dh], the padding columns of the head-padded form or None)"""
    w = 64 if c.f16 else c.dh
    r = np.asarray(rows)[:, :c.H * w].reshape(B_LAYOUTS, c.S, c.H, w).transpose(0, 2, 1, 3)
    return r[..., :c.dh], (r[..., c.dh:] if w > c.dh else None)


def attention_yardsticks(c: AttnCase):
    if c.f16:
        return ()
    return ("hi_only",) if (c.split or c.S == 1) else ("hi_only", "last_k")     # (one key: the softmax is 1 whatever the score)


def attention_reference(c: AttnCase, wrong=None):
    """float64 (out [B, H, S, dh], mag); wrong = "hi_only": q, k, v rounded to fp16 | "last_k": the scores without their last two columns"""
    q, k, v = (x.astype(F8) for x in attention_operands(c))
    if wrong == "hi_only":
        q, k, v = f16(q), f16(k), f16(v)
    qs, ks = (q[..., :c.dh - 2], k[..., :c.dh - 2]) if wrong == "last_k" else (q, k)
    s = qs @ np.swapaxes(ks, -1, -2) / np.sqrt(c.dh)
    p = np.exp(s - s.max(-1, keepdims=True))
    out = (p / p.sum(-1, keepdims=True)) @ v
    return out, float(np.abs(out).max())


def _seq_sum(p):
    acc = np.zeros(p.shape[:-1], F4)
    for j in range(p.shape[-1]):
        acc = acc + p[..., j]
    return acc


def attention_emulate(c: AttnCase):
    q, k, v = attention_operands(c)
    vt = np.swapaxes(v, -1, -2)
    scale = F4(1.0) / np.sqrt(F4(c.dh))
    if c.f16:      # attn_mfma_k: fp16 operands, exp2 of the scaled difference, P rounded to fp16, fp16 out
        s = chain([(q, k)], 16)
        sl = F4(1.4426950408889634) * scale
        mx = s.max(-1, keepdims=True)
        p = np.exp2((s.astype(F8) * sl - mx.astype(F8) * sl).astype(F4)).astype(F4)
        inv = F4(1.0) / _seq_sum(p)
        o = chain([(p.astype(np.float16), vt.astype(np.float16))], 16)
        return (o * inv[..., None]).astype(np.float16).astype(F8)
    if c.kernel == "attention16x3":     # fp16 x 3: unscaled q . k, P scaled by 2^10 before its split
        (qh, ql), (kh, kl), (vh, vl) = (split_x(x) for x in (q, k, vt))
        s = chain([(qh, kl), (ql, kh), (qh, kh)], 16)
        mx = s.max(-1, keepdims=True)
        p = (np.exp(((s - mx) * scale).astype(F4)) * F4(1024.0)).astype(F4)
        inv = F4(1.0) / _seq_sum(p)
        ph, pl = split_x(p)
        o = chain([(ph, vl), (pl, vh), (ph, vh)], 16)
        out = (o * inv[..., None]).astype(F4)
    else:                               # fp32: q scaled first, two passes, unnormalised sum times 1 / l
        s = chain([((q * scale).astype(F4), k)], 2)
        mx = s.max(-1, keepdims=True)
        p = np.exp((s - mx).astype(F4)).astype(F4)
        inv = F4(1.0) / _seq_sum(p)
        o = chain([(p, vt)], 2)
        out = (o * inv[..., None]).astype(F4)
    if c.split:
        hi, lo = split_x(out)
        return hi.astype(F8) + lo.astype(F8)
    return out.astype(F8)


@functools.lru_cache(maxsize=None)
def attention_figures(c: AttnCase):
    ref, mag = attention_reference(c)
    emu = rel_err(attention_emulate(c), ref, mag)
    ys = {w: rel_err(attention_reference(c, w)[0], ref, mag) for w in attention_yardsticks(c)}
    if c.f16:
        return 3.0 * emu, emu, ys, "3 x emulation"
    cap = 1e-2 * min(ys.values())
    return min(4.0 * emu, cap), emu, ys, "4 x emulation" if 4.0 * emu <= cap else "1e-2 x yardstick"


# ================================================================================================================ LayerNorm
LN_FORMS = ("ada", "affine", "gather", "raw")       # AdaLN on rows | gamma / beta on rows | AdaLN on emb[token] + pos[row % S] | raw + stats_out
LN_OUTS = ("y32", "y32_y16_lo", "y32_y16", "y16")   # tiled exact | tiled split | fast AdaLN | fast LayerNorm 2 / head
LN_S = 7                                            # rows per layout of the gather (M = 129: 18 layouts and 3 rows)
LN_CLASSES = 23


@dataclasses.dataclass(frozen=True)
class LnCase:
    D: int
    M: int
    form: str = "ada"
    outs: str = "y32"
    edge: bool = False         # the LayerNorm edge rows in front (M >= 5)

    @property
    def id(self):
        return f"ln-D{self.D}-M{self.M}-{self.form}-{self.outs}{'-edge' if self.edge else ''}"

    @property
    def nv(self):
        return 1 if self.D <= 256 else 2 if self.D <= 512 else 4

    @property
    def ld16(self):
        return self.D + 8

    @property
    def first_run(self):
        return self.nv == 4


def layernorm_cases():
    Ds, Ms = (16, 256, 260, 464, 512, 516, 1024), (1, 3, 4, 5, 129)
    out, i = [], 0
    for D in Ds:
        for M in Ms:
            form = _cycle(LN_FORMS, i)
            out.append(LnCase(D, M, form, "y32" if form == "raw" else _cycle(LN_OUTS, i // 2), edge=(M >= 5 and form in ("ada", "affine"))))
            i += 1
    for D in (256, 464, 1024):          # every form and every output set on each ln_rows<NV>
        for form in ("ada", "affine", "gather"):
            for outs in LN_OUTS:
                c = LnCase(D, 129, form, outs, edge=form != "gather")
                if c not in out:
                    out.append(c)
        if LnCase(D, 129, "raw", "y32") not in out:
            out.append(LnCase(D, 129, "raw", "y32"))
    return sorted(out, key=lambda c: c.first_run)      # ln_rows<4> last


@functools.lru_cache(maxsize=8)
def layernorm_operands(c: LnCase):
    """dict: x [M, D] float32 | tokens, emb, pos; p0, p1 [D] float32"""
    rng = _rng("ln", c.id)
    D, M = c.D, c.M
    op = {}
    if c.form in ("gather", "raw"):
        op["tokens"] = rng.integers(0, LN_CLASSES, M).astype(np.int32)
        op["emb"] = rng.standard_normal((LN_CLASSES, D)).astype(F4)
        op["pos"] = (rng.standard_normal((LN_S, D)) * 0.5).astype(F4)
    else:
        x = rng.standard_normal((M, D)) * np.exp(rng.uniform(np.log(0.3), np.log(3.0), (M, 1)))
        x = x + rng.uniform(-1.0, 1.0, (M, 1))
        if c.edge:
            x[0] = 0.75                                    # constant: variance 0, eps decides
            x[1] = 0.0
            x[1, D // 3] = 1.5                             # one non-zero element
            x[2] = rng.standard_normal(D) * 1e-3
            x[3] = rng.standard_normal(D) * 1e3
            x[4] = rng.standard_normal(D) + 4.0            # offset of 4 standard deviations
        op["x"] = x.astype(F4)
    if c.form in ("ada", "gather"):
        op["p0"], op["p1"] = (rng.standard_normal(D) * 0.3).astype(F4), (rng.standard_normal(D) * 0.3).astype(F4)
    else:
        op["p0"], op["p1"] = (1.0 + rng.standard_normal(D) * 0.3).astype(F4), (rng.standard_normal(D) * 0.3).astype(F4)
    return op


def _ln_x(c, op, dtype):
    if "tokens" in op:
        return op["emb"].astype(dtype)[op["tokens"]] + op["pos"].astype(dtype)[np.arange(c.M) % LN_S]
    return op["x"].astype(dtype)


LN_YARDSTICKS = ("unbiased", "next_pos")


def layernorm_reference(c: LnCase, wrong=None):
    """float64 (y [M, D], stats [M, 2] = mean, rstd, mag); wrong = "unbiased": variance over D - 1 | "next_pos": the gather one position on"""
    op = layernorm_operands(c)
    x = _ln_x(c, op, F8)
    if wrong == "next_pos":
        x = op["emb"].astype(F8)[op["tokens"]] + op["pos"].astype(F8)[(np.arange(c.M) + 1) % LN_S]
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).sum(-1, keepdims=True) / (c.D - 1 if wrong == "unbiased" else c.D)
    rstd = 1.0 / np.sqrt(var + EPS)
    if c.form == "raw":
        y = x
    else:
        g = (1.0 + op["p0"].astype(F8)) if c.form in ("ada", "gather") else op["p0"].astype(F8)
        y = (x - mu) * rstd * g + op["p1"].astype(F8)
    return y, np.concatenate([mu, rstd], -1), float(np.abs(y).max())


def layernorm_yardsticks(c: LnCase):
    return ("unbiased", "next_pos") if c.form == "gather" else ("unbiased",)


def _wave_sum(per_lane):
    v = per_lane
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., np.arange(64) ^ o]
    return v[..., :1]


def layernorm_emulate(c: LnCase):
    """ln_rows in float32, its own summation order: float4 c = 64 i + lane per lane, (x + y) + (z + w), the xor butterfly over the wave"""
    op = layernorm_operands(c)
    x = _ln_x(c, op, F4).astype(F4)
    pad = np.zeros((c.M, c.nv * 256), F4)
    pad[:, :c.D] = x
    lanes = pad.reshape(c.M, c.nv, 64, 4)
    live = (np.arange(c.nv * 256) < c.D).reshape(1, c.nv, 64, 4)

    def per_lane(v):
        acc = np.zeros((c.M, 64), F4)
        for i in range(c.nv):
            acc = acc + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
        return acc

    inv_d = F4(1.0) / F4(c.D)
    mean = _wave_sum(per_lane(lanes)) * inv_d
    dx = np.where(live, lanes - mean[..., None, None], F4(0))
    var = _wave_sum(per_lane(dx * dx)) * inv_d
    rstd = F4(1.0) / np.sqrt(var + F4(EPS))
    stats = np.concatenate([mean, rstd], -1).astype(F8)
    if c.form == "raw":
        return x.astype(F8), stats
    g = (F4(1.0) + op["p0"]) if c.form in ("ada", "gather") else op["p0"]
    y = ((x - mean) * rstd * g + op["p1"]).astype(F4)
    return y.astype(F8), stats


@functools.lru_cache(maxsize=None)
def layernorm_figures(c: LnCase):
    """(bar of y, emulation's distance, yardsticks, binding term, bar of the statistics)"""
    y, st, mag = layernorm_reference(c)
    ye, ste = layernorm_emulate(c)
    if c.form == "raw":
        ys = {w: stats_err(layernorm_reference(c, w)[1], st) for w in layernorm_yardsticks(c)}
    else:
        ys = {w: rel_err(layernorm_reference(c, w)[0], y, mag) for w in layernorm_yardsticks(c)}
    cap = 1e-2 * min(ys.values())
    emu_s = float((np.abs(ste - st) / _stat_mag(st)).max())
    if c.form == "raw":        # y32 receives emb + pos, one fp32 addition: bit for bit; the bar is the statistics'
        return min(4.0 * emu_s, cap), emu_s, ys, "4 x emulation" if 4.0 * emu_s <= cap else "1e-2 x yardstick", min(4.0 * emu_s, cap)
    emu = rel_err(ye, y, mag)
    return min(4.0 * emu, cap), emu, ys, "4 x emulation" if 4.0 * emu <= cap else "1e-2 x yardstick", 4.0 * emu_s


def _stat_mag(st):
    return np.abs(st).max(0, keepdims=True)     # mean and rstd each against its own largest value


def stats_err(got, st):
    return float((np.abs(np.asarray(got, F8) - st) / _stat_mag(st)).max())


# ================================================================================================================ the set the issue names
GEMM_INSTANTIATIONS = frozenset({"gemm_f32_tile<2>"} | {f"gemm16x3_k<256,256,32,2,tag {t}>" for t in range(4)} | {"gemm16x3_k<256,128,32,3,tag 4>"} |
                                {f"gemm16_k<128,128,64,2,tag {t}>" for t in range(5)})
LN_INSTANTIATIONS = frozenset({"ln_rows<1>", "ln_rows<2>", "ln_rows<4>"})
ALL_INSTANTIATIONS = GEMM_INSTANTIATIONS | ATTN_INSTANTIATIONS | LN_INSTANTIATIONS


def hi_lo_slack(ref):
    """What hi + lo itself is from the fp32 value it splits: two 11-bit halves carry 22 bits, and lo ends at fp16's denormal spacing"""
    return 2.0 ** -22 * np.abs(ref) + 2.0 ** -24


def hi_within_one_ulp(hi16, ref, slack):
    """hi alone against fp16(ref): at most one fp16 ulp apart, beyond `slack` = bar x mag (the fp32 value that is rounded is itself that far
    from the reference, which moves a small element by more than its own ulp)"""
    r16 = np.asarray(ref).astype(np.float16)
    ulp = np.spacing(np.maximum(np.abs(r16), np.float16(6.104e-5))).astype(F8)      # (denormals: the smallest normal's spacing)
    return bool((np.abs(np.asarray(hi16).astype(F8) - r16.astype(F8)) <= ulp + slack).all())
