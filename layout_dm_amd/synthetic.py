"""Model geometry, diffusion schedule and deterministic synthetic checkpoints for the product side
(bench.py, the drop-in model class when no checkpoint is given).

The geometry/schedule mirror the reference:
  vocab layout     trainer/helpers/layout_tokenizer.py:79-82,152-153,429-467
  sub-vocab sizes  trainer/models/categorical_diffusion/constrained.py:51-54
  backbone dims    trainer/config/backbone/medium.yaml + models/layoutdm.py:54 (shrink 29/32)
  schedule         trainer/models/categorical_diffusion/util.py:47-70, base.py:44-47
  init             trainer/models/base_model.py:108-116, models/common/nn_lib.py:109-110
(oracle/spec.py + oracle/synth.py hold an independent copy used by the checker;
tests/test_synthetic_consistency.py asserts both produce identical tensors.)
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

LOG_EPS = math.log(1e-30)  # util.py:8
VAR_NAMES = ("c", "x", "y", "w", "h")


@dataclasses.dataclass(frozen=True)
class ModelSpec:
    name: str
    n_category: int
    n_bin: int = 32
    max_elem: int = 25
    n_attr: int = 5
    d_model: int = 464
    n_head: int = 8
    d_ff: int = 1856
    n_layer: int = 4
    n_step: int = 100  # T

    @property
    def seq_len(self) -> int:  # S
        return self.max_elem * self.n_attr

    @property
    def n_bbox(self) -> int:
        return self.n_bin * 4

    @property
    def pad_id(self) -> int:
        return self.n_category + self.n_bbox

    @property
    def mask_id(self) -> int:
        return self.pad_id + 1

    @property
    def n_class(self) -> int:  # C
        return self.mask_id + 1

    @property
    def d_head(self) -> int:
        return self.d_model // self.n_head

    def sub_vocab_size(self, attr: int) -> int:  # K, constrained.py:51-54
        return (self.n_category if attr == 0 else self.n_bin) + 2

    def full_ids(self, attr: int) -> np.ndarray:
        """partial index -> full vocabulary id (layout_tokenizer.py:429-467)."""
        if attr == 0:
            body = np.arange(self.n_category)
        else:
            start = self.n_category + (attr - 1) * self.n_bin
            body = np.arange(start, start + self.n_bin)
        return np.concatenate([body, [self.pad_id, self.mask_id]]).astype(np.int64)


RICO25 = ModelSpec("rico25", n_category=25)
PUBLAYNET = ModelSpec("publaynet", n_category=5)
SPECS = {"rico25": RICO25, "publaynet": PUBLAYNET}


def alpha_schedule(num_timesteps, N, att_1=0.99999, att_T=0.000009, ctt_1=0.000009, ctt_T=0.99999):
    """Restatement of util.py:47-70 (float64 numpy)."""
    att = np.arange(0, num_timesteps) / (num_timesteps - 1) * (att_T - att_1) + att_1
    att = np.concatenate(([1], att))
    at = att[1:] / att[:-1]
    ctt = np.arange(0, num_timesteps) / (num_timesteps - 1) * (ctt_T - ctt_1) + ctt_1
    ctt = np.concatenate(([0], ctt))
    one_minus_ctt = 1 - ctt
    one_minus_ct = one_minus_ctt[1:] / one_minus_ctt[:-1]
    ct = 1 - one_minus_ct
    bt = (1 - at - ct) / N
    att = np.concatenate((att[1:], [1]))
    ctt = np.concatenate((ctt[1:], [0]))
    btt = (1 - att - ctt) / N
    return at, bt, ct, att, btt, ctt


SCHEDULE_NAMES = (
    "log_at", "log_bt", "log_ct", "log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct",
    "log_1_min_ct", "log_1_min_cumprod_ct",
)


def schedule_buffers(spec: ModelSpec):
    """{f"{key}_{name}": float32 array} as registered at constrained.py:56-90.

    torch.log / log_1_min_a (util.py:15-16) are evaluated in float64 then cast to
    float32, exactly as the reference does (torch.tensor(float64) -> .float()).
    """
    out = {}
    with np.errstate(divide="ignore"):
        for a, key in enumerate(VAR_NAMES):
            N = spec.sub_vocab_size(a) - 1
            at, bt, ct, att, btt, ctt = alpha_schedule(spec.n_step, N)
            log_at, log_bt, log_ct = np.log(at), np.log(bt), np.log(ct)
            l_att, l_btt, l_ctt = np.log(att), np.log(btt), np.log(ctt)
            log_1_min_ct = np.log(1 - np.exp(log_ct) + 1e-40)
            log_1_min_cumprod_ct = np.log(1 - np.exp(l_ctt) + 1e-40)
            vals = (log_at, log_bt, log_ct, l_att, l_btt, l_ctt, log_1_min_ct, log_1_min_cumprod_ct)
            for n, v in zip(SCHEDULE_NAMES, vals):
                out[f"{key}_{n}"] = v.astype(np.float32)
    return out


PREFIX = "model.module."  # CustomDataParallel wrapper, models/layoutdm.py:52


def synth_state_dict(spec: ModelSpec, seed: int = 0, perturb: bool = False, prefix: str = PREFIX,
                     weight_std: float = 0.02, pos_emb: str = "elem_attr", timestep_type="adalayernorm"):
    """Returns {key: np.ndarray(float32)} with the 100 reference keys.

    pos_emb / timestep_type: the denoiser variants of the reference's constructor — exactly the key set and shapes of its
    state_dict() for that variant (the defaults draw what they always drew):
      pos_emb="default"                          transformer.pos_emb.pos_emb (S, D) instead of elem_emb / attr_emb (nn_lib.py:73-88)
      timestep_type "adalayernorm" / "adainnorm"       norm1.emb.weight + norm1.linear.*   (the two share their keys)
      timestep_type "adalayernorm_abs" / "adainnorm_abs"   norm1.linear.* only: the sinusoid has no parameters (transformer_utils.py:34-49)
      timestep_type None                         norm1.weight / norm1.bias, a plain nn.LayerNorm (transformer_utils.py:155)"""
    if pos_emb not in ("elem_attr", "default"):
        raise ValueError(f"pos_emb={pos_emb}")
    if timestep_type not in ("adalayernorm", "adainnorm", "adalayernorm_abs", "adainnorm_abs", None):
        raise ValueError(f"timestep_type={timestep_type}")
    rng = np.random.default_rng(seed)
    D, F, C, T = spec.d_model, spec.d_ff, spec.n_class, spec.n_step

    def normal(*shape):
        return (rng.standard_normal(shape) * weight_std).astype(np.float32)

    def bias(n):
        if perturb:
            return (rng.standard_normal(n) * 0.1).astype(np.float32)
        return np.zeros(n, np.float32)

    def gamma(n):
        if perturb:
            return (1.0 + rng.standard_normal(n) * 0.1).astype(np.float32)
        return np.ones(n, np.float32)

    sd = {}
    sd["Lt_history"] = np.zeros(T, np.float32)
    sd["Lt_count"] = np.zeros(T, np.float32)
    sd.update(schedule_buffers(spec))
    tr = "transformer."
    sd[tr + "cat_emb.weight"] = normal(C, D)
    if pos_emb == "default":
        sd[tr + "pos_emb.pos_emb"] = rng.random((spec.seq_len, D)).astype(np.float32)
    else:
        sd[tr + "pos_emb.elem_emb"] = rng.random((spec.max_elem, D)).astype(np.float32)
        sd[tr + "pos_emb.attr_emb"] = rng.random((spec.n_attr, D)).astype(np.float32)
    for i in range(spec.n_layer):
        b = f"{tr}backbone.layers.{i}."
        sd[b + "self_attn.in_proj_weight"] = normal(3 * D, D)
        sd[b + "self_attn.in_proj_bias"] = bias(3 * D)
        sd[b + "self_attn.out_proj.weight"] = normal(D, D)
        sd[b + "self_attn.out_proj.bias"] = bias(D)
        sd[b + "linear1.weight"] = normal(F, D)
        sd[b + "linear1.bias"] = bias(F)
        sd[b + "linear2.weight"] = normal(D, F)
        sd[b + "linear2.bias"] = bias(D)
        if timestep_type is None:
            sd[b + "norm1.weight"] = gamma(D)
            sd[b + "norm1.bias"] = bias(D)
        else:
            if not timestep_type.endswith("_abs"):
                sd[b + "norm1.emb.weight"] = normal(T, D)
            sd[b + "norm1.linear.weight"] = normal(2 * D, D)
            sd[b + "norm1.linear.bias"] = bias(2 * D)
        sd[b + "norm2.weight"] = gamma(D)
        sd[b + "norm2.bias"] = bias(D)
    sd[tr + "head.0.weight"] = gamma(D)
    sd[tr + "head.0.bias"] = bias(D)
    sd[tr + "head.1.weight"] = normal(C, D)
    return {prefix + k: v for k, v in sd.items()}


# "trained-like" weight distributions: the reference's init (sigma 0.02, gains 1) is the easy point for fp16 arithmetic and a
# power-bound kernel's clock depends on operand statistics, so bench.py also times the headline on a wide point
# (tests/test_synthetic_consistency.py keeps this equal to the oracle's copy, on which the reference-produced goldens stand)
TRAINED_LIKE = {"init": 0.02, "mid": 0.06, "wide": 0.15}


def trained_like_state_dict(spec: ModelSpec, point: str, seed: int = 0, prefix: str = PREFIX, ln_spread: float = 0.5,
                            n_outlier: int = 4, outlier_gain: float = 8.0, adaln_gain: float = 5.0):
    """Linear / Embedding sigma of TRAINED_LIKE[point], LayerNorm gains ~ U[1 - ln_spread, 1 + ln_spread], `n_outlier`
    output channels of every residual write scaled by `outlier_gain`, AdaLN timestep embeddings by `adaln_gain`."""
    sd = synth_state_dict(spec, seed=seed, perturb=True, prefix="", weight_std=TRAINED_LIKE[point])
    rng = np.random.default_rng(seed + 1000)
    for k in sorted(sd):
        v = sd[k]
        if k.endswith("norm2.weight") or k.endswith("head.0.weight"):
            sd[k] = (1.0 + ln_spread * rng.uniform(-1.0, 1.0, v.shape)).astype(np.float32)
        elif k.endswith("norm1.emb.weight"):
            sd[k] = (v * adaln_gain).astype(np.float32)
        elif k.endswith("linear2.weight") or k.endswith("out_proj.weight"):
            ch = rng.choice(v.shape[0], n_outlier, replace=False)
            v = v.copy()
            v[ch] *= outlier_gain
            sd[k] = v
    return {prefix + k: v for k, v in sd.items()}


def strip_prefix(sd):
    """Accept either LayoutDM ('model.module.') or bare diffusion-module keys."""
    out = {}
    for k, v in sd.items():
        for p in (PREFIX, "module.", "model."):
            if k.startswith(p):
                k = k[len(p):]
                break
        out[k] = v
    return out




def synth_cond_c(spec: ModelSpec, batch: int, seed: int = 0):
    """Synthetic cond=c inputs shaped exactly like helpers/task.py:94-110 output: per layout
    n ~ U{1..max_elem} elements; categories kept, other attributes of valid elements = mask_id, padded elements =
    pad_id; mask=True on category slots of valid elements and on every slot of padded elements."""
    rng = np.random.default_rng(seed + 77)
    S, A = spec.seq_len, spec.n_attr
    seq = np.full((batch, S), spec.pad_id, np.int64)
    mask = np.ones((batch, S), bool)
    n_elem = rng.integers(1, spec.max_elem + 1, size=batch)
    for b in range(batch):
        n = int(n_elem[b])
        cats = rng.integers(0, spec.n_category, size=n)
        for e in range(n):
            seq[b, e * A] = cats[e]
            seq[b, e * A + 1:(e + 1) * A] = spec.mask_id
            mask[b, e * A + 1:(e + 1) * A] = False
    return {"seq": seq, "mask": mask, "type": "c", "num_element": n_elem}


def linear_bin_centres(n_bin: int) -> np.ndarray:
    """(4, n_bin) box-coordinate centres of the linear quantisation in x, y, w, h order (helpers/bbox_tokenizer.py:
    x / y bins start at 0, w / h bins at 1 / n_bin — the `DummyClusteringModel` the reference builds for
    bbox_quantization=linear)."""
    lo = np.linspace(0.0, 1.0 - 1.0 / n_bin, n_bin)
    hi = np.linspace(1.0 / n_bin, 1.0, n_bin)
    return np.stack([lo, lo, hi, hi])


def synth_cond_refinement(spec: ModelSpec, batch: int, seed: int = 0, refine_lambda: float = 3.0,
                          offset_ratio: float = 0.1):
    """Synthetic cond=refinement inputs shaped like helpers/task.py:127-138 + set_additional_conditions_for_refinement
    (task.py:204-224, `uniform` mode): a random full layout as the noisy `seq_orig`; `seq` keeps its categories, [MASK]
    on the other attributes of valid elements, [PAD] on padded elements; `mask` = category slots + padded slots;
    `weak_logits` (B, C, S) = refine_lambda * Table[seq_orig] with Table = identity outside the coordinate
    vocabularies and 1[|centre_i - centre_j| < offset_ratio] inside each of them."""
    rng = np.random.default_rng(seed + 177)
    S, A, C, N = spec.seq_len, spec.n_attr, spec.n_class, spec.n_bin
    c = synth_cond_c(spec, batch, seed=seed + 1)
    seq_orig = c["seq"].copy()
    for a in range(1, A):  # a random bin of the attribute's own sub-vocabulary on every valid element
        start = spec.n_category + (a - 1) * N
        col = seq_orig[:, a::A]
        valid = col == spec.mask_id
        col[valid] = start + rng.integers(0, N, size=int(valid.sum()))
    table = np.eye(C, dtype=np.float32)
    cen = linear_bin_centres(N)
    for i in range(4):
        sl = slice(spec.n_category + i * N, spec.n_category + (i + 1) * N)
        table[sl, sl] = (np.abs(cen[i][:, None] - cen[i][None, :]) < offset_ratio).astype(np.float32)
    weak = (table[seq_orig].transpose(0, 2, 1) * refine_lambda).astype(np.float32)  # (B, C, S)
    return {"seq": c["seq"], "mask": c["mask"], "type": "refinement", "seq_orig": seq_orig,
            "weak_logits": np.ascontiguousarray(weak)}


def synth_cond_relation(spec: ModelSpec, batch: int, seed: int = 0, edge_ratio: float = 0.1):
    """Synthetic cond=relation inputs: cond=c sequences plus relation graphs in the reference's format (AddCanvasElement
    + AddRelationConstraints(edge_ratio), trainer/data/util.py:111-177): node 0 of every layout is the canvas, every
    pair of nodes carries an edge with probability edge_ratio, edge_attr = 1 << size relation | 1 << location relation
    (sizes 0..3; locations 4..9 between elements, 4..6 + 9 against the canvas are all accepted by the losses).
    Returns (cond, graph): graph = {y, edge_index (2, E) GLOBAL node ids, edge_attr, batch} as numpy arrays."""
    rng = np.random.default_rng(seed + 277)
    c = synth_cond_c(spec, batch, seed=seed + 2)
    A = spec.n_attr
    ys, src, dst, attr, bt = [], [], [], [], []
    off = 0
    for b in range(batch):
        n = int(c["num_element"][b])
        ys.append(np.concatenate([[0], c["seq"][b, 0:n * A:A] + 1]))
        ii, jj = np.triu_indices(n + 1, k=1)
        keep = rng.random(ii.size) < edge_ratio
        ii, jj = ii[keep], jj[keep]
        src.append(off + ii)
        dst.append(off + jj)
        attr.append((1 << rng.integers(0, 4, size=ii.size)) | (1 << rng.integers(4, 10, size=ii.size)))
        bt.append(np.full(n + 1, b))
        off += n + 1
    graph = {"y": np.concatenate(ys).astype(np.int64),
             "edge_index": np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64),
             "edge_attr": np.concatenate(attr).astype(np.int64), "batch": np.concatenate(bt).astype(np.int64)}
    cond = {"seq": c["seq"], "mask": c["mask"], "type": "relation"}
    return cond, graph


def synth_fid_state_dict(num_label: int, seed: int = 0, max_bbox: int = 25):
    """Random FIDNetV3 encoder weights (trainer/fid/model.py:123-164 key names; 256-d, 4 heads, FFN 128, 4 layers) for
    timing the feature extractor without a checkpoint."""
    D, FF, LAYERS = 256, 128, 4
    rng = np.random.default_rng(seed + 4242)
    w = lambda *s: (rng.standard_normal(s) * 0.05).astype(np.float32)
    b = lambda n: (rng.standard_normal(n) * 0.1).astype(np.float32)
    g = lambda n: (1.0 + rng.standard_normal(n) * 0.1).astype(np.float32)
    sd = {"emb_label.weight": (rng.standard_normal((num_label, D)) * 0.5).astype(np.float32),
          "fc_bbox.weight": (rng.standard_normal((D, 4)) * 0.5).astype(np.float32), "fc_bbox.bias": b(D),
          "enc_fc_in.weight": w(D, 2 * D), "enc_fc_in.bias": b(D),
          "enc_transformer.token": rng.standard_normal((1, 1, D)).astype(np.float32)}
    for i in range(LAYERS):
        p = f"enc_transformer.core.layers.{i}."
        sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"] = w(3 * D, D), b(3 * D)
        sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"] = w(D, D), b(D)
        sd[p + "linear1.weight"], sd[p + "linear1.bias"] = w(FF, D), b(FF)
        sd[p + "linear2.weight"], sd[p + "linear2.bias"] = w(D, FF), b(D)
        sd[p + "norm1.weight"], sd[p + "norm1.bias"] = g(D), b(D)
        sd[p + "norm2.weight"], sd[p + "norm2.bias"] = g(D), b(D)
    return sd


def synth_boxes(n: int, seed: int = 0, width: int = 1440, height: int = 2560) -> np.ndarray:
    """(n, 4) float32 xc, yc, w, h of layout-like boxes: pixel-aligned on a width x height canvas (so coordinates repeat, as a
    dataset's do), narrow heights, a share of full-width elements — the input of the coordinate-bin fits when no dataset is at
    hand (tools/clustering_bench.py)."""
    g = np.random.default_rng(seed)
    w = np.clip(np.round(g.beta(1.2, 2.5, n) * width), 1, width)
    h = np.clip(np.round(g.beta(1.0, 6.0, n) * height), 1, height)
    full = g.random(n) < 0.15
    w[full] = width
    x0 = np.round(g.random(n) * (width - w))
    y0 = np.round(g.random(n) * (height - h))
    return np.stack([(x0 + w / 2) / width, (y0 + h / 2) / height, w / width, h / height], axis=1).astype(np.float32)
