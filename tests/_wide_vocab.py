"""Shared pieces of the wide-vocabulary tests (more than 192 classes: 64 and 128 bins per coordinate, served by the exact and
split engines): the edge vocabularies, the tiny backbone, synthetic weights, and sampler cases on rows of up to 576 classes
(tests/_sampler_cases.py assumes rows of at most 192)."""
import functools

import numpy as np
import torch

from oracle import restatement as R
from oracle import spec as SP
from oracle import synth

# (categories, bins) -> classes
VOCABS = [(1, 48),     # 195: the first size past the fp16 engines' cap, 7 head tiles
          (25, 64),    # 283: 9 head tiles, padded to 10 on the row-resident kernels
          (5, 128),    # 519
          (62, 128)]   # 576: every lane slot of the full-vocabulary form taken, Cp == C
VOCAB_IDS = [f"c{c}_b{b}" for c, b in VOCABS]
SEED, FIRST_LAYOUT = 20240611, 700
KINDS = {"deterministic": 0, "random": 1, "top_p": 2, "top_k": 3, "gumbel": 4}


def tiny_spec(n_category, n_bin, n_step=10):
    return SP.ModelSpec(f"wide_{n_category}_{n_bin}", n_category=n_category, n_bin=n_bin, max_elem=4, d_model=64, n_head=4,
                        d_ff=128, n_layer=2, n_step=n_step)


@functools.lru_cache(maxsize=None)
def tiny_model(n_category, n_bin, q_type="constrained"):
    """(spec, state dict, oracle weights) of the tiny backbone on one vocabulary; computed once and shared (never written)."""
    spec = tiny_spec(n_category, n_bin)
    sd = synth.synth_state_dict(spec, seed=1, perturb=True, q_type=q_type)
    return spec, sd, R.as_torch_weights(sd)


def states(spec, B=3, seed=0, p_mask=0.4, p_pad=0.15):
    """(B, S) int64 states of the reverse chain: body tokens of each position's sub-vocabulary, [MASK] and [PAD] mixed in."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.empty(B, spec.seq_len, dtype=torch.long)
    for a in range(spec.n_attr):
        ids = torch.as_tensor(spec.full_ids(a))
        tok[:, a::spec.n_attr] = ids[torch.randint(0, len(ids) - 2, (B, spec.max_elem), generator=g)]
    r = torch.rand(B, spec.seq_len, generator=g)
    tok[r < p_mask] = spec.mask_id
    tok[(r >= p_mask) & (r < p_mask + p_pad)] = spec.pad_id
    return tok


def sampler_cfgs(spec, logp):
    """The samplers' settings at their edges on rows of spec.n_class classes: top_p below the largest probability any row of
    logp holds (only the first maximum survives) and = 1; top_k 1, = the widest live set, above it; temperature 0.05."""
    live = max(spec.sub_vocab_size(a) for a in range(spec.n_attr))
    p_max_min = float(torch.softmax(logp.double(), dim=1).max(dim=1).values.min())
    return [("deterministic", {"name": "deterministic"}),
            ("random", {"name": "random", "temperature": 1.0}),
            ("random_T0.05", {"name": "random", "temperature": 0.05}),
            ("top_p_below_max", {"name": "top_p", "top_p": 0.5 * p_max_min, "temperature": 1.0}),
            ("top_p0.9", {"name": "top_p", "top_p": 0.9, "temperature": 1.0}),
            ("top_p1.0", {"name": "top_p", "top_p": 1.0, "temperature": 1.0}),
            ("top_k1", {"name": "top_k", "top_k": 1, "temperature": 1.0}),
            ("top_k_live", {"name": "top_k", "top_k": live, "temperature": 1.0}),
            ("top_k_above_live", {"name": "top_k", "top_k": min(live + 7, spec.n_class), "temperature": 0.7}),
            ("gumbel", {"name": "gumbel", "temperature": 0.7})]


def oracle_draw(logp, cfg, step):
    """R.sample_tokens on the kernel's own uniforms (and, gumbel, its per-class noise words)."""
    B, C, S = logp.shape
    if cfg["name"] == "deterministic":
        return R.sample_tokens(logp, cfg)
    u = R.token_uniforms(SEED, FIRST_LAYOUT, B, S, step)[..., 0]
    gu = R.token_gumbel_uniforms(SEED, FIRST_LAYOUT, B, S, step, C) if cfg["name"] == "gumbel" else None
    return R.sample_tokens(logp, cfg, uniforms=u, gumbel_uniforms=gu)


def inverse_cdf(lg, u):
    """The oracle's inverse-CDF rule on already filtered logits (B,C,S) float32."""
    cdf = torch.cumsum(torch.softmax(lg, dim=1).double(), dim=1)
    thr = torch.as_tensor(u, dtype=torch.float64).view(lg.shape[0], 1, -1) * cdf[:, -1:, :]
    return (cdf <= thr).sum(dim=1).clamp(max=lg.shape[1] - 1)


def top_p_one_cut_is_rounding(out, ref, logp, cfg, step):
    """top_p = 1.0: the reference drops every class whose float32 cumulative probability (descending order) EXCEEDS 1.0 — decided
    by the rounding of the sum alone, a summation-order artefact (tests/_sampler_cases.py top_p_one_mismatch, whose rule this is
    with the row length as the number of roundings: C instead of 192).  A token is admitted if it is the inverse-CDF draw after
    cutting nothing, or after cutting a tail of the descending order that lies wholly within C roundings of 2^-24 of 1.0
    (cumulative probabilities in float64).  -> number of tokens that are neither."""
    assert cfg["name"] == "top_p" and cfg["top_p"] == 1.0
    B, C, S = logp.shape
    u = R.token_uniforms(SEED, FIRST_LAYOUT, B, S, step)[..., 0]
    lg = (logp / cfg.get("temperature", 1.0)).float()
    s_lg, s_idx = torch.sort(lg, descending=True, dim=1, stable=True)
    p64 = torch.softmax(s_lg.double(), dim=1)
    zone = (torch.cumsum(p64, dim=1) > 1.0 - C * 2.0 ** -24) & (torch.arange(C).view(1, C, 1) > 0)
    n_pos = (p64 > 1e-20).sum(dim=1, keepdim=True)
    rank = s_idx.argsort(dim=1)
    ok = out == ref
    for m in range(4):
        cut = ((torch.arange(C).view(1, C, 1) >= n_pos - m) & zone).gather(1, rank)
        ok |= inverse_cdf(lg.masked_fill(cut, -float("inf")), u) == out
    return int((~ok).sum())


def sched_rows(spec, W, t_post, q_type="constrained"):
    """(n_attr, 10) float32: the StepSchedule of every attribute at t_post (ldm_post_token.h)."""
    T = spec.n_step
    u = (t_post - 1 + (T + 1)) % (T + 1)
    out = np.zeros((spec.n_attr, 10), np.float32)
    for a, key in enumerate(SP.VAR_NAMES):
        pre = "" if q_type == "vanilla" else key + "_"
        g = lambda n, i: float(W[f"{pre}{n}"][i])   # noqa: E731
        out[a] = [g("log_at", t_post), g("log_bt", t_post), g("log_ct", t_post), g("log_cumprod_at", t_post),
                  g("log_cumprod_bt", t_post), g("log_cumprod_ct", t_post), g("log_cumprod_at", u), g("log_cumprod_bt", u),
                  g("log_cumprod_ct", u), g("log_1_min_cumprod_ct", u)]
    return out
