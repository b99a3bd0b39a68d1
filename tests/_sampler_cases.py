"""Shared by tests/test_post_token_scalar.py (host form) and tests/test_sampler_edges_gpu.py (device forms): the
parameter-edge matrix of the stochastic samplers, the teacher-forced states it runs on, and the oracle side of a draw on
identical Philox words (draw uniform + per-class gumbel uniforms)."""
import math
import os

import numpy as np
import torch

from oracle import restatement as R
from oracle import spec as SP
from oracle import synth

WEIGHT_SEED = 1
SEED, FIRST_LAYOUT = 1234567890123, 500
STATE_STEPS = (0, 3, 20, 40, 60, 80, 95, 99)      # loop indices of the golden trajectories (t = 99 - index)


def weights(ds):
    spec = SP.SPECS[ds]
    return spec, R.as_torch_weights(synth.synth_state_dict(spec, seed=WEIGHT_SEED, perturb=True))


def max_live_temperature(C: int) -> float:
    """Largest temperature at which the C - live dead classes of a token (log-probability log(1e-30) each, divided by the
    temperature like every other class: helpers/sampling.py:90) together hold at most 2^-24 of the mass, the resolution
    of the draw's uniform: C * exp(log(1e-30) / T) <= 2^-24  <=>  T <= -log(1e-30) / log(2^24 * C).  The live-class
    forms of the step (ldm_sample_step / ldm_sample_loop) leave the dead classes out and refuse anything above."""
    return -SP.LOG_EPS / math.log(2.0 ** 24 * C)


def admitted_temperature(C: int) -> float:
    """A float32 temperature just inside max_live_temperature (0.1 % below it)."""
    return float(np.float32(max_live_temperature(C) * 0.999))


def edge_cfgs(spec):
    """(id, sampling cfg) of the parameter edges: top_k = 1, at / one above every sub-vocabulary size (category + 2 and
    bin + 2 live classes) and = C; top_p = 1 and below any largest probability (a row of <= 192 classes has a maximum of
    >= 1/192); temperatures 0.05 (the runners-up's exponentials underflow), 0.6 / 1.3 and top_k 5 at 0.7 (the settings of
    the reference-made probabilities in rico25_cond_variants.npz) and the largest the live-class forms admit."""
    C = spec.n_class
    tmax = admitted_temperature(C)
    ks = sorted({spec.sub_vocab_size(0), spec.sub_vocab_size(0) + 1, spec.sub_vocab_size(1), spec.sub_vocab_size(1) + 1, C})
    out = [("top_k1", {"name": "top_k", "top_k": 1, "temperature": 1.0})]
    out += [(f"top_k{k}", {"name": "top_k", "top_k": k, "temperature": 1.0}) for k in ks]
    out += [("top_k5_T0.7", {"name": "top_k", "top_k": 5, "temperature": 0.7}),
            ("top_p1.0", {"name": "top_p", "top_p": 1.0, "temperature": 1.0}),
            ("top_p1e-3", {"name": "top_p", "top_p": 1e-3, "temperature": 1.0}),
            ("top_p0.8_T1.3", {"name": "top_p", "top_p": 0.8, "temperature": 1.3}),
            ("random_T0.05", {"name": "random", "temperature": 0.05}),
            ("random_T0.6", {"name": "random", "temperature": 0.6}),
            ("random_T1.3", {"name": "random", "temperature": 1.3}),
            ("random_Tmax", {"name": "random", "temperature": tmax}),
            ("top_p0.9_Tmax", {"name": "top_p", "top_p": 0.9, "temperature": tmax}),
            ("gumbel_Tmax", {"name": "gumbel", "temperature": tmax})]
    return out


def load_states(golden_dir, ds, steps=STATE_STEPS):
    """[(loop index, t, tokens (B,S) int64)], cond dict or None: states the reference's own stochastic runs visited."""
    if ds == "rico25":
        g, cond = np.load(os.path.join(golden_dir, "rico25_uncond_trajectory.npz")), None
    else:
        g = np.load(os.path.join(golden_dir, "publaynet_cond_c_trajectory.npz"))
        cond = {"seq": g["cond_seq"].astype(np.int64), "mask": g["cond_mask"], "type": "c"}
    return [(i, int(g["steps"][i]), torch.from_numpy(g["states_before"][i].astype(np.int64))) for i in steps], cond


def oracle_logp(W, spec, tokens, t, cond=None):
    """log p(x_{t-1} | x_t) over all C classes after the cond overrides: what R.single_step hands to its draw."""
    return R.single_step(W, spec, tokens, t, {"name": "deterministic"}, cond, return_all=True)[2]


def oracle_draw(logp, cfg, step, seed=SEED, first_layout=FIRST_LAYOUT):
    """R.sample_tokens on the Philox words of (seed, layout, step, position): the draw of R.single_step, noise included."""
    B, C, S = logp.shape
    u = R.token_uniforms(seed, first_layout, B, S, step)[..., 0]
    gu = R.token_gumbel_uniforms(seed, first_layout, B, S, step, C) if cfg["name"] == "gumbel" else None
    return R.sample_tokens(logp, cfg, uniforms=u, gumbel_uniforms=gu)


def support(logp, cfg, slack: float = 0.0):
    """(B,C,S) bool: classes the oracle can draw at all (gumbel noise is finite: the support of `random`).
    slack = 0: exactly the oracle's.  slack > 0, for a numerics mode whose log-probabilities carry an error of up to
    `slack` per class (the fast mode: 1e-3 absolute, which is why test_hip_parity.py's MARGIN_BOUND lets two classes
    closer than 2e-3 change places): a class also counts when errors of that size could put it inside.  Two values closer than d = 2 slack / T can change places in the descending order, and every
    probability moves by a relative d at most.  top-k: value within d of the k-th largest.  top-p: the classes that stay
    ahead of the class whatever the error (value more than d above its own) plus the class itself hold no more than
    top_p + d — or no class stays ahead of it at all: the first of the order survives any top_p (sampling.py:107-108)."""
    if slack > 0 and cfg["name"] in ("top_k", "top_p"):
        T = cfg.get("temperature", 1.0)
        lg = (logp / T).float()
        d = 2 * slack / T
        if cfg["name"] == "top_k":
            kth = torch.topk(lg, cfg["top_k"], 1).values[:, -1:, :]
            return lg >= kth - d
        p = torch.softmax(lg.double(), dim=1)
        ahead = lg.unsqueeze(1) > lg.unsqueeze(2) + d                    # [b, c, j, s]: j surely precedes c
        mass = (ahead * p.unsqueeze(1)).sum(dim=2) + p
        return (mass <= cfg["top_p"] + d) | ~ahead.any(dim=2) | (R.sample_probs(logp, cfg) > 0)
    return R.sample_probs(logp, cfg) > 0


def top_p_one_mismatch(out, logp, cfg, step, seed=SEED, first_layout=FIRST_LAYOUT):
    """top_p = 1.0: nothing but rounding may be cut.  The reference drops every class whose float32 cumulative
    probability (descending order) EXCEEDS top_p; at 1.0 that is decided by the rounding of the sum alone, and torch's own
    float32 cumsum does overshoot 1.0 at the last class of positive mass for a few percent of the tokens (26 of 4 000 draws
    of the host form differ from the oracle through it, 25 of them at t = 0) — a summation-order artefact no other
    summation order reproduces.  So a form is held to this: its token is the inverse-CDF draw after cutting NOTHING, or
    after cutting a tail of the descending order that lies wholly within float32 summation error of 1.0 (192 roundings
    of 2^-24, cumulative probabilities in float64).  Returns the (B,S) bool mismatches against the nearest such draw."""
    assert cfg["name"] == "top_p" and cfg["top_p"] == 1.0
    B, C, S = logp.shape
    u = R.token_uniforms(seed, first_layout, B, S, step)[..., 0]
    lg = (logp / cfg.get("temperature", 1.0)).float()
    s_lg, s_idx = torch.sort(lg, descending=True, dim=1, stable=True)
    p64 = torch.softmax(s_lg.double(), dim=1)
    zone = (torch.cumsum(p64, dim=1) > 1.0 - 192 * 2.0 ** -24) & (torch.arange(C).view(1, C, 1) > 0)
    n_pos = (p64 > 1e-20).sum(dim=1, keepdim=True)                      # classes of positive mass lead the order
    rank = s_idx.argsort(dim=1)                                          # class -> position in the descending order
    ok = torch.zeros(B, S, dtype=torch.bool)
    for m in range(4):                                                   # cut the last m classes of positive mass (+ the rest)
        cut_sorted = (torch.arange(C).view(1, C, 1) >= n_pos - m) & zone
        cut = cut_sorted.gather(1, rank)
        ok |= inverse_cdf(lg.masked_fill(cut, -float("inf")), u) == out
    return ~ok


def inverse_cdf(lg, u):
    """The oracle's inverse-CDF rule on already filtered / noised logits (B,C,S) float32."""
    cdf = torch.cumsum(torch.softmax(lg, dim=1).double(), dim=1)
    thr = torch.as_tensor(u, dtype=torch.float64).view(lg.shape[0], 1, -1) * cdf[:, -1:, :]
    return (cdf <= thr).sum(dim=1).clamp(max=lg.shape[1] - 1)


def wrong_gumbel_draw(logp, cfg, step, variant, seed=SEED, first_layout=FIRST_LAYOUT):
    """Deliberately WRONG gumbel draws, each a mistake a kernel could make while support, determinism and
    seed-sensitivity stay intact: the parity tests must tell every one of them from the right draw."""
    B, C, S = logp.shape
    T = cfg.get("temperature", 1.0)
    u4 = R.token_uniforms(seed, first_layout, B, S, step, n=4)
    u = u4[..., 0]
    gu = torch.from_numpy(R.token_gumbel_uniforms(seed, first_layout, B, S, step, C))
    noise = lambda x: -torch.log(-torch.log(x + 1e-30) + 1e-30)
    if variant == "no_noise":
        lg = logp / T
    elif variant == "shared_across_classes":       # one value per token: cancels in the softmax
        lg = logp / T + noise(gu[:, :1, :])
    elif variant == "before_division":             # (l + g) / T instead of l / T + g
        lg = (logp + noise(gu)) / T
    elif variant == "draw_word_reused":            # class c reads component c & 3 of the DRAW's block
        lg = logp / T + noise(torch.from_numpy(u4).permute(0, 2, 1)[:, torch.arange(C) & 3, :])
    elif variant == "step_ignored":                # counter word 1 stuck at 0
        lg = logp / T + noise(torch.from_numpy(R.token_gumbel_uniforms(seed, first_layout, B, S, 0, C)))
    else:
        raise KeyError(variant)
    return inverse_cdf(lg.float(), u)


def chi_square(draws, p, n_class):
    """Pearson statistic of integer draws against probabilities p over the classes with n p >= 5; returns
    (chi2, dof, bound = dof + 6 sqrt(2 dof) + 10, draws that fell on the other classes, number of those classes)."""
    p = np.asarray(p, np.float64)
    cnt = np.bincount(np.asarray(draws).ravel(), minlength=n_class).astype(np.float64)
    n = cnt.sum()
    keep = p * n >= 5
    chi2 = float((((cnt - n * p) ** 2)[keep] / (n * p)[keep]).sum())
    dof = int(keep.sum()) - 1
    return chi2, dof, dof + 6 * math.sqrt(2 * dof) + 10, float(cnt[~keep].sum()), int((~keep).sum())
