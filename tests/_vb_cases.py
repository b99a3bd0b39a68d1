"""Shared by tests/test_vb_core.py and tests/test_vb_gpu.py: the fixture of tools/make_vb_golden.py (what the reference's
forward() drew and computed), the host check program's case files, and the numpy restatement of the forward noising draw."""
import functools
import os

import numpy as np
import torch

from oracle import restatement as R
from oracle import spec as SP
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = (("rico25", "constrained"), ("publaynet", "constrained"), ("rico25", "vanilla"))
TERMS = ("kl", "nll", "aux")


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "vb", "reference.npz")) as z:
        return {k: z[k] for k in z.files}


def name(ds, q_type):
    return f"{ds}_{q_type}"


def sub_vocab(spec, q_type, attr):
    """(start, count) of the attribute's body, as ldm_create lays the vocabulary out"""
    if q_type == "vanilla":
        return 0, spec.n_class - 2
    return (0, spec.n_category) if attr == 0 else (spec.n_category + (attr - 1) * spec.n_bin, spec.n_bin)


def live_ids(spec, q_type, attr):
    start, count = sub_vocab(spec, q_type, attr)
    return np.concatenate([np.arange(start, start + count), [spec.pad_id, spec.mask_id]])


@functools.lru_cache(maxsize=None)
def schedule_table(ds, q_type):
    """float32 [8][n_attr][T + 1]: the device table's layout (ldm_kernels.h ScheduleRow)"""
    spec = SP.SPECS[ds]
    buf = SP.schedule_buffers(spec, q_type)
    out = np.zeros((8, spec.n_attr, spec.n_step + 1), np.float32)   # (the one-step buffers have T entries, the cumulative ones T + 1)
    for r, n in enumerate(SP.SCHEDULE_NAMES):
        for a, key in enumerate(SP.VAR_NAMES):
            v = buf[n if q_type == "vanilla" else f"{key}_{n}"]
            out[r, a, :len(v)] = v
    return out


def payload(ds, q_type, t, x0, xt=None, rows=None, lse=1, seed=0, first_layout=0, sched=None):
    spec = SP.SPECS[ds]
    x0 = np.ascontiguousarray(x0, np.int32)
    B, S = x0.shape
    sv = [sub_vocab(spec, q_type, a) for a in range(spec.n_attr)]
    hdr = [spec.n_class, spec.n_attr, spec.pad_id, spec.mask_id, spec.n_step, t, B, S, lse]
    hdr += [s for s, _ in sv] + [0] * (8 - len(sv)) + [c for _, c in sv] + [0] * (8 - len(sv))
    raw = np.array(hdr, np.int32).tobytes() + np.array([seed, first_layout], np.uint64).tobytes()
    raw += np.ascontiguousarray(schedule_table(ds, q_type) if sched is None else sched, np.float32).tobytes() + x0.tobytes()
    if xt is not None:
        raw += np.ascontiguousarray(xt, np.int32).tobytes() + np.ascontiguousarray(rows, np.float32).tobytes()
    return raw


def parse_terms(raw, B, S):
    """-> (error word, (4,B,S) float32 kl / nll / aux / hit, (B,4) float64 sums)"""
    raw = np.frombuffer(raw, np.uint8)
    n = 4 * B * S * 4
    return int(raw[:4].view(np.int32)[0]), raw[4:4 + n].view(np.float32).reshape(4, B, S), raw[4 + n:].view(np.float64).reshape(B, 4)


def parse_draw(raw, B, S):
    raw = np.frombuffer(raw, np.uint8)
    return int(raw[:4].view(np.int32)[0]), raw[4:].view(np.int32).reshape(B, S)


def q_pred_row(fx, ds, q_type, t, b, s):
    """exp(q_pred) of position s of layout b as the reference computed it, over the position's sub-vocabulary in class order"""
    spec = SP.SPECS[ds]
    p = f"{name(ds, q_type)}/t{t}/"
    if q_type == "vanilla":
        return fx[p + "q_pred0"][b, :, s]
    return fx[p + f"q_pred{s % spec.n_attr}"][b, :, s // spec.n_attr]


def draw_restatement(fx, ds, q_type, t, x0, seed, first_layout):
    """x_t by the inverse CDF over the REFERENCE's exp(q_pred) rows on R.token_uniforms uniforms (counter: position, t, layout;
    key: seed): cumulative sums in float64, in class order, compared against u * total."""
    spec = SP.SPECS[ds]
    B, S = x0.shape
    u = R.token_uniforms(seed, first_layout, B, S, t)[..., 0].astype(np.float64)
    out = np.empty((B, S), np.int32)
    for b in range(B):
        for s in range(S):
            cdf = np.cumsum(q_pred_row(fx, ds, q_type, t, b, s).astype(np.float64))
            n = int((cdf <= u[b, s] * cdf[-1]).sum())
            out[b, s] = live_ids(spec, q_type, s % spec.n_attr)[min(n, len(cdf) - 1)]
    return out


def bar(fx, key):
    """4 x the reference's own float32-vs-float64 distance of that term (the convention of test_lngemm_reference.py: our float32
    evaluation makes the same kind and number of roundings); where that distance is exactly 0, the smallest positive float32
    term of the fixture."""
    d = float(fx[key + "_dist"])
    return 4.0 * d if d > 0 else float(fx["zero_floor"])


def restated_terms(W, spec, q_type, x0, xt, t, logits=None):
    """-> ((3,B,S) float64 kl / nll / aux, (B,) max |logit| per layout); logits: R.denoiser_logits in float64 if at hand"""
    if logits is None:
        logits = R.denoiser_logits(W, spec, xt, t, dtype=torch.float64)
    recon = R.predict_start_from_logits(logits)
    model = R.q_posterior(W, spec, recon, xt, t, q_type=q_type).double()
    lx0 = R.index_to_log_onehot(x0, spec.n_class)
    true = R.q_posterior(W, spec, lx0, xt, t, q_type=q_type).double()
    lx0, recon = lx0.double(), recon.double()
    kl = (true.exp() * (true - model)).sum(1)
    nll = -(lx0.exp() * model).sum(1)
    aux = (lx0[:, :-1].exp() * (lx0[:, :-1] - recon[:, :-1])).sum(1)
    return torch.stack([kl, nll, aux]).numpy(), logits.abs().amax((1, 2)).numpy()


def restated_bars(fx, key, amax, rel_tol):
    """(B,1): 6 x eps_abs + 4 x the recorded distance, eps_abs = rel_tol x max |logit| of the layout (the
    log-softmax moves by <= 2 eps, the normalised q by <= 2 x that, its lse by <= 1 x that; log-add-exp and the clamp are
    1-Lipschitz)."""
    return (6.0 * rel_tol * amax + 4.0 * float(fx[key + "_dist"]))[:, None]


@functools.lru_cache(maxsize=None)
def restated_fixture(ds, q_type, t):
    """The float64 restatement on the fixture's (x_0, x_t) of one (model, t), computed once per session:
    ((3,B,S) terms, (B,) max |logit|, (B,S,C) float64 logits)."""
    fx, spec = fixture(), SP.SPECS[ds]
    W = R.as_torch_weights(synth.synth_state_dict(spec, seed=int(fx["weight_seed"]), perturb=True, q_type=q_type))
    x0 = torch.from_numpy(fx[f"{name(ds, q_type)}/x0"].astype(np.int64))
    xt = torch.from_numpy(fx[f"{name(ds, q_type)}/t{t}/xt"].astype(np.int64))
    logits = R.denoiser_logits(W, spec, xt, t, dtype=torch.float64)
    want, amax = restated_terms(W, spec, q_type, x0, xt, t, logits)
    return want, amax, logits
