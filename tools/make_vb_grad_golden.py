"""Writes tests/golden/vb_grad/: the gradient of the reference's own training loss with respect to the denoiser's logits, as its
autograd computes it (ConstrainedMaskAndReplaceDiffusion.forward, constrained.py:232-333; VanillaMaskAndReplaceDiffusion.forward,
vanilla.py:160-240), for tests/test_vb_grad_core.py, tests/test_training_host.py and tests/test_vb_grad_gpu.py.  Data only; the
weights are not stored (oracle/synth.py rebuilds them).

    python tools/make_vb_grad_golden.py            # needs the reference tree (oracle.ref_harness)
    LDM_VB_GRAD_GOLDEN_OUT=/tmp/again python tools/make_vb_grad_golden.py   # elsewhere: a regeneration equals the committed files array for array

forward() is driven through instance-level patches like tools/make_vb_golden.py, the reference itself is not edited: `sample_time`
forces t and pt, `q_sample` forces layout 4 all [MASK] and layout 5 x_t == x_0, and a forward hook on `m.transformer` hands
predict_start the transformer's logits as a LEAF with retain_grad(); forward(x0, is_train=True) runs with grad and
(kl_loss + aux_loss).backward() leaves d loss / d logits on the leaf.  The same once more on a float64 copy of the module, fed the
same float32 logits and the same x_t: its gradient is the reference the tests hold every element to, and the per-token-row distance
max_c |g32 - g64| of the two is the reference's own rounding noise, the unit of the tests' bars.

Models (max_seq_length = 4: S = 20; synthetic weights, seed WEIGHT_SEED, perturb=True):
    rico25_constrained      C = 155, live sets 27 and 34           publaynet_constrained   C = 135, live set 7 (and 34)
    rico25_vanilla          the full-vocabulary form               rico25b64_constrained   64 bins: C = 283, live 66 (the wavefront forms)
x_0 (B = 6): all [PAD]; 1; 4; 2 elements; 3 elements (forced all [MASK]); 2 elements (forced x_t == x_0).
Cases per model: t in {0, 1, T // 3, T - 1} with pt = 1 / T; `mixed`: per-layout t with importance weights pt; `sharp`: mixed's
t and pt on the transformer's logits times 8 with one live class of every row pushed 90 below the row maximum, so that both clamps
(log_x0_recon and the posterior at -70) are active somewhere — asserted here.

Files: reference.npz holds everything small (x_0, x_t, t, pt, the loss scalars, the per-layout token sums the scalars were reduced
from, the row distances, `zero_floor`: the smallest positive row distance of all cases); <model>.<case>.npz holds that case's
logits (float32) and the float64 gradient — one file each, so that no committed file passes 1 MiB.
"""
from __future__ import annotations

import copy
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh  # noqa: E402
from oracle import spec as SP  # noqa: E402
from oracle import synth  # noqa: E402

OUT = os.environ.get("LDM_VB_GRAD_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden", "vb_grad")
WEIGHT_SEED = 1
MAX_ELEM = 4
# name -> (dataset, q_type, bins per coordinate)
MODELS = {"rico25_constrained": ("rico25", "constrained", 32), "publaynet_constrained": ("publaynet", "constrained", 32),
          "rico25_vanilla": ("rico25", "vanilla", 32), "rico25b64_constrained": ("rico25", "constrained", 64)}
N_ELEM = (0, 1, 4, 2, 3, 2)
ALL_MASK, KEEP_X0 = 4, 5
T_MIXED = (0, 1, 33, 99, 7, 60)
SHARP_SCALE, SHARP_DROP = 8.0, 90.0


def model_spec(name):
    ds, _, n_bin = MODELS[name]
    return dataclasses.replace(SP.SPECS[ds], max_elem=MAX_ELEM, n_bin=n_bin)


def build_model(name):
    """oracle.ref_harness.build_reference_model at max_seq_length = MAX_ELEM and the model's bins, synthetic weights loaded"""
    ds, q_type, n_bin = MODELS[name]
    spec = model_spec(name)
    rh.install_stubs()
    from trainer.helpers.layout_tokenizer import LayoutSequenceTokenizer
    from trainer.models.categorical_diffusion.constrained import ConstrainedMaskAndReplaceDiffusion as cls
    from trainer.models.common.util import shrink

    if q_type == "vanilla":
        from trainer.models.categorical_diffusion.vanilla import VanillaMaskAndReplaceDiffusion as cls
    data_cfg, dataset_cfg, backbone_cfg = rh.make_cfgs(ds, spec.n_step)
    data_cfg.num_bin_bboxes = n_bin
    dataset_cfg.max_seq_length = MAX_ELEM
    torch.manual_seed(0)
    tok = LayoutSequenceTokenizer(data_cfg, dataset_cfg)
    assert tok.N_total == spec.n_class and tok.max_token_length == spec.seq_len
    m = cls(backbone_cfg=shrink(backbone_cfg, 29 / 32), num_classes=tok.N_total, max_token_length=tok.max_token_length,
            num_timesteps=spec.n_step, pos_emb="elem_attr", transformer_type="flattened", auxiliary_loss_weight=0.1, tokenizer=tok)
    sd = synth.synth_state_dict(spec, seed=WEIGHT_SEED, perturb=True, prefix="", q_type=q_type)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval()
    m64 = copy.deepcopy(m).double()
    if hasattr(m64, "converter"):
        m64.converter.to(torch.device("cpu"))
    return m, m64, spec, q_type


def layouts(spec, seed):
    """(6, S) int64 valid sequences, [PAD] until max (layout_tokenizer.py:222-253)"""
    rng = np.random.default_rng(seed)
    x = np.full((len(N_ELEM), spec.seq_len), spec.pad_id, np.int64)
    for b, n in enumerate(N_ELEM):
        for e in range(n):
            x[b, e * 5] = rng.integers(spec.n_category)
            for a in range(1, 5):
                x[b, e * 5 + a] = spec.n_category + (a - 1) * spec.n_bin + rng.integers(spec.n_bin)
    return torch.from_numpy(x)


def sub_vocab(spec, q_type, attr):
    if q_type == "vanilla":
        return 0, spec.n_class - 2
    return (0, spec.n_category) if attr == 0 else (spec.n_category + (attr - 1) * spec.n_bin, spec.n_bin)


def sharpen(logits, spec, q_type):
    """logits x 8, one live class of every row 90 below the row's maximum"""
    out = logits * SHARP_SCALE
    B, S, _ = out.shape
    for b in range(B):
        for s in range(S):
            start, count = sub_vocab(spec, q_type, s % spec.n_attr)
            c = start + (7 * s + 3 * b) % count
            row = out[b, s, :-1]
            out[b, s, c] = torch.cat([row[:c], row[c + 1:]]).max() - SHARP_DROP
    return out


def drive(m, spec, q_type, x0, t_vec, pt_vec, logits_in=None, xt_in=None, sharp=False):
    """One forward() + backward() with t, pt forced.  logits_in / xt_in None: the module's own transformer and draw (with the two
    forced states), recorded; given (the float64 copy): those float32 logits and those states."""
    from trainer.models.categorical_diffusion.util import index_to_log_onehot

    dtype = next(m.transformer.parameters()).dtype
    rec = {"x_t": [], "post": []}
    orig = {k: getattr(m, k) for k in ("sample_time", "q_sample", "predict_start", "q_posterior")}
    m.sample_time = lambda b, device, method="uniform": (t_vec.clone(), pt_vec.clone().to(dtype))

    def q_sample(log_x_start, t, key=None):
        kw = {"log_x_start": log_x_start, "t": t} if key is None else {"log_x_start": log_x_start, "t": t, "key": key}
        if xt_in is not None:
            return xt_in[len(rec["x_t"])].to(dtype)
        out = orig["q_sample"](**kw)
        K = out.shape[1]
        out[ALL_MASK] = index_to_log_onehot(torch.full((1, *out.shape[2:]), K - 1, dtype=torch.long), K)[0]
        out[KEEP_X0] = log_x_start[KEEP_X0]
        return out

    def q_sample_rec(log_x_start, t, key=None):
        out = q_sample(log_x_start, t, key)
        rec["x_t"].append(out.detach().clone())
        return out

    def predict_start(log_x_t, t):
        rec["xt"] = log_x_t.argmax(1)
        rec["recon"] = orig["predict_start"](log_x_t, t)
        return rec["recon"]

    def q_posterior(log_x_start, log_x_t, t):
        rec["post"].append(orig["q_posterior"](log_x_start=log_x_start, log_x_t=log_x_t, t=t))
        return rec["post"][-1]

    def hook(_mod, _args, out):
        if logits_in is None:
            lg = out["logits"].detach()
            lg = sharpen(lg, spec, q_type) if sharp else lg
        else:
            lg = logits_in.to(dtype)
        rec["logits"] = lg.clone().requires_grad_(True)
        rec["logits"].retain_grad()
        return {"logits": rec["logits"]}

    m.q_sample, m.predict_start, m.q_posterior = q_sample_rec, predict_start, q_posterior
    handle = m.transformer.register_forward_hook(hook)
    hist, count = m.Lt_history.clone(), m.Lt_count.clone()
    try:
        _, losses = m.forward(x0, is_train=True)
        (losses["kl_loss"] + losses["aux_loss"]).backward()
    finally:
        handle.remove()
        for k in orig:
            delattr(m, k)      # the instance attributes: the class's methods are back
        m.Lt_history.copy_(hist)
        m.Lt_count.copy_(count)
        m.zero_grad()
    model = rec["post"][0].detach()
    lx0 = index_to_log_onehot(x0, spec.n_class).to(dtype)
    recon = rec["recon"].detach()
    # the per-layout token SUMS the two scalars were reduced from (float64 additions of the module's own per-token terms)
    true = rec["post"][1].detach()
    kl = (true.exp() * (true - model)).sum(1).double().sum(1)
    nll = -(lx0.exp() * model).sum(1).double().sum(1)
    aux = (lx0[:, :-1].exp() * (lx0[:, :-1] - recon[:, :-1])).sum(1).double().sum(1)
    return {"xt": rec["xt"], "x_t": rec["x_t"], "logits": rec["logits"].detach(), "grad": rec["logits"].grad.detach(),
            "recon": recon, "model": model, "sums": torch.stack([kl, nll, aux], 1),
            "kl_loss": losses["kl_loss"].detach(), "aux_loss": losses["aux_loss"].detach()}


def main():
    os.makedirs(OUT, exist_ok=True)
    fx = {"n_elem": np.array(N_ELEM, np.int32), "all_mask": np.int32(ALL_MASK), "keep_x0": np.int32(KEEP_X0),
          "weight_seed": np.int32(WEIGHT_SEED), "t_mixed": np.array(T_MIXED, np.int32), "max_elem": np.int32(MAX_ELEM),
          "aux_weight": np.float64(0.1)}
    sizes = {}
    for name in MODELS:
        m, m64, spec, q_type = build_model(name)
        T = spec.n_step
        x0 = layouts(spec, seed=20261020 + len(name))
        B = x0.shape[0]
        fx[f"{name}/x0"] = x0.numpy().astype(np.int16)
        fx[f"{name}/n_bin"] = np.int32(spec.n_bin)
        # importance weights (base.py:179-192) for the per-layout batch
        g = torch.Generator().manual_seed(7)
        hist = torch.rand(T, generator=g) * 4.0 + 0.01
        Lt_sqrt = torch.sqrt(hist + 1e-10) + 0.0001
        Lt_sqrt[0] = Lt_sqrt[1]
        pt_all = Lt_sqrt / Lt_sqrt.sum()
        t_mixed = torch.tensor(T_MIXED, dtype=torch.long)
        cases = [(f"t{t}", torch.full((B,), t, dtype=torch.long), torch.full((B,), 1.0 / T), False) for t in (0, 1, T // 3, T - 1)]
        cases += [("mixed", t_mixed, pt_all[t_mixed], False), ("sharp", t_mixed, pt_all[t_mixed], True)]
        fx[f"{name}/cases"] = np.array([c[0] for c in cases])
        for case, t_vec, pt_vec, sharp in cases:
            r = drive(m, spec, q_type, x0, t_vec, pt_vec, sharp=sharp)
            r64 = drive(m64, spec, q_type, x0, t_vec, pt_vec, logits_in=r["logits"], xt_in=r["x_t"])
            assert r["grad"].dtype == torch.float32 and r64["grad"].dtype == torch.float64 and torch.equal(r["xt"], r64["xt"])
            assert (r["xt"][ALL_MASK] == spec.mask_id).all() and (r["xt"][KEEP_X0] == x0[KEEP_X0]).all()
            assert bool((r["grad"][..., -1] == 0).all())
            if sharp:   # both clamps are active somewhere
                assert bool((r["recon"][:, :-1] == -70).any()) and bool((r["model"] == -70).any()), name
            p = f"{name}/{case}/"
            fx[p + "xt"] = r["xt"].numpy().astype(np.int16)
            fx[p + "t"], fx[p + "pt"] = t_vec.numpy().astype(np.int32), pt_vec.numpy()
            fx[p + "kl_loss"], fx[p + "aux_loss"] = np.float32(r["kl_loss"].item()), np.float32(r["aux_loss"].item())
            fx[p + "kl_loss64"], fx[p + "aux_loss64"] = np.float64(r64["kl_loss"].item()), np.float64(r64["aux_loss"].item())
            fx[p + "sums64"] = r64["sums"].numpy()
            fx[p + "row_dist"] = (r["grad"].double() - r64["grad"]).abs().amax(-1).numpy()
            path = os.path.join(OUT, f"{name}.{case}.npz")
            np.savez_compressed(path, logits=r["logits"].numpy(), grad64=r64["grad"].numpy())
            sizes[path] = os.path.getsize(path)
            d = fx[p + "row_dist"]
            print(f"  {name}/{case}: max |grad| {float(r64['grad'].abs().max()):.3g}, row distance max {d.max():.3g}, rows at 0: {(d == 0).sum()}")
    floor = min(float(v[v > 0].min()) for k, v in fx.items() if k.endswith("/row_dist") and (v > 0).any())
    fx["zero_floor"] = np.float64(floor)       # the bar's unit where a row's distance is exactly 0
    path = os.path.join(OUT, "reference.npz")
    np.savez_compressed(path, **fx)
    sizes[path] = os.path.getsize(path)
    assert max(sizes.values()) < (1 << 20)
    print(f"{len(sizes)} files, {sum(sizes.values())} bytes, largest {max(sizes.values())}; zero floor {floor:.3g}")


if __name__ == "__main__":
    main()
