"""Writes tests/golden/vb/reference.npz: what the reference's own forward() (ConstrainedMaskAndReplaceDiffusion.forward,
constrained.py:232-333; VanillaMaskAndReplaceDiffusion.forward, vanilla.py:160-240) draws and computes on given layouts, for
tests/test_vb_core.py and tests/test_vb_gpu.py.  Data only; the weights are not stored (oracle/synth.py rebuilds them).

    python tools/make_vb_golden.py            # needs the reference tree (oracle.ref_harness)
    LDM_VB_GOLDEN_OUT=/tmp/again.npz python tools/make_vb_golden.py     # elsewhere: a regeneration equals the committed file array for array

Models: rico25 and publaynet (constrained), rico25 (vanilla), synthetic weights (seed WEIGHT_SEED, perturb=True).
forward() is driven through instance-level patches, the reference itself is not edited: `sample_time` is replaced to force one
t for the batch, t in {0, 1, T // 3, T - 1} (0: the decoder branch and the u = T wrap of constrained.py:114; 1: reads index 0),
plus one batch with per-layout t and importance weights pt (the loss scalars); `q_sample` / `predict_start` / `q_posterior`
are wrapped to record what forward drew and produced, and `q_sample` also forces two states: layout 4 all [MASK], layout 5
x_t == x_0.

x_0 (B = 6): all [PAD]; 1 element; 25 elements; 7 elements; 12 elements (forced all [MASK]); 3 elements (forced x_t == x_0).

Per (model, t): x_t, the per-token kl / decoder_nll / kl_aux (float32: the reference's own functions on the recorded tensors,
i.e. what forward() reduces), the same formulas evaluated in float64 from the same float32 inputs (the reference's
q_posterior on a float64 copy of the module) and their distance to the float32 values (the reference's own rounding noise:
the tests' bars are multiples of it), log_x0_recon of layout RECON_LAYOUT, exp(q_pred) of every position (the draw test).

chi2_*: the draw test's one (attribute, class, t) and its bins.  The reference's schedule leaves the beta-bar classes
1 - alpha_bar_t - gamma_bar_t = 1e-6 of the mass TOGETHER (base.py:44-47: att + ctt = 0.999999 at every t), an expected
count of 0.02 in 20 000 draws: merged into one bin they still miss the chi-square precondition (every expected count >= 5),
so that bin is merged once more, into the kept class's; two bins (not [MASK] / [MASK]) remain, both checked here.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh  # noqa: E402
from oracle import spec as SP  # noqa: E402
from oracle import synth  # noqa: E402

OUT = os.environ.get("LDM_VB_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden", "vb", "reference.npz")
WEIGHT_SEED = 1
MODELS = (("rico25", "constrained"), ("publaynet", "constrained"), ("rico25", "vanilla"))
N_ELEM = (0, 1, 25, 7, 12, 3)
ALL_MASK, KEEP_X0, RECON_LAYOUT = 4, 5, 3
T_MIXED = (0, 1, 33, 99, 7, 60)
CHI2_DRAWS = 20000


def layouts(spec, seed):
    """(6, S) int64 valid sequences, [PAD] until max (layout_tokenizer.py:222-253)."""
    rng = np.random.default_rng(seed)
    x = np.full((len(N_ELEM), spec.seq_len), spec.pad_id, np.int64)
    for b, n in enumerate(N_ELEM):
        for e in range(n):
            x[b, e * 5] = rng.integers(spec.n_category)
            for a in range(1, 5):
                x[b, e * 5 + a] = spec.n_category + (a - 1) * spec.n_bin + rng.integers(spec.n_bin)
    return torch.from_numpy(x)


def time_weights(m, T):
    """pt_all of sample_time("importance") (base.py:179-198) as the reference itself reports it: the pt it returns next to
    every drawn t, collected until each timestep has been seen (torch's generator is left as it was found)."""
    state = torch.get_rng_state()
    pt_all = torch.full((T,), float("nan"))
    for _ in range(64):
        t, pt = m.sample_time(65536, torch.device("cpu"), "importance")
        pt_all[t] = pt
        if not bool(pt_all.isnan().any()):
            break
    torch.set_rng_state(state)
    assert not bool(pt_all.isnan().any())
    return pt_all


def drive(m, m64, spec, q_type, x0, t_vec, pt_vec):
    """One forward() with t, pt forced -> everything recorded."""
    from trainer.models.categorical_diffusion.util import index_to_log_onehot, log_categorical

    rec = {"q_pred": [], "post": []}
    orig = {k: getattr(m, k) for k in ("sample_time", "q_sample", "predict_start", "q_posterior")}
    m.sample_time = lambda b, device, method="uniform": (t_vec.clone(), pt_vec.clone())

    def q_sample(log_x_start, t, key=None):
        args = (log_x_start, t) if key is None else (log_x_start, t, key)
        rec["q_pred"].append(m.q_pred(*args).exp())
        out = orig["q_sample"](**({"log_x_start": log_x_start, "t": t} if key is None else {"log_x_start": log_x_start, "t": t, "key": key}))
        K = out.shape[1]
        shape = out.shape[2:]
        out[ALL_MASK] = index_to_log_onehot(torch.full((1, *shape), K - 1, dtype=torch.long), K)[0]
        out[KEEP_X0] = log_x_start[KEEP_X0]
        return out

    def predict_start(log_x_t, t):
        rec["xt"] = log_x_t.argmax(1)
        rec["recon"] = orig["predict_start"](log_x_t, t)
        return rec["recon"]

    def q_posterior(log_x_start, log_x_t, t):
        rec["log_x_t"] = log_x_t
        rec["post"].append(orig["q_posterior"](log_x_start=log_x_start, log_x_t=log_x_t, t=t))
        return rec["post"][-1]

    m.q_sample, m.predict_start, m.q_posterior = q_sample, predict_start, q_posterior
    hist, count = m.Lt_history.clone(), m.Lt_count.clone()
    try:
        with torch.no_grad():
            _, losses = m.forward(x0, is_train=True)
    finally:
        for k in orig:
            delattr(m, k)      # the instance attributes: the class's methods are back
        m.Lt_history.copy_(hist)
        m.Lt_count.copy_(count)
    model, true = rec["post"]
    lx0 = index_to_log_onehot(x0, spec.n_class)
    recon = rec["recon"]
    out = {"xt": rec["xt"], "recon": recon, "q_pred": rec["q_pred"],
           "kl": m.multinomial_kl(true, model), "nll": -log_categorical(lx0, model),
           "aux": m.multinomial_kl(lx0[:, :-1], recon[:, :-1]),
           "kl_loss": losses["kl_loss"], "aux_loss": losses["aux_loss"]}
    # the same formulas in float64 from the same float32 inputs
    with torch.no_grad():
        r64, lxt64, lx064 = recon.double(), rec["log_x_t"].double(), lx0.double()
        model64 = m64.q_posterior(log_x_start=r64, log_x_t=lxt64, t=t_vec)
        true64 = m64.q_posterior(log_x_start=lx064, log_x_t=lxt64, t=t_vec)
        assert model64.dtype == torch.float64 and true64.dtype == torch.float64
        out["kl64"] = m64.multinomial_kl(true64, model64)
        out["nll64"] = -log_categorical(lx064, model64)
        out["aux64"] = m64.multinomial_kl(lx064[:, :-1], r64[:, :-1])
    return out


def main():
    fx = {"n_elem": np.array(N_ELEM, np.int32), "all_mask": np.int32(ALL_MASK), "keep_x0": np.int32(KEEP_X0),
          "recon_layout": np.int32(RECON_LAYOUT), "weight_seed": np.int32(WEIGHT_SEED), "t_mixed": np.array(T_MIXED, np.int32)}
    for ds, q_type in MODELS:
        spec = SP.SPECS[ds]
        T = spec.n_step
        name = f"{ds}_{q_type}"
        m, _ = rh.build_reference_model(ds, seed=0, perturb=True, q_type=q_type)
        sd = synth.synth_state_dict(spec, seed=WEIGHT_SEED, perturb=True, prefix="", q_type=q_type)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
        m64 = copy.deepcopy(m).double()
        if hasattr(m64, "converter"):
            m64.converter.to(torch.device("cpu"))
        x0 = layouts(spec, seed=20261019 + len(name))
        fx[f"{name}/x0"] = x0.numpy().astype(np.int16)
        ts = (0, 1, T // 3, T - 1)
        fx[f"{name}/ts"] = np.array(ts, np.int32)
        B = x0.shape[0]
        for t in ts:
            r = drive(m, m64, spec, q_type, x0, torch.full((B,), t, dtype=torch.long), torch.full((B,), 1.0 / T))
            assert (r["xt"][ALL_MASK] == spec.mask_id).all() and (r["xt"][KEEP_X0] == x0[KEEP_X0]).all()
            p = f"{name}/t{t}/"
            fx[p + "xt"] = r["xt"].numpy().astype(np.int16)
            fx[p + "recon"] = r["recon"][RECON_LAYOUT].numpy()
            for k in ("kl", "nll", "aux"):
                fx[p + k] = r[k].numpy()
                assert r[k].dtype == torch.float32
                fx[p + k + "_dist"] = np.float64((r[k].double() - r[k + "64"]).abs().max().item())
            fx[p + "kl_loss"], fx[p + "aux_loss"] = np.float32(r["kl_loss"].item()), np.float32(r["aux_loss"].item())
            # exp(q_pred): constrained, one (B, K, E) block per attribute; vanilla (B, C, S)
            for i, q in enumerate(r["q_pred"]):
                fx[p + f"q_pred{i}"] = q.numpy()
        # the loss scalars at per-layout t with importance weights (base.py:179-192)
        g = torch.Generator().manual_seed(7)
        m.Lt_history.copy_(torch.rand(T, generator=g) * 4.0 + 0.01)
        m.Lt_count.fill_(11.0)
        torch.manual_seed(3)
        t_ref, pt_ref = m.sample_time(4096, torch.device("cpu"), "importance")
        pt_all = time_weights(m, T)
        assert torch.equal(pt_ref, pt_all[t_ref]) and abs(float(pt_all.sum()) - 1.0) < 1e-5 and pt_all[0] == pt_all[1]
        t_vec = torch.tensor(T_MIXED, dtype=torch.long)
        r = drive(m, m64, spec, q_type, x0, t_vec, pt_all[t_vec])
        p = f"{name}/mixed/"
        fx[p + "Lt_history"], fx[p + "Lt_count"] = m.Lt_history.numpy().copy(), m.Lt_count.numpy().copy()
        fx[p + "pt_all"], fx[p + "pt"] = pt_all.numpy(), pt_all[t_vec].numpy()
        fx[p + "xt"] = r["xt"].numpy().astype(np.int16)
        fx[p + "kl_loss"], fx[p + "aux_loss"] = np.float32(r["kl_loss"].item()), np.float32(r["aux_loss"].item())
        for k in ("kl", "nll", "aux"):
            fx[p + k] = r[k].numpy()
            fx[p + k + "_dist"] = np.float64((r[k].double() - r[k + "64"]).abs().max().item())
        m.Lt_history.zero_(), m.Lt_count.zero_()
        # uniform fallback of sample_time (base.py:181-182): pt = 1 / T
        _, pt_u = m.sample_time(4, torch.device("cpu"), "importance")
        assert torch.equal(pt_u, torch.full((4,), 1.0 / T))

    # the chi-square case: rico25 constrained, attribute x (1), class = bin 5, t = T // 3
    spec, T = SP.RICO25, SP.RICO25.n_step
    t, attr, cls = T // 3, 1, spec.n_category + 5
    row = fx[f"rico25_constrained/t{t}/q_pred{attr}"]
    x0 = fx["rico25_constrained/x0"].astype(np.int64)
    b = 2                                                    # the 25-element layout
    e = int(np.argmax(x0[b, attr::5] >= 0))
    k0 = int(x0[b, attr + 5 * e] - spec.n_category)          # live index of that position's x_0
    probs = row[b, :, e].astype(np.float64)                  # body, [PAD], [MASK]
    chi_row = np.full_like(probs, probs[(k0 + 1) % 32])
    chi_row[k0], chi_row[-1] = probs[k0], probs[-1]
    assert np.array_equal(chi_row, probs)                    # three kinds of class, as exp(q_pred) has them
    others = np.delete(probs[:-1], k0).sum()
    assert others * CHI2_DRAWS < 5                           # the beta-bar bin alone misses the precondition ...
    bins = np.array([probs[:-1].sum(), probs[-1]]) / probs.sum()
    assert (bins * CHI2_DRAWS >= 5).all()                    # ... merged with the kept class it holds
    # (the row depends on the live index of x_0 only through where the kept class sits)
    fx["chi2/t"], fx["chi2/attr"], fx["chi2/live_index"] = np.int32(t), np.int32(attr), np.int32(5)
    same, other, mask = probs[k0], probs[(k0 + 1) % 32], probs[-1]
    fx["chi2/probs"] = np.array([same, other, mask], np.float32)
    fx["chi2/bins"] = bins
    fx["chi2/draws"] = np.int32(CHI2_DRAWS)
    assert cls < spec.n_class

    floor = min(float(v[v > 0].min()) for k, v in fx.items() if k.rsplit("/", 1)[-1] in ("kl", "nll", "aux") and (v > 0).any())
    fx["zero_floor"] = np.float32(floor)                     # the smallest positive float32 term: the bar where the distance is 0
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **fx)
    print(OUT, os.path.getsize(OUT), "bytes; zero floor", floor)
    for k in sorted(fx):
        if k.endswith("_dist") or k.endswith("_loss"):
            print(f"  {k} = {float(fx[k]):.4g}")


if __name__ == "__main__":
    main()
