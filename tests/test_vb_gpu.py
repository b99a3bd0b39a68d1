"""GPU: scoring given layouts (ldm_q_sample / ldm_vb_terms / ldm_vb_step, kernels_vb.hip) and what is built on them
(HipMaskAndReplaceDiffusion.vb_terms / elbo / loss / time_weights, LayoutDM.score / evaluate_loss, score_entry).

Expected values: the float64 restatement (_vb_cases.restated_terms: R.denoiser_logits in float64 -> R.predict_start_from_logits
-> R.q_posterior -> the three sums), which tests/test_vb_core.py pins to the reference's recorded terms on the CPU.
Bar per token: 6 x eps_abs + 4 x the recorded float32-vs-float64 distance of the term, eps_abs = LOGIT_REL_TOL[mode] x
max |logit| of the layout — the tolerance tests/test_hip_parity.py holds that mode's logits to, through the 6 of DESIGN
section 3.5 (log-softmax <= 2 eps, the normalised q <= 2 x that, its lse <= 1 x that; log-add-exp and the clamp 1-Lipschitz).
The per-layout sums, the repeat and the alone-vs-in-a-batch checks are bit for bit."""
import dataclasses
import functools
import json
import pickle

import numpy as np
import pytest
import torch

import _hostbuild as HB
import _vb_cases as VC
from _stub_tokenizer import StubTokenizer
from oracle import restatement as R
from oracle import spec as SP
from oracle import synth
from test_hip_parity import BACKBONE_CFG, LOGIT_REL_TOL, WEIGHT_SEED
from test_hip_parity import engine as parity_engine

pytestmark = pytest.mark.gpu

SEED, FIRST = 20261019, 3


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def state_dict(ds, q_type):
    return synth.synth_state_dict(SP.SPECS[ds], seed=WEIGHT_SEED, perturb=True, q_type=q_type)


@functools.lru_cache(maxsize=None)
def diffusion(ds, q_type):
    """the exact-mode HipMaskAndReplaceDiffusion of a fixture model"""
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    d = HipMaskAndReplaceDiffusion(n_category=SP.SPECS[ds].n_category, precision="exact", max_batch=8, q_type=q_type)
    d.load_state_dict(state_dict(ds, q_type))
    return d


def engine_of(ds, q_type, precision):
    if precision == "exact":
        return diffusion(ds, q_type).engine
    assert q_type == "constrained"
    return parity_engine(ds, precision)


def bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def sequential_sums(tok):
    """(3,B,S) float32 -> (B,3) float64: positions left to right, the kernel's documented order"""
    tok = tok.double().cpu().numpy()
    out = np.zeros((tok.shape[1], 3))
    for s in range(tok.shape[2]):
        out += tok[:, :, s].T
    return out


# ----------------------------------------------------------------------------- q_sample
@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_q_sample_equals_the_host_build(cuda, tmp_path, ds, q_type):
    fx, spec = VC.fixture(), SP.SPECS[ds]
    e = engine_of(ds, q_type, "exact")
    exe = HB.host_program("cpu_vb_check")
    x0 = fx[f"{VC.name(ds, q_type)}/x0"][:5].astype(np.int32)
    x0_d = torch.from_numpy(x0).to(cuda)
    for t in fx[f"{VC.name(ds, q_type)}/ts"]:
        t = int(t)
        rc, raw = HB.run_host_io(exe, tmp_path, VC.payload(ds, q_type, t, x0, seed=SEED, first_layout=FIRST), "draw")
        assert rc == 0
        _, host = VC.parse_draw(raw, 5, spec.seq_len)
        got = e.q_sample(x0_d, t, SEED, FIRST)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), host), t
        # the batch cut as 2 + 3 and as 1 x 5, first_layout set
        cut = torch.cat([e.q_sample(x0_d[:2], t, SEED, FIRST), e.q_sample(x0_d[2:], t, SEED, FIRST + 2)])
        ones = torch.cat([e.q_sample(x0_d[i:i + 1], t, SEED, FIRST + i) for i in range(5)])
        assert torch.equal(cut, got) and torch.equal(ones, got)
    t = spec.n_step // 3          # (at t = T - 1 nearly every draw is [MASK] whatever the key)
    assert not torch.equal(e.q_sample(x0_d, t, SEED + 1, FIRST), e.q_sample(x0_d, t, SEED, FIRST))


# ----------------------------------------------------------------------------- vb_terms
CASES = [(ds, "constrained", p) for ds in ("rico25", "publaynet") for p in ("exact", "split", "fast")] + [("rico25", "vanilla", "exact")]


@pytest.mark.parametrize("ds,q_type,precision", CASES)
def test_vb_terms_on_the_fixture(cuda, ds, q_type, precision):
    fx, spec = VC.fixture(), SP.SPECS[ds]
    e = engine_of(ds, q_type, precision)
    x0 = torch.from_numpy(fx[f"{VC.name(ds, q_type)}/x0"].astype(np.int32)).to(cuda)
    for t in fx[f"{VC.name(ds, q_type)}/ts"]:
        t = int(t)
        p = f"{VC.name(ds, q_type)}/t{t}/"
        xt = torch.from_numpy(fx[p + "xt"].astype(np.int32)).to(cuda)
        logits = e.denoise_logits(xt, t)
        sums, tok = e.vb_terms(logits, x0, xt, t, per_token=True)
        want, amax, ref_logits = VC.restated_fixture(ds, q_type, t)     # computed once, shared by the numerics modes
        for i, k in enumerate(VC.TERMS):
            bars = VC.restated_bars(fx, p + k, amax, LOGIT_REL_TOL[precision])
            d = np.abs(tok[i].double().cpu().numpy() - want[i])
            print(f"[{ds}/{q_type}/{precision} t={t}] {k}: max |ours - restatement| = {d.max():.3e}, worst share of its bar {float((d / bars).max()):.3f}")
            assert (d <= bars).all(), (k, t, float(d.max()), float(bars.min()))
        # the sums: the dumped per-token float32 values added in float64, positions left to right — bit for bit
        assert np.array_equal(sums[:, :3].cpu().numpy().view(np.int64), sequential_sums(tok).view(np.int64))
        hits = sums[:, 3].cpu().numpy()
        assert np.array_equal(hits, np.round(hits)) and (hits >= 0).all() and (hits <= spec.seq_len).all()
        if precision == "exact":   # the argmax can differ from the float64 restatement's only where two classes tie within the logits error
            recon = R.predict_start_from_logits(ref_logits)
            assert np.abs(hits - (recon.argmax(1) == x0.cpu().long()).sum(1).numpy()).max() <= 1
        # two runs give the same bits; layout 3 alone gives the bits it has inside the batch of 6; so does ldm_vb_step
        again, tok2 = e.vb_terms(logits, x0, xt, t, per_token=True)
        assert torch.equal(bits(again), bits(sums)) and torch.equal(bits(tok2), bits(tok))
        alone = e.vb_terms(e.denoise_logits(xt[3:4], t), x0[3:4], xt[3:4], t)
        assert torch.equal(bits(alone[0]), bits(sums[3]))
        assert torch.equal(bits(e.vb_step(x0, t, xt=xt)), bits(sums))


# ----------------------------------------------------------------------------- elbo
def test_elbo_on_the_small_backbone(cuda):
    """2 layers, n_step = 20 (small_backbone of tests/test_hip_parity.py), B = 4, precision exact."""
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    fx = VC.fixture()
    spec = dataclasses.replace(SP.RICO25, name="small", d_model=256, n_head=4, d_ff=1024, n_layer=2, n_step=20)
    sd = synth.synth_state_dict(spec, seed=WEIGHT_SEED, perturb=True)
    W = R.as_torch_weights(sd)
    d = HipMaskAndReplaceDiffusion(n_category=spec.n_category, d_model=spec.d_model, n_head=spec.n_head, d_ff=spec.d_ff,
                                   n_layer=spec.n_layer, num_timesteps=spec.n_step, precision="exact", max_batch=8)
    d.load_state_dict(sd)
    x0 = torch.from_numpy(fx["rico25_constrained/x0"][:4].astype(np.int64))
    got = d.elbo(x0, seed=11, first_layout=2)
    assert got.shape == (4,) and got.dtype == torch.float64 and got.is_cuda
    total = None
    for t in range(spec.n_step):
        terms = d.vb_terms(x0, t, seed=11, first_layout=2)
        term = terms["decoder_nll"] if t == 0 else terms["kl"]
        total = term if total is None else total + term
    assert torch.equal(bits(got), bits(total))
    assert torch.equal(bits(d.elbo(x0, seed=11, first_layout=2)), bits(got)) and not torch.equal(d.elbo(x0, seed=12, first_layout=2), got)
    # the restatement on the same drawn x_t.  The recorded float32-vs-float64 distance exists for the fixture's models only:
    # the largest one of this vocabulary's kl / nll stands in (the same formulas on the same sub-vocabularies)
    dist = max(float(v) for k, v in fx.items() if k.startswith("rico25_constrained/") and k.endswith(("kl_dist", "nll_dist")))
    want, bar = np.zeros(4), np.zeros(4)
    for t in range(spec.n_step):
        xt = d.q_sample(x0, t, 11, 2).cpu().long()
        terms, amax = VC.restated_terms(W, spec, "constrained", x0, xt, t)
        want += terms[1 if t == 0 else 0].mean(1)
        bar += 6.0 * LOGIT_REL_TOL["exact"] * amax + 4.0 * dist
    diff = np.abs(got.cpu().numpy() - want)
    print(f"elbo {got.cpu().numpy()}, max |ours - restatement| = {diff.max():.3e}, summed bar {bar.min():.3e}")
    assert (diff <= bar).all() and (got > 0).all()
    d.close()


# ----------------------------------------------------------------------------- loss, time_weights, evaluate_loss
@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_loss_reproduces_the_references_scalars(cuda, ds, q_type):
    fx, spec = VC.fixture(), SP.SPECS[ds]
    p = f"{VC.name(ds, q_type)}/mixed/"
    d = diffusion(ds, q_type)
    T, S = spec.n_step, spec.seq_len
    x0 = torch.from_numpy(fx[f"{VC.name(ds, q_type)}/x0"].astype(np.int64))
    xt = torch.from_numpy(fx[p + "xt"].astype(np.int64))
    t, pt = torch.from_numpy(fx["t_mixed"].astype(np.int64)), torch.from_numpy(fx[p + "pt"])
    got = d.loss(x0, t=t, pt=pt, x_t=xt)
    assert set(got) == {"kl_loss", "aux_loss"}
    # bars: per layout the token mean of the per-token bar, through the same 1 / pt, weights and batch mean
    amax = np.array([float(d.engine.denoise_logits(xt[b:b + 1].int(), int(t[b])).abs().max()) for b in range(len(t))])
    eps = 6.0 * LOGIT_REL_TOL["exact"] * amax
    tn, ptn = t.numpy(), pt.double().numpy()
    bar_kl = np.where(tn == 0, eps + 4 * float(fx[p + "nll_dist"]), eps + 4 * float(fx[p + "kl_dist"]))
    bar_aux = np.where(tn == 0, eps + 4 * float(fx[p + "nll_dist"]), eps + 4 * float(fx[p + "aux_dist"]))
    w = ((1 - tn / T) + 1.0) * 0.1
    for k, bar in (("kl_loss", (bar_kl / ptn).mean()), ("aux_loss", (w * bar_aux / ptn).mean())):
        ref = float(fx[p + k])
        bar += 4 * np.finfo(np.float32).eps * abs(ref)        # the reference's scalar is a float32 mean of float32 quotients
        print(f"[{ds}/{q_type}] {k}: ours {float(got[k]):.6f}, reference {ref:.6f}, bar {bar:.3e}")
        assert abs(float(got[k]) - ref) <= bar
    # given t, pt comes from the checkpoint's history: the fixture's pt_all
    sd = dict(state_dict(ds, q_type))
    sd["model.module.Lt_history"], sd["model.module.Lt_count"] = fx[p + "Lt_history"], fx[p + "Lt_count"]
    d.load_state_dict(sd)
    try:
        assert np.allclose(d.time_weights().numpy(), fx[p + "pt_all"], rtol=1e-6, atol=0)
        again = d.loss(x0, t=t, x_t=xt)
        assert all(abs(float(again[k]) - float(got[k])) <= 1e-6 * abs(float(got[k])) for k in got)
        torch.manual_seed(1)
        ts, pts = d.sample_time(64)
        assert torch.equal(pts, d.time_weights()[ts]) and len(set(ts.tolist())) > 10
    finally:
        d.load_state_dict(state_dict(ds, q_type))
    assert torch.equal(d.time_weights(), torch.ones(T) / T)   # the uniform fallback of base.py:181-182 (Lt_count all 0)
    # drawn x_t: a layout's draw depends on (seed, its global index, its t) alone
    a = d.loss(x0, t=t, pt=pt, seed=5, first_layout=10)
    parts = [d.loss(x0[i:i + 1], t=t[i:i + 1], pt=pt[i:i + 1], seed=5, first_layout=10 + i) for i in range(len(t))]
    for k in a:
        assert abs(float(a[k]) - float(np.mean([float(q[k]) for q in parts]))) <= 1e-12 * abs(float(a[k]))


@functools.lru_cache(maxsize=None)
def layoutdm_model():
    from layout_dm_amd.layoutdm import LayoutDM

    m = LayoutDM(backbone_cfg=BACKBONE_CFG, tokenizer=StubTokenizer(SP.RICO25), q_type="constrained", precision="exact", max_batch=8)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict("rico25", "constrained").items()})
    return m


def test_evaluate_loss_is_the_mean_of_the_batches_losses(cuda):
    m = layoutdm_model()
    x0 = torch.from_numpy(VC.fixture()["rico25_constrained/x0"].astype(np.int64))
    torch.manual_seed(9)
    got = m.evaluate_loss(x0, batch_size=3, seed=5)
    torch.manual_seed(9)
    inner = m.model.module
    want = [sum(float(v) for v in inner.loss(x0[off:off + 3], seed=5, first_layout=off).values()) for off in (0, 3)]
    assert got == (want[0] + want[1]) / 2 and np.isfinite(got) and got > 0
    with pytest.raises(NotImplementedError):
        m.train()
    with pytest.raises(NotImplementedError):
        m.forward({"seq": x0})


def test_layoutdm_score_on_sampled_layouts(cuda):
    m = layoutdm_model()
    layouts = m.sample(batch_size=4, cond=None, sampling_cfg={"name": "random", "temperature": 1.0, "num_timesteps": 10}, seed=3)
    assert set(layouts) == {"bbox", "label", "mask"}
    # an untrained model leaves [PAD] elements between real ones: the entry points keep the valid elements of a layout
    # (test.py:42-49) and that is what a result pickle holds; the reference's encode asserts the prefix form too
    from layout_dm_amd import task
    from layout_dm_amd.test_entry import _filter_invalid

    layouts = task.layouts_from_list(_filter_invalid(layouts), SP.RICO25.max_elem)
    s = m.score(layouts, seed=1)
    assert s.shape == (4,) and s.dtype == torch.float64 and bool(torch.isfinite(s).all()) and bool((s > 0).all())
    seq = m.encode(layouts)["seq"]
    assert torch.equal(bits(m.score(seq, seed=1)), bits(s)) and torch.equal(bits(m.score({"seq": seq}, seed=1)), bits(s))
    with pytest.raises(NotImplementedError):
        m.train()


# ----------------------------------------------------------------------------- refusals
def test_refusals(cuda):
    fx, spec = VC.fixture(), SP.RICO25
    e = engine_of("rico25", "constrained", "exact")
    x0 = torch.from_numpy(fx["rico25_constrained/x0"][:3].astype(np.int32)).to(cuda)
    xt = torch.from_numpy(fx["rico25_constrained/t33/xt"][:3].astype(np.int32)).to(cuda)
    logits = e.denoise_logits(xt, 33)
    good = e.vb_step(x0, 33, xt=xt)
    for t in (spec.n_step, -1):
        for call in (lambda: e.q_sample(x0, t), lambda: e.vb_terms(logits, x0, xt, t), lambda: e.vb_step(x0, t, xt=xt)):
            with pytest.raises(RuntimeError, match="out of range"):
                call()
    for bad, what in ((spec.mask_id, r"\[MASK\]"), (spec.n_class, "outside"), (-1, "outside")):
        x = x0.clone()
        x[2, 7] = bad
        for call in (lambda: e.q_sample(x, 33), lambda: e.vb_terms(logits, x, xt, 33), lambda: e.vb_step(x, 33), lambda: e.vb_step(x, 33, xt=xt)):
            with pytest.raises(ValueError, match=what):
                call()
    z = xt.clone()
    z[1, 0] = spec.n_class + 5     # a given x_t outside the vocabulary never reaches the denoiser's embedding
    with pytest.raises(ValueError, match="outside"):
        e.vb_step(x0, 33, xt=z)
    assert torch.equal(bits(e.vb_step(x0, 33, xt=xt)), bits(good))    # and the next call is clean


# ----------------------------------------------------------------------------- the entry point
def test_score_entry_end_to_end(cuda, tmp_path, capsys):
    import yaml

    from layout_dm_amd import score_entry as SE
    from layout_dm_amd import synthetic as SY
    from test_cond_entry import _layouts
    from test_entry_point import TRAIN_CFG

    job = tmp_path / "job"
    job.mkdir()
    (job / "config.yaml").write_text(yaml.safe_dump(TRAIN_CFG))
    torch.save({k: torch.from_numpy(v) for k, v in SY.synth_state_dict(SY.RICO25, seed=1, perturb=True).items()}, job / "best_model.pt")
    lay = tmp_path / "lay.pkl"
    pickle.dump({"results": _layouts(6)}, open(lay, "wb"))
    args = [f"job_dir={job}", f"layouts={lay}", "seed=4", f"out={tmp_path / 'score.json'}", "batch_size=4", "precision=exact", "max_batch_size=8"]
    out = SE.main(args)
    data = json.load(open(tmp_path / "score.json"))
    assert data == json.loads(json.dumps(out)) and data["n_layouts"] == 6 and len(data["checkpoints"]) == 1
    rec = data["checkpoints"][0]
    assert f"test_loss: {rec['test_loss']}" in capsys.readouterr().out
    assert len(rec["elbo"]) == 6 and all(np.isfinite(v) and v > 0 for v in rec["elbo"]) and rec["test_loss"] > 0
    assert SE.main(args)["checkpoints"][0] == rec               # reproducible under the seed
    # check_checkpoint layouts=...: the selection record carries the same held-out loss (seed 0, the reference's batch of 64)
    from layout_dm_amd import check_checkpoint as CC

    rep = CC.check(str(job), max_batch=8, precision="exact", layouts=str(lay))[0]
    base = SE.main([f"job_dir={job}", f"layouts={lay}", f"out={tmp_path / 's0.json'}", "precision=exact", "max_batch_size=8", "elbo=false"])
    assert rep["test_loss"] == base["checkpoints"][0]["test_loss"] and rep["test_loss_layouts"] == 6 and rep["checkpoint"].endswith("best_model.pt")
