"""GPU: vocabularies above 192 classes (64 and 128 bins per coordinate) on the reference-precision engines (exact, split):
denoiser logits, ldm_posterior, ldm_sample_tokens, ldm_sample_step / ldm_sample_loop, the scoring entry points, decode, and
the drop-in classes end to end — each against the oracle restatement (oracle/restatement.py), which is parametric in n_bin.

Vocabularies: tests/_wide_vocab.py VOCABS (195, 283, 519 and 576 classes).  Backbone: d_model 64, 4 heads, d_ff 128, 2 layers,
4 elements (S = 20), T = 10 — the generic tiled kernels; the reference backbone (row-resident LayerNorm + GEMM head with 10
tiles at 283 classes, layout-resident attention) runs once, in a fresh process.

Tolerances are those of tests/test_hip_parity.py: LOGIT_REL_TOL for logits, 2e-4 absolute for the posterior
(test_posterior_vs_reference_golden).  A stochastic draw on identical uniforms may differ from the oracle's only where float32
rounding moves a CDF edge across the uniform: 2 per 2 000 tokens (tests/test_post_token_scalar.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import restatement as R
from oracle import spec as SP
from oracle import synth

import _vb_cases as VC
import _wide_vocab as WV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_REL_TOL = {"exact": 2e-5, "split": 5e-5}   # tests/test_hip_parity.py
POSTERIOR_TOL = 2e-4                             # tests/test_hip_parity.py::test_posterior_vs_reference_golden


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


_ENG = {}


def engine(n_category, n_bin, precision, q_type="constrained", chunk=0):
    from layout_dm_amd.binding import Engine

    key = (n_category, n_bin, precision, q_type, chunk)
    if key not in _ENG:
        spec, sd, _ = WV.tiny_model(n_category, n_bin, q_type)
        e = Engine(n_category=n_category, n_bin=n_bin, max_elem=spec.max_elem, d_model=spec.d_model, n_head=spec.n_head,
                   d_ff=spec.d_ff, n_layer=spec.n_layer, n_step=spec.n_step, precision=precision, max_batch=8, chunk=chunk,
                   q_type=q_type)
        e.load_state_dict(sd)
        _ENG[key] = e
    return _ENG[key]


def _rel(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


# ----------------------------------------------------------------------------- logits
@pytest.mark.parametrize("precision", ["exact", "split"])
@pytest.mark.parametrize("n_category,n_bin", WV.VOCABS, ids=WV.VOCAB_IDS)
def test_logits_vs_restatement(cuda, n_category, n_bin, precision):
    spec, _, W = WV.tiny_model(n_category, n_bin)
    e = engine(n_category, n_bin, precision)
    tokens = WV.states(spec, B=3, seed=1)
    for t in (0, spec.n_step - 1):
        out = e.denoise_logits(tokens.int(), t).cpu()
        assert out.shape == (3, spec.seq_len, spec.n_class)
        rel = _rel(out, R.denoiser_logits(W, spec, tokens, t))
        print(f"[{spec.n_class} classes / {precision} t={t}] logits rel err {rel:.2e}")
        assert rel <= LOGIT_REL_TOL[precision]


def test_logits_on_the_reference_backbone_in_a_fresh_process(golden_dir):
    """464 / 8 / 1856 / 4, 25 elements, 64 bins (283 classes), B = 2: lngemm16x3_k's head at 10 tiles, the head image packer and the
    layout-resident attention; a fresh process, as tests/test_split_shapes_gpu.py::test_short_sequences_in_a_fresh_process.
    States and weights of the reference fixture: the logits are held to the restatement AND to the reference's own."""
    code = f'''
import dataclasses, os, sys
sys.path.insert(0, {ROOT!r})
import numpy as np, torch
from oracle import restatement as R, spec as SP, synth
from layout_dm_amd.binding import Engine
fx = np.load(os.path.join({golden_dir!r}, "wide_vocab", "wide_vocab_rico25_64.npz"))
spec = dataclasses.replace(SP.RICO25, name="rico25_64", n_bin=64)
sd = synth.synth_state_dict(spec, seed=int(fx["weight_seed"]), perturb=True)
W = R.as_torch_weights(sd)
for prec, tol in (("exact", 2e-5), ("split", 5e-5)):
    e = Engine(n_category=spec.n_category, n_bin=spec.n_bin, precision=prec, max_batch=2)
    e.load_state_dict(sd)
    if prec == "split":
        assert "row_resident_ln_gemm" in e.describe()["kernels"] and "attn_out_proj_fused" in e.describe()["kernels"], e.describe()
    for t in (99, 1):
        tokens = torch.from_numpy(fx[f"tokens_{{t}}"].astype(np.int64))
        assert tokens.shape[0] == 2
        out = e.denoise_logits(tokens.int(), t).cpu()
        for what, ref in (("restatement", R.denoiser_logits(W, spec, tokens, t)), ("reference", torch.from_numpy(fx[f"logits_{{t}}"]))):
            err = ((out - ref).abs().max() / ref.abs().max()).item()
            assert err <= tol, (prec, t, what, err)
            print("OK", prec, t, what, err, flush=True)
    e.close()
'''
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.count("OK ") == 8, p.stdout[-3000:]


# ----------------------------------------------------------------------------- posterior
def _check_posterior(out, ref, what):
    d = (out - ref).abs().max().item()
    print(f"[{what}] posterior max abs err {d:.2e}")
    assert d <= POSTERIOR_TOL, what
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * POSTERIOR_TOL     # (each of the two may move by the tolerance)
    assert torch.equal(out.argmax(1)[clear], ref.argmax(1)[clear]), what
    dead = ref == ref.min()
    assert torch.equal(out[dead], ref[dead]), what             # the log(1e-30) fill is exact


@pytest.mark.parametrize("n_category,n_bin", WV.VOCABS, ids=WV.VOCAB_IDS)
def test_posterior_vs_restatement(cuda, n_category, n_bin):
    spec, _, W = WV.tiny_model(n_category, n_bin)
    e = engine(n_category, n_bin, "exact")
    tokens = WV.states(spec, B=3, seed=3)
    assert (tokens == spec.mask_id).any() and (tokens == spec.pad_id).any()
    for t in (0, 1, spec.n_step - 1):
        logits = R.denoiser_logits(W, spec, tokens, t)
        ref = R.q_posterior(W, spec, R.predict_start_from_logits(logits), tokens, t)
        out = e.posterior(logits, tokens.int(), t).cpu()
        _check_posterior(out, ref, f"{spec.n_class} classes t={t}")


def test_vanilla_posterior_and_step_at_283_classes(cuda):
    """q_type = vanilla: every class is live (live set 283 > 192) — the full-vocabulary form on the step path too."""
    spec, _, W = WV.tiny_model(25, 64, "vanilla")
    e = engine(25, 64, "exact", q_type="vanilla")
    tokens = WV.states(spec, B=3, seed=4)
    t = 4
    logits = R.denoiser_logits(W, spec, tokens, t)
    ref = R.q_posterior(W, spec, R.predict_start_from_logits(logits), tokens, t, q_type="vanilla")
    _check_posterior(e.posterior(logits, tokens.int(), t).cpu(), ref, "vanilla 283 classes")
    ref_next, lg, logp = R.single_step(W, spec, tokens, t, {"name": "deterministic"}, return_all=True, q_type="vanilla")
    top2 = logp.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3 * float(lg.abs().max())
    nxt = e.sample_step(tokens.int(), t, {"name": "deterministic"}).cpu().long()
    assert clear.float().mean() > 0.25 and torch.equal(nxt[clear], ref_next[clear])
    cfg = {"name": "random", "temperature": 1.0}
    u = R.token_uniforms(WV.SEED, WV.FIRST_LAYOUT, 3, spec.seq_len, 2)[..., 0]
    ref_draw = R.single_step(W, spec, tokens, t, cfg, uniforms=u, q_type="vanilla")
    got = e.sample_step(tokens.int(), t, cfg, seed=WV.SEED, first_layout=WV.FIRST_LAYOUT, step=2).cpu().long()
    assert int((got != ref_draw).sum()) <= 2 * got.numel() // 2000


# ----------------------------------------------------------------------------- sample_tokens
@pytest.mark.parametrize("n_category,n_bin", WV.VOCABS, ids=WV.VOCAB_IDS)
def test_sample_tokens_vs_restatement_on_identical_uniforms(cuda, n_category, n_bin):
    """All five samplers at their parameter edges (WV.sampler_cfgs) on the oracle's own log-probabilities, 8 layouts:
    160 tokens per setting, 1 600 per vocabulary — one CDF-edge rounding is admitted over all settings together."""
    spec, _, W = WV.tiny_model(n_category, n_bin)
    e = engine(n_category, n_bin, "exact")
    tokens = WV.states(spec, B=8, seed=5)
    _, _, logp = R.single_step(W, spec, tokens, 5, {"name": "deterministic"}, return_all=True)
    top2 = logp.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0
    bad, total = {}, 0
    for step, (name, cfg) in enumerate(WV.sampler_cfgs(spec, logp)):
        out = e.sample_tokens(logp, cfg, seed=WV.SEED, first_layout=WV.FIRST_LAYOUT, step=step).cpu().long()
        ref = WV.oracle_draw(logp, cfg, step)
        if name in ("deterministic", "top_k1", "top_p_below_max"):   # nothing left to draw: the same float32 values, the same argmax
            assert torch.equal(out[clear], logp.argmax(1)[clear]), name
        bad[name] = WV.top_p_one_cut_is_rounding(out, ref, logp, cfg, step) if name == "top_p1.0" else int((out != ref).sum())
        total += out.numel()
    print(f"[{spec.n_class} classes] sample_tokens mismatches over {total} tokens: {bad}")
    assert sum(bad.values()) <= 2 * total // 2000, bad


def test_exact_tie_takes_the_first_maximum_in_class_order(cuda):
    """Two and three equal maxima per token, placed in different lanes and slots of the 9-slot map (classes 70 / 200 / 575 ...)"""
    spec, _, _ = WV.tiny_model(62, 128)
    e = engine(62, 128, "exact")
    C, S = spec.n_class, spec.seq_len
    g = torch.Generator().manual_seed(6)
    logp = (-5.0 - 20.0 * torch.rand(2, C, S, generator=g)).float()
    want = torch.empty(2, S, dtype=torch.long)
    for b in range(2):
        for s in range(S):
            ties = sorted(torch.randperm(C, generator=g)[:2 + (s % 2)].tolist())
            logp[b, ties, s] = -1.25
            want[b, s] = ties[0]
    logp[0, [70, 200, 575], 0] = -1.25
    want[0, 0] = min(70, int(want[0, 0]))
    out = e.sample_tokens(logp, {"name": "deterministic"}).cpu().long()
    assert torch.equal(out, want) and torch.equal(want, logp.argmax(1))


# ----------------------------------------------------------------------------- greedy step
@pytest.mark.parametrize("n_category,n_bin", WV.VOCABS, ids=WV.VOCAB_IDS)
def test_greedy_step_teacher_forced(cuda, n_category, n_bin):
    """The step path (live form, one wavefront per token): exact and split give the oracle's greedy tokens wherever its
    top-two gap exceeds 1e-3 x max |logit| — fifty times the split engine's logits tolerance."""
    spec, _, W = WV.tiny_model(n_category, n_bin)
    tokens = WV.states(spec, B=3, seed=7)
    for t in (spec.n_step - 1, 2):
        ref_next, logits, logp = R.single_step(W, spec, tokens, t, {"name": "deterministic"}, return_all=True)
        top2 = logp.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-3 * float(logits.abs().max())
        assert clear.float().mean() > 0.25       # (the comparison below is not vacuous)
        for precision in ("exact", "split"):
            nxt = engine(n_category, n_bin, precision).sample_step(tokens.int(), t, {"name": "deterministic"}).cpu().long()
            assert torch.equal(nxt[clear], ref_next[clear]), (precision, t)
            for a in range(spec.n_attr):
                assert torch.isin(nxt[:, a::spec.n_attr], torch.as_tensor(spec.full_ids(a))).all()


# ----------------------------------------------------------------------------- loop
def _conds(spec, B):
    g = torch.Generator().manual_seed(8)
    c = synth.synth_cond_c(spec, B, seed=1)
    seq, mask = torch.from_numpy(c["seq"]), torch.from_numpy(c["mask"])
    # partial: some whole elements given (strong mask), the rest [MASK]; no [PAD] disable (helpers/task.py:61-75)
    full = WV.states(spec, B=B, seed=9, p_mask=0.0, p_pad=0.0)
    keep = (torch.rand(B, spec.max_elem, generator=g) < 0.4).repeat_interleave(spec.n_attr, dim=1)
    pseq = torch.where(keep, full, torch.full_like(full, spec.mask_id))
    weak = (-8.0 * torch.rand(B, spec.n_class, spec.seq_len, generator=g)).float()
    return {"c": {"seq": seq, "mask": mask, "type": "c"},
            "partial": {"seq": pseq, "mask": keep, "type": "partial"},
            "refinement": {"seq": seq, "mask": mask, "type": "refinement", "weak_logits": weak,
                           "weak_mask": (~mask)[:, None, :].expand(B, spec.n_class, spec.seq_len)}}


def _replay(W, spec, start, inter, steps, cfg, cond, seed, first):
    """The oracle's step on the ENGINE's own previous state with the kernel's uniforms, step by step: a draw that differs does
    not carry over into the comparison of the steps behind it.  -> (mismatches, tokens compared)"""
    B, S = start.shape
    prev, bad = start.long(), 0
    for i, t in enumerate(steps):
        u = gu = None
        if cfg["name"] != "deterministic":
            u = R.token_uniforms(seed, first, B, S, i)[..., 0]
            if cfg["name"] == "gumbel":
                gu = R.token_gumbel_uniforms(seed, first, B, S, i, spec.n_class)
        ref = R.single_step(W, spec, prev, t, cfg, cond, uniforms=u, gumbel_uniforms=gu)
        bad += int((inter[i].long() != ref).sum())
        prev = inter[i].long()
    return bad, len(steps) * B * S


@pytest.mark.parametrize("precision", ["exact", "split"])
def test_loop_vs_restatement_on_identical_uniforms(cuda, precision):
    """T = 10, B = 5 in chunks of 2 (three passes, the last with one layout), 283 classes: random, top_p and gumbel, unconditional
    and under cond c / partial / refinement (weak_logits (5, 283, 20)); the captured graph gives the bits of the plain launches."""
    spec, _, W = WV.tiny_model(25, 64)
    e = engine(25, 64, precision, chunk=2)
    assert e.chunk == 2
    B, steps = 5, R.timestep_list(spec.n_step, spec.n_step)
    conds = _conds(spec, B)
    runs = [("random", {"name": "random", "temperature": 1.0}, None), ("top_p", {"name": "top_p", "top_p": 0.9, "temperature": 1.0}, None),
            ("gumbel", {"name": "gumbel", "temperature": 0.7}, None),
            ("random/c", {"name": "random", "temperature": 1.0}, "c"), ("top_p/partial", {"name": "top_p", "top_p": 0.9, "temperature": 1.0}, "partial"),
            ("gumbel/refinement", {"name": "gumbel", "temperature": 0.7}, "refinement")]
    bad = total = 0
    for k, (name, cfg, ctype) in enumerate(runs):
        cond = conds[ctype] if ctype else None
        hip_cond = {x: v for x, v in cond.items() if x != "weak_mask"} if cond else None
        start = cond["seq"].int() if cond else torch.full((B, spec.seq_len), spec.mask_id, dtype=torch.int32)
        outs = []
        for use_graph in (False, True):
            tok, inter = e.sample_loop(start.clone().to(cuda), steps, steps, cfg, cond=hip_cond, seed=WV.SEED + k, first_layout=WV.FIRST_LAYOUT,
                                       intermediates=True, use_graph=use_graph)
            outs.append((tok.cpu(), inter.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), name
        final, inter = outs[1]
        assert torch.equal(final, inter[-1]) and (final != spec.mask_id).all(), name
        for a in range(spec.n_attr):
            assert torch.isin(final[:, a::spec.n_attr].long(), torch.as_tensor(spec.full_ids(a))).all(), name
        if cond:
            m = cond["mask"]
            assert torch.equal(final.long()[m], cond["seq"][m]), name
        n, tot = _replay(W, spec, start, inter, steps, cfg, cond, WV.SEED + k, WV.FIRST_LAYOUT)
        print(f"[loop {name} / {precision}] tokens differing from the oracle's step on identical uniforms: {n}/{tot}")
        bad += n
        total += tot
    assert bad <= 2 * total // 2000, (bad, total)


# ----------------------------------------------------------------------------- scoring
def _vb_dist(spec):
    """The recorded float32-vs-float64 distance of a term exists for the fixture's 155- and 135-class models only.  The largest
    one recorded stands in, scaled by the row length: the float32 sums of a token run over C classes instead of 155."""
    fx = VC.fixture()
    d = max(float(v) for k, v in fx.items() if k.endswith(("kl_dist", "nll_dist", "aux_dist")))
    return d * spec.n_class / 155.0


@pytest.mark.parametrize("precision", ["exact", "split"])
@pytest.mark.parametrize("n_category,n_bin", [(25, 64), (62, 128)], ids=["283", "576"])
def test_vb_terms_and_step_vs_float64_restatement(cuda, n_category, n_bin, precision):
    spec, _, W = WV.tiny_model(n_category, n_bin)
    e = engine(n_category, n_bin, precision)
    x0 = WV.states(spec, B=3, seed=10, p_mask=0.0, p_pad=0.2)
    dist = _vb_dist(spec)
    for t in (0, 4, spec.n_step - 1):
        xt = e.q_sample(x0.int(), t, WV.SEED, WV.FIRST_LAYOUT)
        logits = e.denoise_logits(xt, t)
        sums, tok = e.vb_terms(logits, x0.int(), xt, t, per_token=True)
        want, amax = VC.restated_terms(W, spec, "constrained", x0, xt.cpu().long(), t)
        bars = (6.0 * LOGIT_REL_TOL[precision] * amax + 4.0 * dist)[:, None]
        for i, k in enumerate(VC.TERMS):
            d = np.abs(tok[i].double().cpu().numpy() - want[i])
            print(f"[{spec.n_class} classes / {precision} t={t}] {k}: max |ours - restatement| = {d.max():.3e}, bar {float(bars.min()):.3e}")
            assert (d <= bars).all(), (k, t, float(d.max()), float(bars.min()))
        step = e.vb_step(x0.int(), t, xt=xt)
        assert torch.equal(step.view(torch.int64), sums.view(torch.int64))
        drawn = e.vb_step(x0.int(), t, seed=WV.SEED, first_layout=WV.FIRST_LAYOUT)
        assert torch.equal(drawn.view(torch.int64), sums.view(torch.int64))


@pytest.mark.parametrize("n_category,n_bin", [(25, 64), (62, 128)], ids=["283", "576"])
def test_q_sample_vs_float64_restatement_and_error_word(cuda, n_category, n_bin):
    """x_t by the inverse CDF over exp(q_pred) of the position's sub-vocabulary (kept class alpha_bar + beta_bar, every other
    non-MASK class beta_bar, [MASK] gamma_bar; float32 terms as util.py:19-21, sums in float64) on R.token_uniforms."""
    spec, sd, W = WV.tiny_model(n_category, n_bin)
    e = engine(n_category, n_bin, "exact")
    B, S = 8, spec.seq_len
    x0 = WV.states(spec, B=B, seed=11, p_mask=0.0, p_pad=0.2)
    bad = total = 0
    for t in (0, 3, 6, spec.n_step - 1):
        got = e.q_sample(x0.int(), t, WV.SEED, WV.FIRST_LAYOUT).cpu().long()
        u = R.token_uniforms(WV.SEED, WV.FIRST_LAYOUT, B, S, t)[..., 0].astype(np.float64)
        want = torch.empty_like(got)
        for a, key in enumerate(SP.VAR_NAMES):
            ids = torch.as_tensor(spec.full_ids(a))
            LA, LB, LC, L1C = (W[f"{key}_{n}"][t].float() for n in ("log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct", "log_1_min_cumprod_ct"))
            eps = torch.tensor(SP.LOG_EPS, dtype=torch.float32)
            same, other = R.log_add_exp(0.0 + LA, LB).exp(), R.log_add_exp(eps + LA, LB).exp()
            mask = R.log_add_exp(eps + L1C, LC).exp()
            xa = x0[:, a::spec.n_attr]
            p = other.double().expand(B, xa.shape[1], len(ids)).clone()
            p[..., -1] = mask.double()
            k0 = (xa.unsqueeze(-1) == ids.view(1, 1, -1)).long().argmax(-1)
            p.scatter_(2, k0.unsqueeze(-1), same.double().expand(B, xa.shape[1], 1))
            cdf = p.cumsum(-1)
            n = (cdf <= torch.from_numpy(u[:, a::spec.n_attr]).unsqueeze(-1) * cdf[..., -1:]).sum(-1).clamp(max=len(ids) - 1)
            want[:, a::spec.n_attr] = ids[n]
        bad += int((got != want).sum())
        total += got.numel()
        ones = torch.cat([e.q_sample(x0[i:i + 1].int(), t, WV.SEED, WV.FIRST_LAYOUT + i) for i in range(B)]).cpu().long()
        assert torch.equal(ones, got)
    print(f"[{spec.n_class} classes] q_sample tokens differing from the float64 restatement: {bad}/{total}")
    assert bad <= 2 * total // 2000
    # the error word: an x-position holding a token of the y sub-vocabulary; a token outside [0, C); [MASK] in x_0
    wrong = x0.clone()
    wrong[1, 1] = spec.n_category + spec.n_bin + 3
    with pytest.raises(ValueError, match="sub-vocabulary"):
        e.q_sample(wrong.int(), 3)
    logits = e.denoise_logits(x0.int(), 3)
    with pytest.raises(ValueError, match="sub-vocabulary"):
        e.vb_terms(logits, wrong.int(), x0.int(), 3)
    with pytest.raises(ValueError, match="sub-vocabulary"):
        e.vb_step(x0.int(), 3, xt=wrong.int())
    wrong = x0.clone()
    wrong[0, 0] = spec.n_class
    with pytest.raises(ValueError, match="outside"):
        e.q_sample(wrong.int(), 3)
    wrong[0, 0] = spec.mask_id
    with pytest.raises(ValueError, match=r"\[MASK\]"):
        e.vb_step(wrong.int(), 3)
    assert torch.equal(e.q_sample(x0.int(), 3, WV.SEED, WV.FIRST_LAYOUT).cpu(), e.q_sample(x0.int(), 3, WV.SEED, WV.FIRST_LAYOUT).cpu())


# ----------------------------------------------------------------------------- decode
@pytest.mark.parametrize("n_category,n_bin", [(25, 64), (5, 128)], ids=["64_bins", "128_bins"])
def test_decode_bit_for_bit(cuda, n_category, n_bin):
    spec, _, _ = WV.tiny_model(n_category, n_bin)
    e = engine(n_category, n_bin, "exact")
    tokens = WV.states(spec, B=8, seed=12, p_mask=0.0, p_pad=0.0)
    tokens[2, 2 * spec.n_attr:] = spec.pad_id
    tokens[5] = spec.pad_id
    rng = np.random.default_rng(3)
    centres = np.sort(rng.random((4, n_bin)), axis=1)
    for cen in (None, centres):
        got = e.decode(tokens.int(), None if cen is None else torch.from_numpy(cen))
        want = R.decode_layouts(spec, tokens, cen)
        for k in ("bbox", "label", "mask"):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k].cpu(), want[k]), (k, cen is None)


# ----------------------------------------------------------------------------- the drop-in classes
BACKBONE_CFG = {"_target_": "trainer.models.transformer_utils.TransformerEncoder",
                "encoder_layer": {"_target_": "trainer.models.transformer_utils.Block", "d_model": 64, "nhead": 4,
                                  "dim_feedforward": 128, "dropout": 0.0, "batch_first": True, "norm_first": True,
                                  "timestep_type": "adalayernorm", "diffusion_step": 10},
                "num_layers": 2}


def test_end_to_end_fit_bins_auto_engine_sample_decode(cuda, caplog):
    """boxes -> fit_coordinate_bins at 64 clusters -> LayoutDM(precision="auto") on a stub tokenizer with those centres ->
    sample_from_layouts(cond c) -> decode: auto IS the split engine (no fp16 engine exists), says why, and every token lies in
    its position's sub-vocabulary."""
    import logging

    from _stub_tokenizer import StubTokenizer
    from layout_dm_amd import clustering as cl
    from layout_dm_amd.layoutdm import LayoutDM

    rng = np.random.default_rng(0)
    boxes = np.clip(rng.random((4000, 4)).astype(np.float32), 0.01, 1.0)
    models = cl.fit_coordinate_bins(boxes, "kmeans", n_clusters_list=(64,))
    # (LayoutDM shrinks the configured backbone by 29/32: 71 -> 64, 142 -> 128)
    cfg = {**BACKBONE_CFG, "encoder_layer": {**BACKBONE_CFG["encoder_layer"], "d_model": 71, "dim_feedforward": 142}}
    assert int(29 / 32 * 71) == 64 and int(29 / 32 * 142) == 128
    spec = SP.ModelSpec("e2e_64", n_category=25, n_bin=64, max_elem=4, d_model=64, n_head=4, d_ff=128, n_layer=2, n_step=10)
    tok = StubTokenizer(spec)
    tok.bbox_tokenizer.bbox_quantization = "kmeans"
    tok.bbox_tokenizer.clustering_models = {k: cl.ClusterModel("kmeans", np.sort(m.cluster_centers_, axis=0)) for k, m in models.items()}
    with caplog.at_level(logging.INFO, logger="layout_dm_amd"):
        m = LayoutDM(backbone_cfg=cfg, tokenizer=tok, q_type="constrained", num_timesteps=10, precision="auto", max_batch=8)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, seed=1, perturb=True).items()})
    inner = m.model.module
    assert inner.selected_precision == "split" and inner.verified is None and inner._v_fast is None and not inner._v_rung
    assert inner.engine.describe()["precision"] == "split_f16"
    rec = [r.getMessage() for r in caplog.records if "precision='auto'" in r.getMessage()]
    assert rec and "283 classes" in rec[-1] and "192" in rec[-1], rec
    assert inner.selection_report["n_class"] == 283 and "192" in inner.selection_report["reason"]
    B, E = 6, spec.max_elem
    layouts = {"bbox": torch.from_numpy(boxes[:B * E]).view(B, E, 4), "label": torch.from_numpy(rng.integers(0, 25, (B, E))),
               "mask": torch.arange(E).view(1, E) < torch.tensor([4, 3, 1, 4, 2, 4]).view(B, 1)}
    scfg = {"name": "random", "temperature": 1.0, "num_timesteps": 10}
    ids = m.sample_from_layouts(layouts, "c", scfg, seed=5, cond_seed=1)
    assert set(ids) == {"bbox", "label", "mask"} and ids["bbox"].shape == (B, E, 4) and ids["bbox"].dtype == torch.float64
    assert torch.equal(ids["mask"], layouts["mask"]) and torch.equal(ids["label"][layouts["mask"]], layouts["label"][layouts["mask"]])
    from layout_dm_amd import task

    cond = task.get_cond({k: v.to(cuda) for k, v in layouts.items()}, tok, "c", seed=1)
    seq = inner.sample(batch_size=B, cond=cond, sampling_cfg=scfg, seed=5).cpu()
    for a in range(spec.n_attr):
        assert torch.isin(seq[:, a::spec.n_attr], torch.as_tensor(spec.full_ids(a)[:-1])).all()      # body or [PAD], never [MASK]
    centres = np.stack([tok.bbox_tokenizer.clustering_models[f"{k}-64"].cluster_centers_.reshape(-1) for k in "xywh"]).astype(np.float64)
    want = R.decode_layouts(spec, seq, centres)
    assert torch.equal(want["bbox"], ids["bbox"]) and torch.equal(want["mask"], ids["mask"])
    inner.close()


def test_fp16_names_raise_not_implemented_with_the_librarys_message(cuda):
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    for precision in ("fast", "fast_verified", "mixed", "hybrid_verified"):
        with pytest.raises(NotImplementedError, match="192 classes"):
            HipMaskAndReplaceDiffusion(n_category=25, n_bin=64, precision=precision, max_batch=4)


def test_relation_stays_at_32_bins(cuda):
    """cond=relation above 32 bins: NotImplementedError from Python, rc -4 from ldm_relation_update (the relation kernel's rows
    and lane map are 32 wide: DESIGN section 7)."""
    from _stub_tokenizer import StubTokenizer
    from layout_dm_amd.relation import relation_geometry

    spec, _, _ = WV.tiny_model(25, 64)
    with pytest.raises(NotImplementedError, match="32 bins"):
        relation_geometry(StubTokenizer(spec))
    e = engine(25, 64, "exact")
    B = 2
    graph = {"y": torch.zeros(2 * B, dtype=torch.long), "edge_index": torch.tensor([[0, 2], [1, 3]]), "edge_attr": torch.tensor([17, 17]),
             "batch": torch.tensor([0, 0, 1, 1])}
    rel = e.make_relation(graph, np.tile(np.linspace(0, 1, 64), (4, 1)), [31, 31, 63, 63], 3e6, 3, B)
    logp = torch.zeros(B, spec.n_class, spec.seq_len, device=cuda)
    with pytest.raises(RuntimeError, match=r"\(-4\).*<= 32"):
        e.relation_update(logp, torch.full((B, spec.seq_len), spec.pad_id), rel, 50)


# ----------------------------------------------------------------------------- the reference fixture on the reference backbone
REF_SPEC = SP.ModelSpec("rico25_64", n_category=25, n_bin=64)
_REF = {}


@pytest.fixture(scope="module")
def fx(golden_dir):
    with np.load(os.path.join(golden_dir, "wide_vocab", "wide_vocab_rico25_64.npz")) as z:
        return {k: z[k] for k in z.files}


def ref_engine(fx, precision):
    from layout_dm_amd.binding import Engine

    if precision not in _REF:
        e = Engine(n_category=25, n_bin=64, precision=precision, max_batch=2)
        e.load_state_dict(synth.synth_state_dict(REF_SPEC, seed=int(fx["weight_seed"]), perturb=True))
        _REF[precision] = e
    return _REF[precision]


def test_greedy_step_teacher_forced_on_the_fixture_trajectory(cuda, fx):
    """Every chosen state of the reference's greedy trajectory (num_timesteps = 10 of T = 100: skip_step = 9): first, on the CPU,
    the oracle's top-two gap exceeds 1e-3 x max |logit| at every token of these states; then exact and split give the reference's
    tokens exactly."""
    from layout_dm_amd.diffusion import timestep_schedule

    W = R.as_torch_weights(synth.synth_state_dict(REF_SPEC, seed=int(fx["weight_seed"]), perturb=True))
    after = torch.from_numpy(fx["traj_states_after"].astype(np.int64))
    before = torch.cat([torch.full_like(after[:1], REF_SPEC.mask_id), after[:-1]])
    t_model, t_post = timestep_schedule(100, 10)
    assert t_model == fx["traj_steps"].tolist()
    chosen = fx["traj_chosen"].tolist()
    assert len(chosen) >= 5 and any(((before[i] == REF_SPEC.mask_id) & (after[i] != REF_SPEC.mask_id)).any() for i in chosen)
    for i in chosen:
        nxt, logits, logp = R.single_step(W, REF_SPEC, before[i], t_model[i], {"name": "deterministic"},
                                          skip_step=t_model[i] - t_post[i], return_all=True)
        top2 = logp.topk(2, dim=1).values
        assert bool(((top2[:, 0] - top2[:, 1]) > 1e-3 * float(logits.abs().max())).all()), i
        assert torch.equal(nxt, after[i])
    for precision in ("exact", "split"):
        e = ref_engine(fx, precision)
        for i in chosen:
            got = e.sample_step(before[i].int(), t_model[i], {"name": "deterministic"}, t_post=t_post[i]).cpu().long()
            assert torch.equal(got, after[i]), (precision, i, int((got != after[i]).sum()))


@pytest.mark.parametrize("precision", ["exact", "split"])
def test_greedy_loop_reproduces_the_fixture(cuda, fx, precision):
    from layout_dm_amd.diffusion import timestep_schedule

    e = ref_engine(fx, precision)
    after = torch.from_numpy(fx["traj_states_after"].astype(np.int32))
    t_model, t_post = timestep_schedule(100, 10)
    for use_graph in (False, True):
        tok = torch.full((2, REF_SPEC.seq_len), REF_SPEC.mask_id, dtype=torch.int32, device=cuda)
        out, inter = e.sample_loop(tok, t_model, t_post, {"name": "deterministic"}, intermediates=True, use_graph=use_graph)
        assert torch.equal(inter.cpu(), after) and torch.equal(out.cpu(), after[-1]), (precision, use_graph)
    dec = e.decode(out)
    assert dec["bbox"].dtype == torch.float32 and np.array_equal(dec["bbox"].cpu().numpy(), fx["decode_bbox"])
    assert np.array_equal(dec["label"].cpu().numpy(), fx["decode_label"]) and np.array_equal(dec["mask"].cpu().numpy(), fx["decode_mask"])
