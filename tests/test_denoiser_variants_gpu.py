"""GPU: the denoiser variants of the reference's LayoutDM class beyond its default, through the C-ABI, against the real reference's
fixtures tests/golden/variants/*.npz (tools/make_denoiser_variant_golden.py; CPU half: tests/test_denoiser_variants.py).

  * logits per variant and numerics mode within the bound the default variant's golden test holds that mode to
    (tests/test_hip_parity.py LOGIT_REL_TOL): all five modes for the variants that only change load-time tables (pos_emb=default
    under q_type=vanilla, adalayernorm_abs, timestep_type None), exact and split for the two adainnorm kinds, whose error is held
    to 2 x the same mode's measured error on the default variant's golden at the same weight seed (the statistics run over 125
    samples instead of 464); the *_abs variants against the reference's logits with the restated sinusoid patched in;
  * posterior log-probabilities in the exact mode, teacher-forced greedy steps on the marked states in exact and split;
  * the reference's shipped preset experiment/vqdiffusion.yaml (q_type vanilla, pos_emb default) free through LayoutDM.sample on auto;
  * the instance-norm kernel alone (kernels_norm.hip in_rows) through ldm_denoise_logits on a one-layer model against a float64
    NumPy restatement, at the smallest shapes where it can still go wrong."""
import math
import os

import numpy as np
import pytest
import torch

from _stub_tokenizer import StubTokenizer
from layout_dm_amd import synthetic
from test_denoiser_variants import TOOL, fixture

pytestmark = pytest.mark.gpu

LOGIT_REL_TOL = {"exact": 2e-5, "split": 5e-5, "fast": 1e-3, "mixed": 1e-3, "hybrid": 1e-3}   # tests/test_hip_parity.py, per mode
TABLE_ONLY = ("vanilla_default", "abs", "none")
INSTANCE = ("adainnorm", "adainnorm_abs")
SPEC = TOOL.SPEC


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


_ENG = {}


def engine(name, precision):
    from layout_dm_amd.binding import Engine

    if (name, precision) not in _ENG:
        v = TOOL.VARIANTS[name] if name != "default" else TOOL.Variant("default")
        e = Engine(n_category=SPEC.n_category, n_bin=SPEC.n_bin, max_elem=SPEC.max_elem, d_model=SPEC.d_model, n_head=SPEC.n_head,
                   d_ff=SPEC.d_ff, n_layer=SPEC.n_layer, n_step=SPEC.n_step, precision=precision, max_batch=2, q_type=v.q_type,
                   timestep_type=v.timestep_type)
        e.load_state_dict(TOOL.state_dict(v, seed=1))
        _ENG[(name, precision)] = e
    return _ENG[(name, precision)]


def _rel(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


def logits_error(golden_dir, name, precision):
    """max over t in {99, 1, 0} of max |logits - reference| / max |reference| (the *_abs variants: the patched-table logits)"""
    fx = fixture(golden_dir, name)
    key = "logits_patched_" if TOOL.VARIANTS[name].is_abs else "logits_"
    e = engine(name, precision)
    worst = 0.0
    for t in (99, 1, 0):
        out = e.denoise_logits(torch.from_numpy(fx[f"tokens_{t}"].astype(np.int32)), t).cpu()
        worst = max(worst, _rel(out, torch.from_numpy(fx[key + str(t)])))
    return worst


# ----------------------------------------------------------------------------- against the reference's fixtures
@pytest.mark.parametrize("precision", ["exact", "split", "mixed", "hybrid", "fast"])
@pytest.mark.parametrize("name", TABLE_ONLY)
def test_logits_of_the_table_only_variants_in_every_mode(cuda, golden_dir, name, precision):
    worst = logits_error(golden_dir, name, precision)
    d = engine(name, precision).describe()
    print(f"[{name}/{precision}] max rel logits error vs reference: {worst:.3e}; {d.get('kernels')}")
    assert worst <= LOGIT_REL_TOL[precision]
    # the variant is named, and only what is not the default
    v = TOOL.VARIANTS[name]
    assert d.get("pos_emb") == ("default" if v.pos_emb == "default" else None)
    assert d.get("timestep_emb") == ("abs" if v.is_abs else "none" if v.timestep_type is None else None)
    assert "norm1" not in d


@pytest.mark.parametrize("precision", ["exact", "split"])
@pytest.mark.parametrize("name", INSTANCE)
def test_logits_of_the_instance_norm_variants(cuda, golden_dir, name, precision):
    """max rel logits error vs the reference over t in {99, 1, 0} within 2 x the same mode's error, measured here, of the default
    variant on tests/golden/rico25_step_cases.npz (same weight seed, same t).  Measured on the MI355X:
    adainnorm 1.117e-6 exact / 9.70e-7 split, adainnorm_abs 1.091e-6 / 8.28e-7, the default variant 7.97e-7 / 6.75e-7."""
    worst = logits_error(golden_dir, name, precision)
    g = np.load(os.path.join(golden_dir, "rico25_step_cases.npz"))
    assert {99, 1, 0} <= set(g["ts"].tolist())
    base = max(_rel(engine("default", precision).denoise_logits(torch.from_numpy(g[f"tokens_{t}"].astype(np.int32)), t).cpu(),
                    torch.from_numpy(g[f"logits_{t}"])) for t in (99, 1, 0))
    d = engine(name, precision).describe()
    print(f"[{name}/{precision}] max rel logits error vs reference: {worst:.3e}; the default variant's in this mode: {base:.3e}; {d.get('kernels')}")
    assert d["kernels"] == "tiled_gemm+attn+instance_norm" and d["norm1"] == "instance" and d["per_layout_t"] == "1"
    assert d.get("timestep_emb") == ("abs" if TOOL.VARIANTS[name].is_abs else None)
    assert worst <= 2 * base


@pytest.mark.parametrize("name", TABLE_ONLY + INSTANCE)
def test_posterior_in_the_exact_mode(cuda, golden_dir, name):
    """ldm_posterior on the reference's logits against the reference's q_posterior(predict_start(...)), as
    tests/test_hip_parity.py::test_posterior_vs_reference_golden holds the default variant: 2e-4 absolute, the same argmax, the
    log(1e-30) fill exactly."""
    fx, e = fixture(golden_dir, name), engine(name, "exact")
    for t in (99, 1, 0):
        tokens = torch.from_numpy(fx[f"tokens_{t}"].astype(np.int32))
        ref = torch.from_numpy(fx[f"post_{t}"])
        out = e.posterior(torch.from_numpy(fx[f"logits_{t}"]), tokens, t).cpu()
        assert (out - ref).abs().max().item() <= 2e-4, t
        assert torch.equal(out.argmax(1), ref.argmax(1))
        dead = ref <= math.log(1e-30) + 1.0
        assert torch.equal(out[dead], ref[dead])


@pytest.mark.parametrize("precision", ["exact", "split"])
@pytest.mark.parametrize("name", TABLE_ONLY + INSTANCE)
def test_greedy_steps_teacher_forced_on_the_marked_states(cuda, golden_dir, name, precision):
    """Every marked state of the reference's greedy trajectory (num_timesteps = 10 of T = 100: skip_step = 9; the reference's own
    top-two gap exceeds 1e-3 x max |logit| at every token there): the step gives the reference's tokens exactly."""
    from layout_dm_amd.diffusion import timestep_schedule

    fx, e = fixture(golden_dir, name), engine(name, precision)
    after = torch.from_numpy(fx["traj_states_after"].astype(np.int64))
    before = torch.cat([torch.full_like(after[:1], SPEC.mask_id), after[:-1]])
    t_model, t_post = timestep_schedule(100, 10)
    assert t_model == fx["traj_steps"].tolist() and len(fx["traj_chosen"]) >= 5
    for i in fx["traj_chosen"].tolist():
        got = e.sample_step(before[i].int(), t_model[i], {"name": "deterministic"}, t_post=t_post[i]).cpu().long()
        assert torch.equal(got, after[i]), (i, int((got != after[i]).sum()))


BACKBONE = {"encoder_layer": {"d_model": 512, "nhead": 8, "dim_feedforward": 2048, "timestep_type": "adalayernorm", "diffusion_step": 100},
            "num_layers": 4}


def test_vqdiffusion_preset_runs_free_through_layoutdm_on_auto(cuda, golden_dir):
    """experiment/vqdiffusion.yaml — q_type vanilla, pos_emb default — through the drop-in class as a user builds it: precision auto,
    the checkpoint with its `model.module.` keys.  Greedy: the states after the steps the fixture marks (a prefix of the trajectory:
    up to there every decision is clear, so the free-running loop IS the reference's) are the reference's; then a stochastic call."""
    from layout_dm_amd.layoutdm import LayoutDM

    fx = fixture(golden_dir, "vanilla_default")
    v = TOOL.VARIANTS["vanilla_default"]
    m = LayoutDM(BACKBONE, StubTokenizer(SPEC), q_type="vanilla", pos_emb="default", precision="auto", max_batch=4, device=0)
    try:
        m.load_state_dict(TOOL.state_dict(v, seed=1, prefix="model.module."))
        inner = m.model.module
        assert inner.selected_precision in ("fast_verified", "hybrid_verified", "mixed_verified", "split", "exact")
        assert inner.selection_report["denoiser_variant"] == "pos_emb=default"
        assert inner.engine.describe()["pos_emb"] == "default"
        chosen = fx["traj_chosen"].tolist()
        n = next((i for i in range(10) if i not in chosen), 10)          # the marked prefix
        assert n >= 5
        states = m.model.sample(batch_size=2, sampling_cfg={"name": "deterministic", "num_timesteps": 10}, get_intermediate_results=True)
        assert len(states) == 10
        for i in range(n):
            assert torch.equal(states[i], torch.from_numpy(fx["traj_states_after"][i].astype(np.int64))), i
        assert (states[-1] != SPEC.mask_id).all()
        out = m.sample(batch_size=3, sampling_cfg={"name": "random", "temperature": 1.0, "num_timesteps": 20}, seed=5)
        assert out["bbox"].shape == (3, SPEC.max_elem, 4) and out["label"].shape == (3, SPEC.max_elem) and out["mask"].dtype == torch.bool
        assert torch.isfinite(out["bbox"]).all()
    finally:
        m.model.module.close()


def test_auto_goes_straight_to_split_for_instance_norm_and_says_why(cuda, caplog):
    import logging

    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    v = TOOL.VARIANTS["adainnorm"]
    with caplog.at_level(logging.INFO, logger="layout_dm_amd"):
        m = HipMaskAndReplaceDiffusion(n_category=SPEC.n_category, precision="auto", max_batch=2, device=0, timestep_type="adainnorm")
        try:
            m.load_state_dict(TOOL.state_dict(v, seed=1))
            assert m.selected_precision == "split" and m.verified is None
            assert m.engine.describe()["kernels"] == "tiled_gemm+attn+instance_norm"
            assert "no fp16 engine was built" in m.selection_report["reason"] and m.selection_report["denoiser_variant"] == "timestep_type=adainnorm"
        finally:
            m.close()
    assert any("timestep_type=adainnorm" in r.getMessage() and "no fp16 engine was built" in r.getMessage() for r in caplog.records)
    for precision in ("fast", "mixed", "hybrid", "fast_verified"):
        with pytest.raises(NotImplementedError, match="adainnorm / adainnorm_abs .* use precision split or exact"):
            HipMaskAndReplaceDiffusion(n_category=SPEC.n_category, precision=precision, max_batch=2, device=0, timestep_type="adainnorm_abs")


def test_finalize_names_the_keys_of_a_checkpoint_with_both_or_neither_position_table(cuda):
    from layout_dm_amd.binding import Engine

    tiny = _tiny(3)
    e = Engine(n_category=tiny.n_category, max_elem=tiny.max_elem, d_model=tiny.d_model, n_head=tiny.n_head, d_ff=tiny.d_ff,
               n_layer=tiny.n_layer, n_step=tiny.n_step, precision="exact", max_batch=2)
    try:
        sd = synthetic.synth_state_dict(tiny, seed=2, perturb=True, prefix="")
        both = {**sd, "transformer.pos_emb.pos_emb": np.zeros((tiny.seq_len, tiny.d_model), np.float32)}
        with pytest.raises(RuntimeError, match=r"pos_emb\.pos_emb .*pos_emb\.elem_emb \+ .*pos_emb\.attr_emb.*both are present"):
            e.load_state_dict(both)
    finally:
        e.close()
    e = Engine(n_category=tiny.n_category, max_elem=tiny.max_elem, d_model=tiny.d_model, n_head=tiny.n_head, d_ff=tiny.d_ff,
               n_layer=tiny.n_layer, n_step=tiny.n_step, precision="exact", max_batch=2)
    try:
        neither = {k: a for k, a in sd.items() if "pos_emb" not in k}
        with pytest.raises(RuntimeError, match=r"pos_emb\.pos_emb .*pos_emb\.elem_emb \+ .*pos_emb\.attr_emb.*neither is present"):
            e.load_state_dict(neither)
        e.load_state_dict(sd)        # ... and the handle still takes a good checkpoint
        mlp = {**sd, "transformer.backbone.layers.0.norm1.emb.1.weight": np.zeros((24, 1), np.float32)}
        with pytest.raises(RuntimeError, match=r"norm1\.emb\.1\.weight: timestep_type adalayernorm_mlp / adainnorm_mlp is not supported"):
            e.load_state_dict(mlp)
    finally:
        e.close()


# ----------------------------------------------------------------------------- the instance-norm kernel alone
def _tiny(max_elem, n_step=10):
    """one block, d_model 48 in 3 heads of 16: 48 channels on a workgroup's 256 column threads, S = 5 max_elem rows on its 4 row groups"""
    return synthetic.ModelSpec("tiny", n_category=25, max_elem=max_elem, d_model=48, n_head=3, d_ff=64, n_layer=1, n_step=n_step)


def _ln64(x):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(x.var(-1, keepdims=True) + 1e-5)


def one_block_logits(sd, spec, tokens, t):
    """float64 NumPy restatement of the one-block denoiser with norm1 = AdaInsNorm (transformer_utils.py:86-100: InstanceNorm1d over the
    sequence axis — per (layout, channel) mean and biased variance over the layout's S rows, eps 1e-5, no affine — then (1 + scale),
    shift); everything else as oracle/restatement.py denoiser_logits.  tokens (B,S), t (B,) per-layout timesteps -> (B,S,C)."""
    W = {k: np.asarray(a, np.float64) for k, a in sd.items()}
    D, H, dh = spec.d_model, spec.n_head, spec.d_model // spec.n_head
    B, S = tokens.shape
    tr, b = "transformer.", "transformer.backbone.layers.0."
    if tr + "pos_emb.pos_emb" in W:
        pos = W[tr + "pos_emb.pos_emb"][:S]
    else:
        s = np.arange(S)
        pos = W[tr + "pos_emb.elem_emb"][s // spec.n_attr] + W[tr + "pos_emb.attr_emb"][s % spec.n_attr]
    x = W[tr + "cat_emb.weight"][tokens] + pos
    e = W[b + "norm1.emb.weight"][np.asarray(t)]
    ss = (e / (1.0 + np.exp(-e))) @ W[b + "norm1.linear.weight"].T + W[b + "norm1.linear.bias"]      # (B, 2 D)
    scale, shift = ss[:, None, :D], ss[:, None, D:]
    x = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5) * (1 + scale) + shift
    qkv = x @ W[b + "self_attn.in_proj_weight"].T + W[b + "self_attn.in_proj_bias"]
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, S, H, dh).transpose(0, 2, 1, 3) for i in range(3))
    sc = q @ k.transpose(0, 1, 3, 2) / math.sqrt(dh)
    p = np.exp(sc - sc.max(-1, keepdims=True))
    a = ((p / p.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, S, D)
    x = x + a @ W[b + "self_attn.out_proj.weight"].T + W[b + "self_attn.out_proj.bias"]
    h = _ln64(x) * W[b + "norm2.weight"] + W[b + "norm2.bias"]
    x = x + np.maximum(h @ W[b + "linear1.weight"].T + W[b + "linear1.bias"], 0.0) @ W[b + "linear2.weight"].T + W[b + "linear2.bias"]
    return (_ln64(x) * W[tr + "head.0.weight"] + W[tr + "head.0.bias"]) @ W[tr + "head.1.weight"].T


def _tiny_engine(spec, sd, precision, max_batch=3, chunk=0):
    from layout_dm_amd.binding import Engine

    e = Engine(n_category=spec.n_category, max_elem=spec.max_elem, d_model=spec.d_model, n_head=spec.n_head, d_ff=spec.d_ff,
               n_layer=spec.n_layer, n_step=spec.n_step, precision=precision, max_batch=max_batch, chunk=chunk, timestep_type="adainnorm")
    e.load_state_dict(sd)
    assert e.describe()["kernels"] == "tiled_gemm+attn+instance_norm"
    return e


def _tiny_case(max_elem, B, seed):
    spec = _tiny(max_elem)
    sd = synthetic.synth_state_dict(spec, seed=seed, perturb=True, prefix="", weight_std=0.1, timestep_type="adainnorm")
    tokens = torch.from_numpy(np.random.default_rng(seed).integers(0, spec.n_class, (B, spec.seq_len)).astype(np.int32))
    return spec, sd, tokens


# (S, precisions): S = 15 on 4 row groups — groups of 4, 4, 4 and 3 rows; S = 130: past one 128-row tile, which only the fp32 attention takes
@pytest.mark.parametrize("max_elem,precision", [(3, "exact"), (3, "split"), (26, "exact")])
def test_instance_norm_kernel_alone_against_float64(cuda, max_elem, precision):
    """B = 3 layouts in chunks of 2 — a chunk boundary mid-batch — at one t, then at three distinct per-layout t in one pass."""
    spec, sd, tokens = _tiny_case(max_elem, 3, seed=7)
    e = _tiny_engine(spec, sd, precision, max_batch=3, chunk=2)
    try:
        assert e.chunk == 2
        for t in ([4, 4, 4], [9, 0, 5]):
            ref = torch.from_numpy(one_block_logits(sd, spec, tokens.numpy(), t))
            out = (e.denoise_logits(tokens, t[0]) if len(set(t)) == 1 else e.denoise_logits_t(tokens, t)).cpu().double()
            err = _rel(out, ref)
            print(f"[S={spec.seq_len}/{precision}/t={t}] max rel logits error vs float64: {err:.3e}")
            assert err <= LOGIT_REL_TOL[precision]
        # a row of the per-layout call has the bits of the single-t call at its t (include/ldm_hip.h)
        per = e.denoise_logits_t(tokens, [9, 0, 5]).cpu()
        for b, t in enumerate([9, 0, 5]):
            assert torch.equal(per[b], e.denoise_logits(tokens, t).cpu()[b]), b
    finally:
        e.close()


@pytest.mark.parametrize("precision", ["exact", "split"])
def test_instance_norm_of_equal_rows_is_exactly_the_shift(cuda, precision):
    """A layout whose rows are all equal (one token everywhere, every position row the same) has variance 0 in every channel: the
    normalised rows must be EXACTLY `shift`, whatever the rows hold — so its logits have the same bits for any token and under any
    scale row, and are those of the float64 restatement.  (A residue of one float32 ulp of the row — 6e-8 — times 1 / sqrt(eps) = 316
    times (1 + scale) would show in the bits.)  The other layouts of the batch are ordinary ones."""
    spec, sd, tokens = _tiny_case(3, 3, seed=11)
    sd["transformer.pos_emb.elem_emb"][:] = sd["transformer.pos_emb.elem_emb"][0]
    sd["transformer.pos_emb.attr_emb"][:] = sd["transformer.pos_emb.attr_emb"][0]
    D = spec.d_model
    other = {k: a.copy() for k, a in sd.items()}
    other["transformer.backbone.layers.0.norm1.linear.weight"][:D] *= -3.0       # another scale row, the same shift row
    other["transformer.backbone.layers.0.norm1.linear.bias"][:D] += 0.7
    outs = []
    for weights, tok in ((sd, 3), (sd, 140), (other, 77)):
        tk = tokens.clone()
        tk[1] = tok
        e = _tiny_engine(spec, weights, precision)
        try:
            outs.append(e.denoise_logits(tk, 6).cpu())
        finally:
            e.close()
        ref = torch.from_numpy(one_block_logits(weights, spec, tk.numpy(), [6, 6, 6]))
        assert _rel(outs[-1].double(), ref) <= LOGIT_REL_TOL[precision]
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][1], outs[2][1])
    assert not torch.equal(outs[0][0], outs[2][0])      # (an ordinary layout does see the other scale row)
