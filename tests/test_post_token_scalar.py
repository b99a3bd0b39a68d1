"""CPU: the per-token scalar tail of a reverse step (layout_dm_amd/csrc/ldm_post_token.h — log-softmax, constrained
posterior on the token's sub-vocabulary, cond overrides, draw with the kernel's Philox stream), compiled for the host and
run against the oracle on states of the REFERENCE's trajectories (tests/golden): greedy tokens, and stochastic draws on
identical uniforms for random / top-k / top-p, and for gumbel on identical per-class noise words; the same over the
parameter edges of top-k / top-p / temperature (tests/_sampler_cases.py).  This is the form in which one lane of
the stack kernel can finish a token behind the fused vocabulary head."""
import io
import os
import struct

import numpy as np
import pytest
import torch

from oracle import restatement as R
from oracle import spec as SP
from oracle import synth

import _hostbuild as HB
import _sampler_cases as SC

KINDS = {"deterministic": 0, "random": 1, "top_p": 2, "top_k": 3, "gumbel": 4}
SCHED_KEYS = ("log_at", "log_bt", "log_ct", "log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct")


@pytest.fixture(scope="module")
def harness():
    return HB.host_program("cpu_post_token_check", extra=("-Wextra",))


def _run(harness, tmp_path, spec, W, tokens, t_post, logits, cfg, step, seed, first_layout, cond=None, f64=False,
         alias=True):
    """tokens (B,S) int64, logits (B,S,C) float32 -> tokens drawn by the scalar tail, (B,S) int64."""
    B, S = tokens.shape
    C, A, T = spec.n_class, spec.n_attr, spec.n_step
    N = B * S
    pos = np.tile(np.arange(S, dtype=np.int32), B)
    attr = pos % A
    start = np.array([int(spec.full_ids(a)[0]) for a in range(A)], np.int32)[attr]
    count = np.array([len(spec.full_ids(a)) - 2 for a in range(A)], np.int32)[attr]
    u = (t_post - 1 + (T + 1)) % (T + 1)  # constrained.py:114
    sched = np.zeros((A, 10), np.float32)
    for a, key in enumerate(SP.VAR_NAMES):
        g = lambda n, i: float(W[f"{key}_{n}"][i])
        sched[a] = [g("log_at", t_post), g("log_bt", t_post), g("log_ct", t_post),
                    g("log_cumprod_at", t_post), g("log_cumprod_bt", t_post), g("log_cumprod_ct", t_post),
                    g("log_cumprod_at", u), g("log_cumprod_bt", u), g("log_cumprod_ct", u),
                    g("log_1_min_cumprod_ct", u)]
    cond_tok = np.full(N, -1, np.int32)
    strong = np.zeros(N, np.int32)
    pad_dis = np.zeros(N, np.int32)
    weak = None
    if cond is not None:
        cs = np.asarray(cond["seq"]).reshape(-1).astype(np.int32)
        cond_tok = cs
        strong = np.asarray(cond["mask"]).reshape(-1).astype(np.int32)
        if cond.get("type") in ("c", "cwh", "refinement", "relation"):  # base.py:272-284
            pad_dis = ((attr != 0) & (cs != spec.pad_id)).astype(np.int32)
        if cond.get("type") == "refinement":
            weak = np.ascontiguousarray(np.asarray(cond["weak_logits"], np.float32).transpose(0, 2, 1)).reshape(N, C)
    layout = (np.repeat(np.arange(B, dtype=np.uint64), S) + np.uint64(first_layout))
    with io.BytesIO() as f:
        f.write(np.array([0x4C444D31, N, C, spec.pad_id, spec.mask_id, KINDS[cfg["name"]], int(cfg.get("top_k", 1)),
                          1 if f64 else 0, 1 if weak is not None else 0, 1 if alias else 0], np.int32).tobytes())
        f.write(np.array([cfg.get("temperature", 1.0), cfg.get("top_p", 1.0)], np.float32).tobytes())
        f.write(struct.pack("<Q", seed))
        for arr in (tokens.numpy().reshape(-1).astype(np.int32), start, count, cond_tok, strong, pad_dis, pos,
                    np.full(N, step, np.int32)):
            f.write(np.ascontiguousarray(arr, np.int32).tobytes())
        f.write(layout.tobytes())
        f.write(np.ascontiguousarray(sched[attr], np.float32).tobytes())
        f.write(np.ascontiguousarray(logits.numpy().reshape(N, -1)[:, :C], np.float32).tobytes())
        if weak is not None:
            f.write(weak.tobytes())
        rc, raw = HB.run_host_io(harness, tmp_path, f.getvalue())
    assert rc == 0, rc
    return torch.from_numpy(np.frombuffer(raw, np.int32).astype(np.int64)).view(B, S)


def _weights(ds):
    spec = SP.SPECS[ds]
    return spec, R.as_torch_weights(synth.synth_state_dict(spec, seed=1, perturb=True))


@pytest.mark.parametrize("f64", [True, False], ids=["f64_lse", "f32_lse"])
def test_scalar_tail_greedy_equals_reference_tokens(harness, tmp_path, golden_dir, f64):
    """Greedy: the reference's own argmax tokens on states of its stochastic trajectories (uncond, cond=c with the
    strong mask and the [PAD] disable, refinement with the additive prior)."""
    cases = []
    spec, W = _weights("rico25")
    g = np.load(os.path.join(golden_dir, "rico25_uncond_trajectory.npz"))
    cases.append((spec, W, g, None))
    g = np.load(os.path.join(golden_dir, "rico25_refinement_trajectory.npz"))
    table = torch.from_numpy(g["weak_table"])
    seq_orig = torch.from_numpy(g["seq_orig"].astype(np.int64))
    cases.append((spec, W, g, {"seq": g["cond_seq"].astype(np.int64), "mask": g["cond_mask"], "type": "refinement",
                               "weak_logits": table[seq_orig].permute(0, 2, 1).contiguous().numpy()}))
    spec_p, W_p = _weights("publaynet")
    g = np.load(os.path.join(golden_dir, "publaynet_cond_c_trajectory.npz"))
    cases.append((spec_p, W_p, g, {"seq": g["cond_seq"].astype(np.int64), "mask": g["cond_mask"], "type": "c"}))
    gv = np.load(os.path.join(golden_dir, "rico25_cond_variants.npz"))
    for ctype in ("cwh", "partial"):  # helpers/task.py:61-110
        sub = {k[len(ctype) + 1:]: gv[k] for k in gv.files if k.startswith(ctype + "_")}
        cases.append((spec, W, sub, {"seq": sub["cond_seq"].astype(np.int64), "mask": sub["cond_mask"], "type": ctype}))
    bad = total = 0
    for spec, W, g, cond in cases:
        for i in (0, 25, 50, 75, 99):
            t = int(g["steps"][i])
            toks = torch.from_numpy(g["states_before"][i].astype(np.int64))
            logits = R.denoiser_logits(W, spec, toks, t)
            # working storage: a separate buffer for the even states, the token's own logits row (as in the kernel) for the odd
            out = _run(harness, tmp_path, spec, W, toks, t, logits, {"name": "deterministic"}, i, 0, 0, cond, f64=f64,
                       alias=bool(i & 1))
            ref = torch.from_numpy(g["greedy_next"][i].astype(np.int64))
            mism = out != ref
            if mism.any():  # only where the reference's own top-2 margin is at the fp32 rounding level
                assert float(torch.from_numpy(g["greedy_margin"][i])[mism].max()) < 1e-4
            bad += int(mism.sum())
            total += ref.numel()
    assert bad <= (0 if f64 else 2), f"{bad}/{total}"


DRAW_CFGS = [{"name": "random", "temperature": 1.0}, {"name": "random", "temperature": 0.7},
             {"name": "top_k", "top_k": 5, "temperature": 1.0}, {"name": "top_p", "top_p": 0.9, "temperature": 1.0}]


@pytest.mark.parametrize("cfg", DRAW_CFGS, ids=["random", "random_T0.7", "top_k5", "top_p0.9"])
def test_scalar_tail_draws_equal_oracle_on_identical_uniforms(harness, tmp_path, golden_dir, cfg):
    """Stochastic samplers: same Philox uniforms (seed, global layout index, step, position) as the oracle's inverse-CDF
    rule, i.e. as the wave-per-token kernel: token for token, except where fp32 rounding moves a CDF edge across u."""
    spec, W = _weights("rico25")
    g = np.load(os.path.join(golden_dir, "rico25_uncond_trajectory.npz"))
    bad = total = 0
    for i in (3, 40, 80, 99):
        t = int(g["steps"][i])
        toks = torch.from_numpy(g["states_before"][i].astype(np.int64))
        B, S = toks.shape
        logits = R.denoiser_logits(W, spec, toks, t)
        out = _run(harness, tmp_path, spec, W, toks, t, logits, cfg, i, 1234567890123, 500)
        u = R.token_uniforms(1234567890123, 500, B, S, i)[..., 0]
        ref = R.single_step(W, spec, toks, t, cfg, uniforms=u)
        bad += int((out != ref).sum())
        total += ref.numel()
    assert bad <= 2, f"{bad}/{total}"


def test_scalar_tail_gumbel_support_and_determinism(harness, tmp_path, golden_dir):
    spec, W = _weights("rico25")
    g = np.load(os.path.join(golden_dir, "rico25_uncond_trajectory.npz"))
    i = 60
    t = int(g["steps"][i])
    toks = torch.from_numpy(g["states_before"][i].astype(np.int64))
    logits = R.denoiser_logits(W, spec, toks, t)
    cfg = {"name": "gumbel", "temperature": 1.0}
    a = _run(harness, tmp_path, spec, W, toks, t, logits, cfg, i, 99, 0)
    b = _run(harness, tmp_path, spec, W, toks, t, logits, cfg, i, 99, 0)
    c = _run(harness, tmp_path, spec, W, toks, t, logits, cfg, i, 100, 0)
    assert torch.equal(a, b) and not torch.equal(a, c)
    for at in range(spec.n_attr):
        assert torch.isin(a[:, at::spec.n_attr], torch.as_tensor(spec.full_ids(at))).all()


# ----------------------------------------------------------------------------- gumbel on explicit Philox noise
GUMBEL_STATES = (3, 40, 80, 99)   # the states of test_scalar_tail_draws_equal_oracle_on_identical_uniforms


def _gumbel_case(harness, tmp_path, golden_dir, cfg):
    """[(host tokens, oracle logp, loop index)] over GUMBEL_STATES."""
    spec, W = _weights("rico25")
    g = np.load(os.path.join(golden_dir, "rico25_uncond_trajectory.npz"))
    out = []
    for i in GUMBEL_STATES:
        t = int(g["steps"][i])
        toks = torch.from_numpy(g["states_before"][i].astype(np.int64))
        _, logits, logp = R.single_step(W, spec, toks, t, {"name": "deterministic"}, return_all=True)
        out.append((_run(harness, tmp_path, spec, W, toks, t, logits, cfg, i, SC.SEED, SC.FIRST_LAYOUT), logp, i))
    return out


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_scalar_tail_gumbel_equals_oracle_on_identical_words(harness, tmp_path, golden_dir, temperature):
    """gumbel: logp / T + noise(u_c) with the per-class uniforms of R.token_gumbel_uniforms (counter word 0 =
    pos | (1 + c / 4) << 16, component c & 3), then the inverse CDF on the draw's own uniform: token for token against
    R.single_step's draw, with the file's allowance for a CDF edge within fp32 rounding of u.  T = 0.7 tells
    l / T + g from (l + g) / T."""
    cfg = {"name": "gumbel", "temperature": temperature}
    bad = total = 0
    for out, logp, i in _gumbel_case(harness, tmp_path, golden_dir, cfg):
        ref = SC.oracle_draw(logp, cfg, i)
        assert SC.support(logp, cfg).gather(1, out[:, None, :]).all()
        bad += int((out != ref).sum())
        total += ref.numel()
    print(f"[host form, gumbel T={temperature}] tokens differing from the oracle on identical words: {bad}/{total}")
    assert bad <= 2, f"{bad}/{total}"


WRONG_NOISE = ["no_noise", "shared_across_classes", "before_division", "draw_word_reused"]


@pytest.mark.parametrize("variant", WRONG_NOISE)
def test_scalar_tail_gumbel_parity_rejects_wrong_noise(harness, tmp_path, golden_dir, variant):
    """The parity check above is not vacuous: against an oracle whose noise is missing, shared by the classes of a token
    (it cancels in the softmax), added before the temperature division, or taken from the draw's own Philox block, the
    same comparison at T = 0.7 exceeds the `bad <= 2` allowance by far (at least 1 % of the tokens: five times the
    largest share any device parity test allows, 2e-3)."""
    cfg = {"name": "gumbel", "temperature": 0.7}
    bad = total = 0
    for out, logp, i in _gumbel_case(harness, tmp_path, golden_dir, cfg):
        bad += int((out != SC.wrong_gumbel_draw(logp, cfg, i, variant)).sum())
        total += out.numel()
    print(f"[host form vs WRONG oracle: {variant}] {bad}/{total}")
    assert bad > 2 and bad >= 0.01 * total, f"{variant}: {bad}/{total}"


def test_oracle_gumbel_noise_changes_the_draws(golden_dir):
    """Oracle alone: on the same draw uniform, the tokens drawn with gumbel noise differ from the noise-free `random`
    draws for a large share of the tokens — at least 5 %, ten times the widest device parity bound (5e-3) — so parity
    on these inputs cannot be met by a sampler that drops or cancels the noise.  Counter word 1 matters too: the noise
    of step i differs from that of step 0."""
    spec, W = _weights("rico25")
    g = np.load(os.path.join(golden_dir, "rico25_uncond_trajectory.npz"))
    diff = total = 0
    for i in GUMBEL_STATES:
        toks = torch.from_numpy(g["states_before"][i].astype(np.int64))
        logp = SC.oracle_logp(W, spec, toks, int(g["steps"][i]))
        with_noise = SC.oracle_draw(logp, {"name": "gumbel", "temperature": 1.0}, i)
        without = SC.oracle_draw(logp, {"name": "random", "temperature": 1.0}, i)
        # without explicit noise a seeded gumbel draw keeps its earlier meaning (plain random): golden tests rely on it
        B, S = toks.shape
        u = R.token_uniforms(SC.SEED, SC.FIRST_LAYOUT, B, S, i)[..., 0]
        assert torch.equal(R.sample_tokens(logp, {"name": "gumbel", "temperature": 1.0}, uniforms=u), without)
        diff += int((with_noise != without).sum())
        total += without.numel()
    print(f"[oracle] gumbel vs noise-free draws on the same uniform: {diff}/{total} differ")
    assert diff >= 0.05 * total, f"{diff}/{total}"
    a = R.token_gumbel_uniforms(7, 3, 2, 5, 4, spec.n_class)
    assert a.shape == (2, spec.n_class, 5) and a.dtype == np.float32 and (a > 0).all() and (a < 1).all()
    assert not np.array_equal(a, R.token_gumbel_uniforms(7, 3, 2, 5, 0, spec.n_class))
    # the noise words are disjoint from the draw's word (counter word 0 = pos, component 0)
    d = R.token_uniforms(7, 3, 2, 5, 4, n=4)
    assert not np.isin(a, d).any()


# ----------------------------------------------------------------------------- parameter edges
@pytest.mark.parametrize("ds", ["rico25", "publaynet"])
def test_scalar_tail_parameter_edges(harness, tmp_path, golden_dir, ds):
    """top_k = 1 / at, above every sub-vocabulary size / = C, top_p = 1 and below the largest probability, temperatures
    0.05 .. the largest the live-class forms admit (SC.edge_cfgs) on states of the reference's trajectories (Rico25
    unconditional; PubLayNet cond=c: strong mask + [PAD] disable), against R.single_step's draw on identical uniforms.
    top_p = 1.0 is held to "nothing but rounding may be cut" (SC.top_p_one_mismatch).  Allowance: the file's rate of CDF-edge roundings (2 per 2 000 tokens) on the 4 000 tokens of each setting; never a
    token outside the oracle's support; top_k = 1 is the argmax wherever the oracle's top-2 gap exceeds fp32 rounding."""
    spec, W = _weights(ds)
    states, cond = SC.load_states(golden_dir, ds)
    cfgs = SC.edge_cfgs(spec)
    bad = {k: 0 for k, _ in cfgs}
    total = raw_top_p_one = 0
    for i, t, toks in states:
        _, logits, logp = R.single_step(W, spec, toks, t, {"name": "deterministic"}, cond, return_all=True)
        top2 = logp.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-4
        total += toks.numel()
        for name, cfg in cfgs:
            out = _run(harness, tmp_path, spec, W, toks, t, logits, cfg, i, SC.SEED, SC.FIRST_LAYOUT, cond)
            sup_cfg = {"name": "random", "temperature": 1.0} if name == "top_p1.0" else cfg   # (its cut is rounding: below)
            assert SC.support(logp, sup_cfg).gather(1, out[:, None, :]).all(), (name, i)
            if name == "top_p1.0":  # nothing but rounding may be cut: see SC.top_p_one_mismatch
                raw_top_p_one += int((out != SC.oracle_draw(logp, cfg, i)).sum())
                bad[name] += int(SC.top_p_one_mismatch(out, logp, cfg, i).sum())
                continue
            bad[name] += int((out != SC.oracle_draw(logp, cfg, i)).sum())
            if name == "top_k1":
                assert torch.equal(out[clear], logp.argmax(1)[clear]), i
            if name == "top_p1e-3":  # only the first maximum survives: no randomness left
                assert torch.equal(out[clear], logp.argmax(1)[clear]), i
    print(f"[host form, {ds}] mismatches per setting over {total} tokens: {bad}; top_p = 1.0 against the oracle's own "
          f"float32 cumsum: {raw_top_p_one}")
    assert max(bad.values()) <= 2 * total // 2000, bad


def test_live_class_form_needs_the_temperature_bound(harness, tmp_path, golden_dir):
    """The live-class forms leave a token's dead classes (log(1e-30) each) out of the draw.  The reference divides by the
    temperature first, so the dead classes hold C exp(log(1e-30) / T) of the mass: 2^-24 at SC.max_live_temperature(C)
    (3.19 for the 155 classes of Rico25); at T = 10 the 121 dead classes of a bin token hold 121 * 1e-3 against a live mass of
    at most 34 (34 live classes, each p^(1/10) <= 1), i.e. >= 0.35 % of the draws.  Inside the bound the live-class form (this host build
    IS one: SlotMap<1, 64, LIVE>) draws the oracle's tokens; at T = 10 it cannot draw the dead classes the oracle draws —
    which is why ldm_sample_step / ldm_sample_loop refuse such a temperature instead of approximating
    (tests/test_sampler_edges_gpu.py::test_temperature_contract)."""
    spec, W = _weights("rico25")
    C = spec.n_class
    assert 3.1 < SC.max_live_temperature(C) < 3.3
    assert C * np.exp(SP.LOG_EPS / SC.admitted_temperature(C)) <= 2.0 ** -24 < C * np.exp(SP.LOG_EPS / (1.01 * SC.max_live_temperature(C)))
    states, _ = SC.load_states(golden_dir, "rico25", steps=(3, 40, 80, 99))
    dead_drawn = bad = total = 0
    for i, t, toks in states:
        _, logits, logp = R.single_step(W, spec, toks, t, {"name": "deterministic"}, return_all=True)
        cfg = {"name": "random", "temperature": 10.0}
        out = _run(harness, tmp_path, spec, W, toks, t, logits, cfg, i, SC.SEED, SC.FIRST_LAYOUT)
        ref = SC.oracle_draw(logp, cfg, i)
        dead_drawn += int((logp.gather(1, ref[:, None, :]) == logp.min()).sum())
        bad += int((out != ref).sum())
        total += ref.numel()
    print(f"[host live-class form, T=10] oracle draws on dead classes {dead_drawn}/{total}; tokens differing {bad}/{total}")
    assert dead_drawn >= 0.002 * total     # the reference's distribution does put >= 0.35 % of its mass there (docstring)
    assert bad >= dead_drawn               # ... and the live-class form can follow none of those draws


def test_scalar_tail_under_address_and_undefined_sanitizers(tmp_path, golden_dir):
    """every case above once more on the ASan + UBSan build of the same program: the tail indexes the token's logits row, its
    working storage (aliased onto that row or separate) and the sub-vocabulary slots by formulas the kernel shares; a read or
    write past any of them, or signed overflow in the index arithmetic, ends the run with a non-zero code"""
    exe = HB.host_program("cpu_post_token_check", sanitize=True, extra=("-Wextra",))
    for f64 in (True, False):
        test_scalar_tail_greedy_equals_reference_tokens(exe, tmp_path, golden_dir, f64)
    for cfg in DRAW_CFGS:
        test_scalar_tail_draws_equal_oracle_on_identical_uniforms(exe, tmp_path, golden_dir, cfg)
    test_scalar_tail_gumbel_support_and_determinism(exe, tmp_path, golden_dir)
    for temperature in (1.0, 0.7):
        test_scalar_tail_gumbel_equals_oracle_on_identical_words(exe, tmp_path, golden_dir, temperature)
    for variant in WRONG_NOISE:
        test_scalar_tail_gumbel_parity_rejects_wrong_noise(exe, tmp_path, golden_dir, variant)
    for ds in ("rico25", "publaynet"):
        test_scalar_tail_parameter_edges(exe, tmp_path, golden_dir, ds)
    test_live_class_form_needs_the_temperature_bound(exe, tmp_path, golden_dir)
