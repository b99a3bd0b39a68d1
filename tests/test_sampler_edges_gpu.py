"""GPU: the stochastic samplers of the three lane-group forms of layout_dm_amd/csrc/ldm_post_token.h::draw_token

    tokens   ldm_sample_tokens                     DppGroup<64>, full vocabulary, (B,C,S) log-probabilities in
    exact    ldm_sample_step, `exact` engine       posterior_sample_k, DppGroup<16>, live classes
    fast     ldm_sample_step, `fast` engine        tail of the stack kernel, DppGroup<16>, live classes

against the oracle (oracle/restatement.py) on identical Philox words: gumbel with its per-class noise, the parameter
edges of top-k / top-p / temperature (tests/_sampler_cases.py), the reference-made probabilities of
tests/golden/rico25_cond_variants.npz, the argument checks, and the temperature bound of the live-class forms."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import _sampler_cases as SC
from oracle import restatement as R
from oracle import spec as SP
from test_hip_parity import cuda, engine, weights  # noqa: F401  (fixture + shared helpers)

pytestmark = pytest.mark.gpu

EDGE_BOUND = 2e-3                                   # test_sampler_deterministic_and_inverse_cdf's CDF-edge bound
STEP_BOUND = {"exact": 1e-3, "fast": 5e-3}          # what a whole loop is allowed against the oracle (test_hip_parity.py)


def _draw(form, ds, logp, toks, t, cfg, step, cond=None):
    """One draw of `form` on the Philox words of (SC.SEED, SC.FIRST_LAYOUT + layout, step, position) -> (B,S) int64 cpu."""
    kw = dict(seed=SC.SEED, first_layout=SC.FIRST_LAYOUT, step=step)
    if form == "tokens":
        return engine(ds, "exact").sample_tokens(logp, cfg, **kw).cpu().long()
    return engine(ds, form).sample_step(toks.int(), t, cfg, cond=cond, **kw).cpu().long()


# ----------------------------------------------------------------------------- gumbel
def test_gumbel_full_vocabulary_form_equals_oracle(cuda):  # noqa: F811
    """ldm_sample_tokens, B = 64, on the log-probabilities of test_sampler_deterministic_and_inverse_cdf."""
    spec = SP.RICO25
    e = engine("rico25", "exact", max_batch=64)
    B = 64
    logp = torch.log_softmax(3.0 * torch.randn(B, spec.n_class, spec.seq_len, generator=torch.Generator().manual_seed(0)), dim=1)
    u = R.token_uniforms(11, 5, B, spec.seq_len, 42)[..., 0]
    gu = R.token_gumbel_uniforms(11, 5, B, spec.seq_len, 42, spec.n_class)
    for T in (1.0, 0.7):
        cfg = {"name": "gumbel", "temperature": T}
        out = e.sample_tokens(logp, cfg, seed=11, first_layout=5, step=42).cpu().long()
        ref = R.sample_tokens(logp, cfg, uniforms=u, gumbel_uniforms=gu)
        frac = (out != ref).float().mean().item()
        plain = (out != R.sample_tokens(logp, cfg, uniforms=u)).float().mean().item()
        print(f"[gumbel / tokens T={T}] share differing from the oracle: {frac:.2e} (bound {EDGE_BOUND:.0e}); from the "
              f"noise-free draw: {plain:.3f}")
        assert frac <= EDGE_BOUND, (T, frac)
        assert plain > 0.05                      # the inputs discriminate


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_gumbel_step_equals_oracle(cuda, golden_dir, precision):  # noqa: F811
    """ldm_sample_step against R.single_step with noise, teacher-forced on eight states of the reference's trajectory;
    T = 0.7 tells l / T + g from (l + g) / T.  A single step may not exceed what a whole loop is allowed."""
    spec, W = weights("rico25")
    states, _ = SC.load_states(golden_dir, "rico25")
    for T in (1.0, 0.7):
        cfg = {"name": "gumbel", "temperature": T}
        bad = total = 0
        for i, t, toks in states:
            logp = SC.oracle_logp(W, spec, toks, t)
            out = _draw(precision, "rico25", logp, toks, t, cfg, i)
            assert SC.support(logp, cfg).gather(1, out[:, None, :]).all()
            bad += int((out != SC.oracle_draw(logp, cfg, i)).sum())
            total += out.numel()
        print(f"[gumbel / {precision} step T={T}] tokens differing from the oracle: {bad}/{total} = {bad / total:.2e} "
              f"(bound {STEP_BOUND[precision]:.0e})")
        assert bad <= STEP_BOUND[precision] * total, (T, bad, total)


def test_gumbel_fast_loop_equals_oracle(cuda):  # noqa: F811
    """The one-launch loop of the fast mode, B = 5, all 100 steps with their intermediates, against R.sample_loop with
    the noise of every step: counter word 1 advances with the step (noise frozen at step 0 fails from step 1 on)."""
    spec, W = weights("rico25")
    e = engine("rico25", "fast")
    B = 5
    cfg = {"name": "gumbel", "temperature": 1.0}
    steps = R.timestep_list(spec.n_step, 100)
    tok = torch.full((B, spec.seq_len), spec.mask_id, dtype=torch.int32, device=cuda)
    out, inter = e.sample_loop(tok, steps, steps, cfg, seed=321, first_layout=70, intermediates=True)
    ref = torch.stack(R.sample_loop(W, spec, B, cfg, seed=321, first_layout=70, get_intermediate_results=True,
                                    gumbel_noise=True)).int()
    diff = inter.cpu() != ref
    frac = diff.float().mean().item()
    print(f"[gumbel / fast loop, B={B}] tokens differing from the oracle: {int(diff.sum())}/{diff.numel()} = {frac:.2e} "
          f"(bound 5e-03); layouts that diverged: {int(diff.any(dim=2).any(dim=0).sum())}/{B}")
    assert frac <= 5e-3, frac
    assert (out.cpu() != spec.mask_id).all()


# ----------------------------------------------------------------------------- parameter edges
@pytest.mark.parametrize("form", ["tokens", "exact", "fast"])
@pytest.mark.parametrize("ds", ["rico25", "publaynet"])
def test_parameter_edges_equal_oracle(cuda, golden_dir, ds, form):  # noqa: F811
    """SC.edge_cfgs on states of the reference's trajectories (Rico25 unconditional; PubLayNet cond=c).  Per setting at
    most 2e-3 of the tokens differ from the oracle's draw on identical uniforms; never a token outside the oracle's
    support (tokens / exact: strictly; fast: its fp16 logits carry up to 1e-3 of error per class, which lets two classes closer
    than 2e-3 change places at a top-k / top-p boundary, so a class counts as supported when errors of that size could
    admit it, SC.support); top_k = 1 and top_p below the largest probability are the argmax wherever the oracle's top-2
    gap is beyond the form's numerics; top_p = 1.0 is held to "nothing but rounding may be cut" (SC.top_p_one_mismatch)."""
    spec, W = weights(ds)
    states, cond = SC.load_states(golden_dir, ds)
    cfgs = SC.edge_cfgs(spec)
    bad = {k: 0 for k, _ in cfgs}
    total = raw = 0
    gap_bound = 2e-3 if form == "fast" else 1e-4     # MARGIN_BOUND of test_hip_parity.py
    slack = 1e-3 if form == "fast" else 0.0          # per-class error of the fp16 logits: half the gap bound (SC.support)
    for i, t, toks in states:
        logp = SC.oracle_logp(W, spec, toks, t, cond)
        top2 = logp.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > gap_bound
        total += toks.numel()
        for name, cfg in cfgs:
            out = _draw(form, ds, logp, toks, t, cfg, i, cond)
            sup_cfg = {"name": "random", "temperature": 1.0} if name == "top_p1.0" else cfg   # (its cut is rounding: below)
            assert SC.support(logp, sup_cfg, slack).gather(1, out[:, None, :]).all(), (name, i)
            if name == "top_p1.0":
                raw += int((out != SC.oracle_draw(logp, cfg, i)).sum())
                bad[name] += int(SC.top_p_one_mismatch(out, logp, cfg, i).sum())
                continue
            bad[name] += int((out != SC.oracle_draw(logp, cfg, i)).sum())
            if name in ("top_k1", "top_p1e-3"):
                assert torch.equal(out[clear], logp.argmax(1)[clear]), (name, i)
    worst = max(bad.values())
    print(f"[edges / {ds} / {form}] mismatches per setting over {total} tokens (bound {EDGE_BOUND * total:.0f}): {bad}; "
          f"top_p = 1.0 against the oracle's own float32 cumsum: {raw}")
    assert worst <= EDGE_BOUND * total, bad


def _row(spec, entries):
    row = torch.full((spec.n_class,), SP.LOG_EPS)
    for c, p in entries.items():
        row[c] = math.log(p)
    return row


def test_hand_made_rows_ties_and_cumulative_edges(cuda):  # noqa: F811
    """ldm_sample_tokens on hand-made rows, 8 000 draws each (every surviving class has probability >= 0.1):
    top-k keeps every value not below the k-th (sampling.py:73-78), so a tie at the k-th value survives whole; top-p cuts a
    class whose cumulative probability EXCEEDS top_p — with top_p eight float32 ulps above a cumulative edge the class at
    the edge stays, eight below it goes."""
    spec = SP.RICO25
    B = 64
    e = engine("rico25", "exact", max_batch=64)

    def drawn(row, cfg):
        logp = row.view(1, -1, 1).repeat(B, 1, spec.seq_len).contiguous()
        out = e.sample_tokens(logp, cfg, seed=5, step=1).cpu().long()
        ref = R.sample_tokens(logp, cfg, uniforms=R.token_uniforms(5, 0, B, spec.seq_len, 1)[..., 0])
        assert (out != ref).float().mean().item() <= EDGE_BOUND, cfg
        return sorted(np.unique(out.numpy()).tolist())

    tie = _row(spec, {90: 0.3, 5: 0.3, 40: 0.2, 7: 0.1, 120: 0.1})
    assert drawn(tie, {"name": "top_k", "top_k": 1, "temperature": 1.0}) == [5, 90]          # tie of the two largest
    assert drawn(tie, {"name": "top_k", "top_k": 2, "temperature": 1.0}) == [5, 90]
    assert drawn(tie, {"name": "top_k", "top_k": 3, "temperature": 1.0}) == [5, 40, 90]
    assert drawn(tie, {"name": "top_k", "top_k": 4, "temperature": 0.5}) == [5, 7, 40, 90, 120]  # tie at the 4th value
    assert drawn(tie, {"name": "top_k", "top_k": spec.n_class, "temperature": 1.0}) == [5, 7, 40, 90, 120]
    row = _row(spec, {10: 0.4, 3: 0.3, 40: 0.2, 7: 0.1})
    ulp = 2.0 ** -24
    for edge, inside, outside in ((0.7, [3, 10], [10]), (0.9, [3, 10, 40], [3, 10])):
        assert drawn(row, {"name": "top_p", "top_p": edge * (1 + 8 * ulp), "temperature": 1.0}) == inside
        assert drawn(row, {"name": "top_p", "top_p": edge * (1 - 8 * ulp), "temperature": 1.0}) == outside
    assert drawn(row, {"name": "top_p", "top_p": 0.39, "temperature": 1.0}) == [10]            # below the largest
    assert drawn(row, {"name": "random", "temperature": 0.01}) == [10]                          # 0.75^100 = 3e-13
    assert drawn(row, {"name": "top_k", "top_k": 1, "temperature": 1.0}) == [10]


def test_step_draws_follow_the_reference_made_probabilities(cuda, golden_dir):  # noqa: F811
    """The probabilities the REFERENCE handed to torch.multinomial (rico25_cond_variants.npz: top-k 5 at T 0.7, plain
    T 0.6, top-p 0.8 at T 1.3, on states of its cond=cwh run): ldm_sample_step of the exact engine under the fixture's
    cond, each state tiled to 510 layouts (the Philox words are keyed by the global layout index: 170 independent draws
    per token).  Every drawn token has reference probability > 0.  Chi-square per (setting, state), pooled by class over
    the positions that are not strong-masked: the positions are independent multinomials with different rows, whose
    summed class counts have at most the variance of ONE multinomial with the averaged row, so the usual bound
    dof + 6 sqrt(2 dof) + 10 holds for the pooled statistic."""
    spec = SP.RICO25
    g = np.load(os.path.join(golden_dir, "rico25_cond_variants.npz"))
    rep = 170
    e = engine("rico25", "exact", max_batch=512)
    seq = torch.from_numpy(g["cwh_cond_seq"].astype(np.int64)).repeat(rep, 1)
    mask = torch.from_numpy(g["cwh_cond_mask"]).repeat(rep, 1)
    cond = {"seq": seq, "mask": mask, "type": "cwh"}
    free = ~torch.from_numpy(g["cwh_cond_mask"])
    cfgs = {"top_k": {"name": "top_k", "top_k": 5, "temperature": 0.7}, "temp": {"name": "random", "temperature": 0.6},
            "top_p_temp": {"name": "top_p", "top_p": 0.8, "temperature": 1.3}}
    for name, cfg in cfgs.items():
        for i in (0, 60, 99):
            toks = torch.from_numpy(g["cwh_states_before"][i].astype(np.int32)).repeat(rep, 1)
            p = torch.from_numpy(g[f"probs_{name}_{i}"])                       # (3, C, S)
            out = e.sample_step(toks, int(g["cwh_steps"][i]), cfg, cond=cond, seed=17, step=i).cpu().long()
            assert (p.repeat(rep, 1, 1).gather(1, out[:, None, :]) > 0).all(), (name, i)
            sel = free.repeat(rep, 1)
            pbar = p.permute(0, 2, 1)[free].double().mean(0).numpy()
            chi2, dof, bound, off, n_off = SC.chi_square(out[sel].numpy(), pbar / pbar.sum(), spec.n_class)
            print(f"[reference-made probabilities / {name} / state {i}] chi2 {chi2:.1f} dof {dof} bound {bound:.1f} "
                  f"({int(sel.sum())} draws)")
            assert off <= 5 * n_off + 10
            assert chi2 < bound, (name, i, chi2, dof)


# ----------------------------------------------------------------------------- argument checks
def _bad_samplers(n_class):
    from layout_dm_amd.binding import LdmSampler

    return [("temperature must be > 0", LdmSampler(1, 0.0, 1.0, 1)), ("temperature must be > 0", LdmSampler(4, -1.0, 1.0, 1)),
            ("temperature must be > 0", LdmSampler(2, float("nan"), 0.9, 1)), ("top_p must be in", LdmSampler(2, 1.0, 0.0, 1)),
            ("top_p must be in", LdmSampler(2, 1.0, 1.0001, 1)), ("top_p must be in", LdmSampler(2, 1.0, float("nan"), 1)),
            ("top_k out of range", LdmSampler(3, 1.0, 1.0, 0)), ("top_k out of range", LdmSampler(3, 1.0, 1.0, n_class + 1)),
            ("unknown sampler kind", LdmSampler(5, 1.0, 1.0, 1))]


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_invalid_sampler_arguments_are_refused_before_any_launch(cuda, precision):  # noqa: F811
    """ldm_loop.cpp check_sampler through the three entry points: an error code, its text in ldm_last_error, and the
    output buffers untouched (nothing was launched)."""
    spec = SP.RICO25
    e = engine("rico25", precision)
    B, S, Cn = 2, spec.seq_len, spec.n_class
    logp = torch.zeros(B, Cn, S, device=cuda)
    tin = torch.full((B, S), spec.mask_id, dtype=torch.int32, device=cuda)
    tm = (C.c_int32 * 2)(50, 49)
    for text, s in _bad_samplers(Cn):
        calls = {
            "ldm_sample_tokens": lambda out: e.lib.ldm_sample_tokens(e._h, logp.data_ptr(), None, C.byref(s), 1, 0, 0, B,
                                                                      out.data_ptr(), None),
            "ldm_sample_step": lambda out: e.lib.ldm_sample_step(e._h, tin.data_ptr(), out.data_ptr(), 50, 50, None, None,
                                                                  C.byref(s), 1, 0, 0, B, None),
            "ldm_sample_loop": lambda out: e.lib.ldm_sample_loop(e._h, out.data_ptr(), None, None, tm, tm, 2, C.byref(s), 1,
                                                                  0, B, None, 0, None)}
        for fn, call in calls.items():
            out = torch.full((B, S), -7, dtype=torch.int32, device=cuda)
            rc = call(out)
            torch.cuda.synchronize()
            assert rc != 0, (fn, text)
            assert text in e.lib.ldm_last_error(e._h).decode(), (fn, text, e.lib.ldm_last_error(e._h).decode())
            assert (out == -7).all(), (fn, text)
    with pytest.raises(RuntimeError, match="temperature must be > 0"):   # the Python layer surfaces the text
        e.sample_step(tin, 50, {"name": "random", "temperature": 0.0})


# ----------------------------------------------------------------------------- the temperature contract
def test_temperature_contract(cuda, golden_dir):  # noqa: F811
    """A dead class of a token carries exp(log(1e-30) / T) of the mass once the reference has divided by the temperature.
    Just inside C exp(log(1e-30) / T) <= 2^-24 (T = 3.18 for Rico25) the full-vocabulary form and both live-class forms
    draw the oracle's tokens (share <= 2e-3).  Well outside (T = 10: >= 0.35 % of the oracle's draws are dead classes,
    tests/test_post_token_scalar.py::test_live_class_form_needs_the_temperature_bound measures what a live-class form does
    there) ldm_sample_tokens still agrees with the oracle over all C classes, and ldm_sample_step / ldm_sample_loop
    REFUSE every stochastic sampler instead of approximating; deterministic decoding ignores the temperature."""
    spec, W = weights("rico25")
    states, _ = SC.load_states(golden_dir, "rico25")
    t_in = SC.admitted_temperature(spec.n_class)
    bad = {f: 0 for f in ("tokens", "exact", "fast")}
    bad_out = dead = total = 0
    for i, t, toks in states:
        logp = SC.oracle_logp(W, spec, toks, t)
        cfg = {"name": "random", "temperature": t_in}
        ref = SC.oracle_draw(logp, cfg, i)
        for f in bad:
            bad[f] += int((_draw(f, "rico25", logp, toks, t, cfg, i) != ref).sum())
        cfg = {"name": "random", "temperature": 10.0}
        ref = SC.oracle_draw(logp, cfg, i)
        bad_out += int((_draw("tokens", "rico25", logp, toks, t, cfg, i) != ref).sum())
        dead += int((logp.gather(1, ref[:, None, :]) == logp.min()).sum())
        total += ref.numel()
    print(f"[temperature contract] T={t_in:.4f}: mismatches {bad} of {total}; T=10 full vocabulary: {bad_out} of {total}, "
          f"oracle draws on dead classes {dead}")
    assert max(bad.values()) <= EDGE_BOUND * total, bad
    assert bad_out <= EDGE_BOUND * total and dead >= 0.002 * total
    tok = states[3][2].int()
    steps = R.timestep_list(spec.n_step, 4)
    for precision in ("exact", "fast"):
        e = engine("rico25", precision)
        for name in ("random", "top_p", "top_k", "gumbel"):
            cfg = {"name": name, "temperature": 1.001 * SC.max_live_temperature(spec.n_class), "top_p": 0.9, "top_k": 5}
            with pytest.raises(RuntimeError, match="temperature .* live classes only"):
                e.sample_step(tok, 59, cfg)
            with pytest.raises(RuntimeError, match="temperature .* live classes only"):
                e.sample_loop(tok.clone(), steps, steps, cfg, use_graph=False)
        det = e.sample_step(tok, 59, {"name": "deterministic", "temperature": 10.0}).cpu()
        assert torch.equal(det, e.sample_step(tok, 59, {"name": "deterministic"}).cpu())
