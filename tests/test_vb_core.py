"""Scoring given layouts — CPU side: the host build of csrc/ldm_vb_core.h (the arithmetic of kernels_vb.hip, through
tests/cpu_vb_check.cpp on the one-lane group) against what the reference's forward() recorded in tests/golden/vb/reference.npz
(tools/make_vb_golden.py).  Every case also runs in the ASan + UBSan build of the same stand-alone program.

Terms: from the reference's OWN log_x0_recon, x_0, x_t, t the per-token kl / decoder_nll / kl_aux equal the reference's within
4 x the reference's float32-vs-float64 distance of that term and (model, t) (_vb_cases.bar); kl >= -bar; with x_t == x_0 at
t = 1 the true posterior is a point mass and kl == nll within the bar.
Draws: the host core's tokens equal a numpy restatement (inverse CDF over the reference's exp(q_pred) rows on
R.token_uniforms uniforms) on every position of 5 layouts, four t, both constrained vocabularies and vanilla; a chi-square of
20 000 draws of one (class, t) against exp(q_pred) at the 1 - 1e-6 quantile (seeded: deterministic).  The reference's
schedule gives the beta-bar classes 1e-6 of the mass together, so the fixture's bins are {not [MASK], [MASK]}
(tools/make_vb_golden.py says why and checks the expected counts)."""
from statistics import NormalDist

import numpy as np
import pytest

import _hostbuild as HB
import _vb_cases as VC
from oracle import restatement as R
from oracle import spec as SP

SEED, FIRST = 20261019, 3


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    return HB.host_program("cpu_vb_check", sanitize=request.param == "sanitized")


def run(exe, tmp_path, mode, raw):
    rc, out = HB.run_host_io(exe, tmp_path, raw, mode)
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_terms_from_the_references_log_x0_recon(exe, tmp_path, ds, q_type):
    fx, spec = VC.fixture(), SP.SPECS[ds]
    b = int(fx["recon_layout"])
    x0 = fx[f"{VC.name(ds, q_type)}/x0"][b:b + 1]
    for t in fx[f"{VC.name(ds, q_type)}/ts"]:
        p = f"{VC.name(ds, q_type)}/t{int(t)}/"
        rows = fx[p + "recon"].T[None]                                     # (C,S) -> (1,S,C)
        err, tok, sums = VC.parse_terms(run(exe, tmp_path, "terms", VC.payload(ds, q_type, int(t), x0, fx[p + "xt"][b:b + 1], rows)), 1, spec.seq_len)
        assert err == 0
        for i, k in enumerate(VC.TERMS):
            ref, bar = fx[p + k][b], VC.bar(fx, p + k)
            worst = float(np.abs(tok[i, 0].astype(np.float64) - ref).max())
            print(f"[{ds}/{q_type} t={int(t)}] {k}: max |ours - reference| = {worst:.3e}, bar {bar:.3e}")
            assert worst <= bar, (k, int(t))
        # kl_aux reads log_x0_recon alone: the classes that are not x_0 weigh 1e-30 and vanish in float32 — the reference's bits
        assert np.array_equal(tok[2, 0].view(np.int32), fx[p + "aux"][b].view(np.int32))
        assert float(tok[0].min()) >= -VC.bar(fx, p + "kl")
        assert np.array_equal(tok[3, 0] != 0, fx[p + "recon"].argmax(0) == x0[0])
        for q in range(4):                                                  # float64, positions left to right
            acc = 0.0
            for s in range(spec.seq_len):
                acc += float(tok[q, 0, s])
            assert sums[0, q] == acc


@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_kl_equals_nll_where_the_true_posterior_is_a_point_mass(exe, tmp_path, ds, q_type):
    """x_t == x_0 at t = 1: q(x_0 | x_1 = x_0, x_0) is one class (every other carries <= 1e-30), so kl = -log p(x_0 | x_1) = nll
    whatever the model says — here the reference's log_x0_recon of t = 1."""
    fx, spec = VC.fixture(), SP.SPECS[ds]
    b, p = int(fx["recon_layout"]), f"{VC.name(ds, q_type)}/t1/"
    x0 = fx[f"{VC.name(ds, q_type)}/x0"][b:b + 1]
    _, tok, _ = VC.parse_terms(run(exe, tmp_path, "terms", VC.payload(ds, q_type, 1, x0, x0, fx[p + "recon"].T[None])), 1, spec.seq_len)
    worst = float(np.abs(tok[0].astype(np.float64) - tok[1]).max())
    print(f"[{ds}/{q_type}] max |kl - nll| = {worst:.3e}, bar {VC.bar(fx, p + 'kl'):.3e}")
    assert worst <= VC.bar(fx, p + "kl")
    # and the reference's own forced state (layout keep_x0) says the same
    k = int(fx["keep_x0"])
    assert float(np.abs(fx[p + "kl"][k].astype(np.float64) - fx[p + "nll"][k]).max()) <= VC.bar(fx, p + "kl")


@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_draws_equal_the_restatement_on_the_references_rows(exe, tmp_path, ds, q_type):
    fx, spec = VC.fixture(), SP.SPECS[ds]
    x0 = fx[f"{VC.name(ds, q_type)}/x0"][:5].astype(np.int32)
    for t in fx[f"{VC.name(ds, q_type)}/ts"]:
        err, got = VC.parse_draw(run(exe, tmp_path, "draw", VC.payload(ds, q_type, int(t), x0, seed=SEED, first_layout=FIRST)), 5, spec.seq_len)
        want = VC.draw_restatement(fx, ds, q_type, int(t), x0, SEED, FIRST)
        assert err == 0 and np.array_equal(got, want), (int(t), int((got != want).sum()))
        # cutting the batch changes nothing: layouts 2..4 alone, with their global index
        _, part = VC.parse_draw(run(exe, tmp_path, "draw", VC.payload(ds, q_type, int(t), x0[2:], seed=SEED, first_layout=FIRST + 2)), 3, spec.seq_len)
        assert np.array_equal(part, got[2:])
    assert (got != x0).any() and (got == spec.mask_id).any()


def test_draw_chi_square_against_exp_q_pred(exe, tmp_path):
    fx, spec = VC.fixture(), SP.RICO25
    t, attr, n = int(fx["chi2/t"]), int(fx["chi2/attr"]), int(fx["chi2/draws"])
    kept = VC.live_ids(spec, "constrained", attr)[int(fx["chi2/live_index"])]
    B = n // spec.max_elem
    assert B * spec.max_elem == n == 20000
    x0 = np.empty((B, spec.seq_len), np.int32)
    for a in range(spec.n_attr):
        x0[:, a::spec.n_attr] = VC.live_ids(spec, "constrained", a)[0]
    x0[:, attr::spec.n_attr] = kept
    _, xt = VC.parse_draw(run(exe, tmp_path, "draw", VC.payload("rico25", "constrained", t, x0, seed=SEED, first_layout=0)), B, spec.seq_len)
    draws = xt[:, attr::spec.n_attr].reshape(-1)
    # the row the fixture's bins came from is what this position has (three kinds of class)
    same, other, mask = fx["chi2/probs"].astype(np.float64)
    bins = np.array([same + other * (len(VC.live_ids(spec, "constrained", attr)) - 2), mask])
    assert np.allclose(bins / bins.sum(), fx["chi2/bins"], rtol=1e-6, atol=0) and (fx["chi2/bins"] * n >= 5).all()
    obs = np.array([(draws != spec.mask_id).sum(), (draws == spec.mask_id).sum()], np.float64)
    exp = fx["chi2/bins"] * n
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    thr = NormalDist().inv_cdf(1 - 0.5e-6) ** 2              # the 1 - 1e-6 quantile of chi-square with 1 degree of freedom: 23.93
    print(f"chi2 = {chi2:.3f} (threshold {thr:.2f}); observed {obs}, expected {exp}")
    assert chi2 <= thr
    assert set(np.unique(draws)) <= set(VC.live_ids(spec, "constrained", attr))


def test_host_core_refuses_bad_tokens(exe, tmp_path):
    spec = SP.RICO25
    x0 = VC.fixture()["rico25_constrained/x0"][:2].astype(np.int32)
    for bad, bit in ((spec.mask_id, 2), (spec.n_class, 1), (-1, 1), (spec.n_category, 4)):   # (a bin id at a category position)
        x = x0.copy()
        x[1, 5] = bad
        err, xt = VC.parse_draw(run(exe, tmp_path, "draw", VC.payload("rico25", "constrained", 3, x)), 2, spec.seq_len)
        assert err == bit and xt[1, 5] == spec.mask_id


@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_host_core_from_logits(exe, tmp_path, ds, q_type):
    """The whole per-token path — log-softmax (float64, and the fast mode's fp32 form), both posteriors, the sums — from the
    restatement's logits rounded to float32, all six layouts (all-[PAD], forced all-[MASK], forced x_t = x_0 among them),
    against the float64 restatement within the bar the GPU test gives the exact mode."""
    fx, spec = VC.fixture(), SP.SPECS[ds]
    t = spec.n_step // 3
    p = f"{VC.name(ds, q_type)}/t{t}/"
    x0, xt = fx[f"{VC.name(ds, q_type)}/x0"].astype(np.int64), fx[p + "xt"].astype(np.int64)
    want, amax, logits = VC.restated_fixture(ds, q_type, t)
    for lse in (1, 0):
        raw = run(exe, tmp_path, "logits", VC.payload(ds, q_type, t, x0, xt, logits.float().numpy(), lse=lse))
        err, tok, _ = VC.parse_terms(raw, len(x0), spec.seq_len)
        assert err == 0
        for i, k in enumerate(VC.TERMS):
            d = np.abs(tok[i].astype(np.float64) - want[i])
            print(f"[{ds}/{q_type} lse={'f64' if lse else 'f32'}] {k}: max |host core - restatement| = {d.max():.3e}")
            assert (d <= VC.restated_bars(fx, p + k, amax, 2e-5)).all(), (k, lse)


@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_float64_restatement_is_pinned_to_the_reference(ds, q_type):
    """The oracle of tests/test_vb_gpu.py — R.denoiser_logits in float64 -> R.predict_start_from_logits -> R.q_posterior -> the
    three sums — against the reference's recorded per-token terms: this is what pins that oracle to the reference and not to
    the kernels.  Bar: _vb_cases.bar, 4 x the reference's own float32-vs-float64 distance of the term and (model, t) — the bar
    the host core is held to above.  (Not 1 x: the restatement's logits are float64 where the reference's are float32, and
    several maxima sit an ulp above the distance itself.)  kl_aux has a recorded distance of exactly 0 and would fall to the
    fixture's zero floor (1e-2): it is held to decoder_nll's bar of the same (model, t) instead — both are -log_x0_recon[x_0]
    plus terms below 1e-26, read through the same float32 roundings.  Measured: kl <= 4.3e-6, nll <= 1.9e-6, aux <= 9.5e-7
    against bars of 5.7e-6 - 3.8e-5."""
    fx = VC.fixture()
    for t in fx[f"{VC.name(ds, q_type)}/ts"]:
        p = f"{VC.name(ds, q_type)}/t{int(t)}/"
        want, _, _ = VC.restated_fixture(ds, q_type, int(t))
        for i, k in enumerate(VC.TERMS):
            bar = VC.bar(fx, p + ("nll" if k == "aux" else k))
            d = np.abs(want[i] - fx[p + k].astype(np.float64))
            print(f"[{ds}/{q_type} t={int(t)}] restatement vs reference, {k}: max {d.max():.3e}, bar {bar:.3e} (recorded distance {float(fx[p + k + '_dist']):.3e})")
            assert d.max() <= bar, (k, int(t), float(d.max()), bar)


def test_draws_where_every_class_carries_mass(exe, tmp_path):
    """The reference's schedule leaves the beta-bar classes 1e-6 of the mass, so no draw above ever lands on an "other" class.
    Here the host core runs on a hand-made schedule row — alpha-bar 0.3, beta-bar 0.5 spread over the K - 1 non-[MASK] classes,
    gamma-bar 0.2 — and is compared, token for token, with a numpy inverse CDF over exp(q_pred) restated here (util.py:19-21 in
    float32), and by chi-square over ALL classes of one position's sub-vocabulary (20 000 draws, every expected count >= 5)."""
    spec, t, attr = SP.RICO25, 7, 2
    ids = VC.live_ids(spec, "constrained", attr)
    K = len(ids)
    f32 = np.float32
    la, lb, lc = f32(np.log(0.3)), f32(np.log(0.5 / (K - 1))), f32(np.log(0.2))
    l1c = f32(np.log(1 - np.exp(np.float64(lc)) + 1e-40))
    sched = VC.schedule_table("rico25", "constrained").copy()
    sched[3, :, t], sched[4, :, t], sched[5, :, t], sched[7, :, t] = la, lb, lc, l1c

    def lae(a, b):
        m = np.maximum(a, b)
        return (m + np.log(np.exp(a - m, dtype=f32) + np.exp(b - m, dtype=f32), dtype=f32)).astype(f32)

    eps = f32(np.log(f32(1e-30)))
    same, other, mask = (np.exp(lae(f32(0) + la, lb), dtype=f32), np.exp(lae(eps + la, lb), dtype=f32), np.exp(lae(eps + l1c, lc), dtype=f32))
    n = 20000
    B = n // spec.max_elem
    rng = np.random.default_rng(5)
    x0 = np.empty((B, spec.seq_len), np.int32)
    for a in range(spec.n_attr):
        x0[:, a::spec.n_attr] = VC.live_ids(spec, "constrained", a)[0]
    live0 = rng.integers(0, K - 1, (B, spec.max_elem))          # body classes and [PAD], never [MASK]
    live0[:, 0] = 9                                             # one fixed class: the chi-square's position
    x0[:, attr::spec.n_attr] = ids[live0]
    _, xt = VC.parse_draw(run(exe, tmp_path, "draw", VC.payload("rico25", "constrained", t, x0, seed=SEED, first_layout=FIRST, sched=sched)), B, spec.seq_len)
    got = xt[:, attr::spec.n_attr]
    u = R.token_uniforms(SEED, FIRST, B, spec.seq_len, t)[..., 0].astype(np.float64)[:, attr::spec.n_attr]
    want = np.empty_like(got)
    for b in range(B):
        for e in range(spec.max_elem):
            row = np.full(K, other, np.float64)
            row[live0[b, e]], row[-1] = same, mask
            cdf = np.cumsum(row)
            want[b, e] = ids[min(int((cdf <= u[b, e] * cdf[-1]).sum()), K - 1)]
    # a libm that rounds exp / log another way than numpy moves a bin edge by an ulp: a handful of 20 000 uniforms may sit there
    assert (got != want).sum() <= 2, int((got != want).sum())
    assert len(set(np.unique(got[:, 1:]))) == K                 # every class of the sub-vocabulary is drawn
    row = np.full(K, other, np.float64)
    row[9], row[-1] = same, mask
    exp = row / row.sum() * B
    obs = np.array([(got[:, 0] == c).sum() for c in ids], np.float64)
    # first: the 800 draws of the position whose x_0 is fixed, over all K classes (expected counts >= 12); second: all 20 000
    # draws, each re-indexed relative to its own kept class — kept / any other / [MASK]
    rel = np.where(got == spec.mask_id, K - 1, np.where(got == ids[live0], 0, 1))
    obs3 = np.array([(rel == 0).sum(), (rel == 1).sum(), (rel == K - 1).sum()], np.float64)
    exp3 = np.array([same, other * (K - 2), mask], np.float64)
    exp3 = exp3 / exp3.sum() * n
    assert (exp >= 5).all() and (exp3 >= 5).all()
    chi_k, chi_3 = float(((obs - exp) ** 2 / exp).sum()), float(((obs3 - exp3) ** 2 / exp3).sum())
    from scipy.stats import chi2 as chi2_dist
    thr_k, thr_3 = float(chi2_dist.isf(1e-6, K - 1)), float(chi2_dist.isf(1e-6, 2))
    print(f"chi2 over {K} classes (800 draws) = {chi_k:.2f} (threshold {thr_k:.2f}); over kept / other / [MASK] (20 000 draws) = {chi_3:.2f} ({thr_3:.2f})")
    assert chi_k <= thr_k and chi_3 <= thr_3
