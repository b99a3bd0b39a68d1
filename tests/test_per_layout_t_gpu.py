"""GPU: a timestep PER LAYOUT in one denoiser pass (ldm_denoise_logits_t / ldm_q_sample_t / ldm_vb_terms_t / ldm_vb_step_t) and
what diffusion.py builds on it (loss() in one call per window, elbo() on packed calls).

The expected value is always the existing single-t entry point run on the SAME full batch, with the layout's row taken from the
call at its t — the same row position on both sides — and the comparison is bit for bit: a pass depends on t through the AdaLN
parameters, the schedule rows and the Philox counter alone, and each takes the row's value in the arithmetic of the single-t
form (ln_rows: the same expression on per-row pointers; lngemm16x3_k: 1.0f + scale formed per lane as the staging loop forms it)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import _vb_cases as VC
from oracle import spec as SP
from oracle import synth
from test_hip_parity import WEIGHT_SEED
from test_hip_parity import engine as parity_engine
from test_vb_gpu import bits, diffusion, engine_of, state_dict

pytestmark = pytest.mark.gpu

SEED, FIRST = 20261020, 3
SMALL = dataclasses.replace(SP.RICO25, name="small", d_model=256, n_head=4, d_ff=1024, n_layer=2, n_step=20)


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


def make_engine(spec, precision, max_batch, chunk=0, q_type="constrained", seed=WEIGHT_SEED):
    from layout_dm_amd.binding import Engine

    e = Engine(n_category=spec.n_category, n_bin=spec.n_bin, max_elem=spec.max_elem, d_model=spec.d_model, n_head=spec.n_head,
               d_ff=spec.d_ff, n_layer=spec.n_layer, n_step=spec.n_step, precision=precision, max_batch=max_batch, chunk=chunk,
               q_type=q_type)
    e.load_state_dict(synth.synth_state_dict(spec, seed=seed, perturb=True, q_type=q_type))
    return e


def valid_x0(spec, B, seed):
    """(B,S) int32 tokens of their positions' sub-vocabularies (body or [PAD]; never [MASK])"""
    rng = np.random.default_rng(seed)
    out = np.empty((B, spec.seq_len), np.int32)
    for s in range(spec.seq_len):
        ids = VC.live_ids(spec, "constrained", s % spec.n_attr)[:-1]
        out[:, s] = rng.choice(ids, size=B)
    return out


def rows_equal_the_single_t_calls(e, tokens, t, rows=None):
    """denoise_logits_t(tokens, t)[b] against denoise_logits(tokens, t[b])[b], bit for bit, for b in rows (default: all)"""
    got = e.denoise_logits_t(tokens, t)
    assert got.shape == (tokens.shape[0], e.S, e.C) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    for tv in sorted(set(t)):
        ref = e.denoise_logits(tokens, tv)
        for b in (b for b in range(len(t)) if t[b] == tv and (rows is None or b in rows)):
            assert torch.equal(bits(got[b]), bits(ref[b])), (b, tv, float((got[b] - ref[b]).abs().max()))
    return got


# ----------------------------------------------------------------------------- 1. logits, bit for bit
@pytest.mark.parametrize("precision", ["exact", "split", "mixed", "hybrid", "fast_small"])
def test_logits_rows_have_the_bits_of_the_single_t_call(cuda, precision):
    """Rico25, S = 125, B = 5, t = [0, 99, 1, 50, 50]: every 128-row block holds two or three layouts at different t and both
    ends of the AdaLN table are read.  fast_small: the fast engine on a backbone the stack kernel does not serve (the tiled path)."""
    if precision == "fast_small":
        spec, t = SMALL, [0, 19, 1, 10, 10]
        e = make_engine(spec, "fast", 8)
    else:
        spec, t = SP.RICO25, [0, 99, 1, 50, 50]
        e = parity_engine("rico25", precision)
    assert e.per_layout_t and e.describe()["per_layout_t"] == "1"
    print(f"[{precision}] kernels: {e.describe()['kernels']}")
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, spec.n_class, (5, spec.seq_len), generator=g).int().to(cuda)
    got = rows_equal_the_single_t_calls(e, tokens, t)
    assert not torch.equal(got[3], e.denoise_logits(tokens, t[0])[3])          # (t does matter)
    # all t equal: the whole tensor has the bits of the single-t call
    for tv in (t[1], t[3]):
        assert torch.equal(bits(e.denoise_logits_t(tokens, [tv] * 5)), bits(e.denoise_logits(tokens, tv)))
    if precision == "fast_small":
        e.close()


# ----------------------------------------------------------------------------- 2. short rows
@pytest.mark.parametrize("precision", ["exact", "split"])
def test_short_rows_six_layouts_per_block(cuda, precision):
    """max_elem = 5 (S = 25), B = 12 at twelve different t: five or six layouts share one 128-row block."""
    spec = dataclasses.replace(SP.RICO25, name="short5", max_elem=5)
    e = make_engine(spec, precision, 12)
    kern = e.describe()["kernels"]
    print(f"[{precision}] S = {spec.seq_len}: kernels = {kern} ({'row-resident' if 'row_resident' in kern else 'tiled'} form ran)")
    t = [0, 99, 1, 50, 7, 33, 98, 2, 64, 12, 81, 25]
    g = torch.Generator().manual_seed(6)
    tokens = torch.randint(0, spec.n_class, (12, spec.seq_len), generator=g).int().to(cuda)
    rows_equal_the_single_t_calls(e, tokens, t)
    e.close()


# ----------------------------------------------------------------------------- 3. chunk boundary
def test_rows_on_both_sides_of_a_chunk_boundary(cuda):
    e = parity_engine("rico25", "split", max_batch=8, chunk=4)
    chunk = e.chunk                                                        # (ldm_get_layout)
    assert chunk == 4 and "row_resident_ln_gemm" in e.describe()["kernels"]
    B = chunk + 3
    t = [3 if b % 2 == 0 else 77 for b in range(B)]
    g = torch.Generator().manual_seed(7)
    tokens = torch.randint(0, SP.RICO25.n_class, (B, SP.RICO25.seq_len), generator=g).int().to(cuda)
    rows_equal_the_single_t_calls(e, tokens, t, rows=(chunk - 1, chunk, chunk + 2))
    # the bound's terms across the boundary: the second chunk reads ITS layouts' timesteps and layout indices
    x0 = torch.from_numpy(np.concatenate([VC.fixture()["rico25_constrained/x0"], VC.fixture()["rico25_constrained/x0"][:1]]).astype(np.int32)).to(cuda)
    got = e.vb_step_t(x0, t, seed=SEED, first_layout=FIRST)
    for tv in (3, 77):
        ref = e.vb_step(x0, tv, seed=SEED, first_layout=FIRST)
        for b in (b for b in (chunk - 1, chunk, chunk + 2) if t[b] == tv):
            assert torch.equal(bits(got[b]), bits(ref[b])), (b, tv)


# ----------------------------------------------------------------------------- 4. q_sample_t / vb_terms_t / vb_step_t
@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_noising_and_terms_at_per_layout_t(cuda, ds, q_type):
    fx = VC.fixture()
    e = engine_of(ds, q_type, "exact")
    p = f"{VC.name(ds, q_type)}/mixed/"
    x0 = torch.from_numpy(fx[f"{VC.name(ds, q_type)}/x0"].astype(np.int32)).to(cuda)
    xt = torch.from_numpy(fx[p + "xt"].astype(np.int32)).to(cuda)
    t = [int(v) for v in fx["t_mixed"]]
    B = len(t)
    perm = [4, 0, 5, 2, 1, 3]
    drawn = e.q_sample_t(x0, t, SEED, FIRST)
    permuted = e.q_sample_t(x0[perm], [t[i] for i in perm], SEED, FIRST, layout=perm)
    logits = e.denoise_logits_t(xt, t)
    sums, tok = e.vb_terms_t(logits, x0, xt, t, per_token=True)
    step_given = e.vb_step_t(x0, t, xt=xt)
    step_drawn = e.vb_step_t(x0, t, seed=SEED, first_layout=FIRST)
    step_perm = e.vb_step_t(x0[perm], [t[i] for i in perm], seed=SEED, first_layout=FIRST, layout=perm)
    assert drawn.dtype == torch.int32 and sums.dtype == torch.float64 and sums.shape == (B, 4) and tok.shape == (3, B, e.S)
    for b in range(B):
        want = e.q_sample(x0, t[b], SEED, FIRST)
        assert torch.equal(drawn[b], want[b]) and torch.equal(permuted[perm.index(b)], want[b]), b
        ref_sums, ref_tok = e.vb_terms(e.denoise_logits(xt, t[b]), x0, xt, t[b], per_token=True)
        assert torch.equal(bits(sums[b]), bits(ref_sums[b])) and torch.equal(bits(tok[:, b]), bits(ref_tok[:, b])), b
        assert torch.equal(bits(step_given[b]), bits(e.vb_step(x0, t[b], xt=xt)[b])), b
        ref_drawn = e.vb_step(x0, t[b], seed=SEED, first_layout=FIRST)[b]
        assert torch.equal(bits(step_drawn[b]), bits(ref_drawn)) and torch.equal(bits(step_perm[perm.index(b)]), bits(ref_drawn)), b
    assert torch.equal(bits(step_given), bits(sums))
    assert not torch.equal(drawn, x0)


def test_wide_vocabulary_at_per_layout_t(cuda):
    """64 bins (283 classes), exact, B = 3: the 576-class instantiations of vb_terms_k"""
    spec = dataclasses.replace(SP.RICO25, name="rico25_64", n_bin=64)
    e = make_engine(spec, "exact", 3)
    x0 = torch.from_numpy(valid_x0(spec, 3, 8)).to(cuda)
    t = [0, 57, 99]
    drawn, step = e.q_sample_t(x0, t, SEED, FIRST), e.vb_step_t(x0, t, seed=SEED, first_layout=FIRST)
    for b in range(3):
        assert torch.equal(drawn[b], e.q_sample(x0, t[b], SEED, FIRST)[b]), b
        assert torch.equal(bits(step[b]), bits(e.vb_step(x0, t[b], seed=SEED, first_layout=FIRST)[b])), b
    assert bool(torch.isfinite(step).all()) and bool((step[:, :3] >= 0).all())
    e.close()


# ----------------------------------------------------------------------------- 5. loss() and elbo()
def count_calls(engine):
    calls = {"vb_step": 0, "vb_step_t": 0, "q_sample": 0}
    for name in calls:
        inner = getattr(engine, name)

        def spy(*a, _inner=inner, _name=name, **k):
            calls[_name] += 1
            return _inner(*a, **k)
        setattr(engine, name, spy)
    return calls


@functools.lru_cache(maxsize=None)
def split_diffusion():
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    d = HipMaskAndReplaceDiffusion(n_category=SP.RICO25.n_category, precision="split", max_batch=8)
    d.load_state_dict(state_dict("rico25", "constrained"))
    return d


@pytest.mark.parametrize("precision", ["exact", "split"])
def test_loss_in_one_call_equals_the_grouped_loss(cuda, precision):
    fx = VC.fixture()
    d = diffusion("rico25", "constrained") if precision == "exact" else split_diffusion()
    p = "rico25_constrained/mixed/"
    x0 = torch.from_numpy(fx["rico25_constrained/x0"].astype(np.int64))
    xt = torch.from_numpy(fx[p + "xt"].astype(np.int64))
    t, pt = torch.from_numpy(fx["t_mixed"].astype(np.int64)), torch.from_numpy(fx[p + "pt"])
    calls = count_calls(d.engine)
    try:
        one = d.loss(x0, t=t, pt=pt, x_t=xt)
        assert calls == {"vb_step": 0, "vb_step_t": 1, "q_sample": 0}
        grouped = d.loss(x0, t=t, pt=pt, x_t=xt, grouped=True)
        assert calls["vb_step"] == len(set(t.tolist())) and calls["vb_step_t"] == 1
        one_drawn = d.loss(x0, t=t, pt=pt, seed=5, first_layout=10)
        grouped_drawn = d.loss(x0, t=t, pt=pt, seed=5, first_layout=10, grouped=True)
    finally:
        for name in calls:
            delattr(d.engine, name)
    for a, b in ((one, grouped), (one_drawn, grouped_drawn)):
        assert set(a) == set(b) == {"kl_loss", "aux_loss"}
        for k in a:
            print(f"[{precision}] {k}: one call {float(a[k])!r}, grouped {float(b[k])!r}")
            assert torch.equal(bits(a[k].reshape(1)), bits(b[k].reshape(1))), k
    assert float(one["kl_loss"]) != float(one_drawn["kl_loss"])


def test_elbo_on_packed_calls_is_the_sum_of_the_vb_terms_calls(cuda):
    """B = 4, max_batch = 8, T = 20 (the small backbone of tests/test_vb_gpu.py): 10 calls of two timesteps each where 20 stood."""
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    d = HipMaskAndReplaceDiffusion(n_category=SMALL.n_category, d_model=SMALL.d_model, n_head=SMALL.n_head, d_ff=SMALL.d_ff,
                                   n_layer=SMALL.n_layer, num_timesteps=SMALL.n_step, precision="exact", max_batch=8)
    d.load_state_dict(synth.synth_state_dict(SMALL, seed=WEIGHT_SEED, perturb=True))
    x0 = torch.from_numpy(VC.fixture()["rico25_constrained/x0"][:4].astype(np.int64))
    total = None
    for t in range(SMALL.n_step):
        terms = d.vb_terms(x0, t, seed=11, first_layout=2)
        term = terms["decoder_nll"] if t == 0 else terms["kl"]
        total = term if total is None else total + term
    calls = count_calls(d.engine)
    got = d.elbo(x0, seed=11, first_layout=2)
    assert calls == {"vb_step": 0, "vb_step_t": 10, "q_sample": 0}
    assert torch.equal(bits(got), bits(total))
    two = d.elbo(x0, n_draws=2, seed=11, first_layout=2)                      # draws 11 and 12, averaged
    other = d.elbo(x0, seed=12, first_layout=2)
    # (one accumulator runs through both draws' terms: the same 40 positive float64 terms in another order — 40 roundings at most)
    assert torch.allclose(two, (got + other) / 2, rtol=40 * 2.0 ** -52, atol=0) and calls["vb_step_t"] == 40
    d.close()


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals(cuda):
    fx, spec = VC.fixture(), SP.RICO25
    e = engine_of("rico25", "constrained", "exact")
    x0 = torch.from_numpy(fx["rico25_constrained/x0"][:3].astype(np.int32)).to(cuda)
    xt = torch.from_numpy(fx["rico25_constrained/t33/xt"][:3].astype(np.int32)).to(cuda)
    logits = e.denoise_logits(xt, 33)
    good = e.vb_step_t(x0, [33, 1, 0], xt=xt)
    for bad in (-1, spec.n_step):
        t = [33, bad, 0]
        for call in (lambda: e.denoise_logits_t(xt, t), lambda: e.q_sample_t(x0, t), lambda: e.vb_terms_t(logits, x0, xt, t),
                     lambda: e.vb_step_t(x0, t, xt=xt)):
            with pytest.raises(RuntimeError, match=rf"timestep {bad} of layout 1 out of range"):
                call()
    with pytest.raises(ValueError, match="3 timesteps"):
        e.vb_step_t(x0, [1, 2])
    x = x0.clone()
    x[2, 7] = spec.mask_id                                                 # the token checks of the single-t calls
    with pytest.raises(ValueError, match=r"\[MASK\]"):
        e.vb_step_t(x, [33, 1, 0])
    assert torch.equal(bits(e.vb_step_t(x0, [33, 1, 0], xt=xt)), bits(good))   # and the next call is clean


def test_an_engine_without_the_per_layout_form_refuses_and_loss_groups(cuda):
    """fast on the reference's backbone (the stack kernel): rc -4 from the C calls; loss() takes the grouped path by itself"""
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    fx = VC.fixture()
    d = HipMaskAndReplaceDiffusion(n_category=SP.RICO25.n_category, precision="fast", max_batch=8)
    d.load_state_dict(state_dict("rico25", "constrained"))
    e = d.engine
    assert e.describe()["kernels"] == "stack" and e.describe()["per_layout_t"] == "0" and not e.per_layout_t
    x0 = torch.from_numpy(fx["rico25_constrained/x0"].astype(np.int64))
    t = [int(v) for v in fx["t_mixed"]]
    for call in (lambda: e.denoise_logits_t(x0.int().to(cuda), t), lambda: e.vb_step_t(x0.int().to(cuda), t)):
        with pytest.raises(RuntimeError, match=r"\(-4\).*fast_f16"):
            call()
    calls = count_calls(e)
    got = d.loss(x0, t=torch.tensor(t), pt=torch.from_numpy(fx["rico25_constrained/mixed/pt"]), seed=5)
    assert calls["vb_step_t"] == 0 and calls["vb_step"] == len(set(t)) and np.isfinite(float(got["kl_loss"]))
    d.close()
