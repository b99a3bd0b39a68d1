"""GPU: the cond=refinement prior built on the device (ldm_refinement_prior, kernels_refine.hip).

  * the kernel against torch indexing on the CPU — `(table[seq].permute(0, 2, 1) * w)` — BIT FOR BIT (compared as int32: the
    sign of zero counts) on random tables with negative entries, C x S x B over every tile edge of the kernel (one float, fewer
    floats than a 16-byte group, slabs of odd length so that layouts start at every misalignment, several chunks per
    layout, more than one workgroup wave), the (1,S) -> B broadcast, int32 / int64 ids, a non-default stream, ids 0 and C - 1,
    and a sequence beyond the LDS staging limit;
  * guard bands: the output an interior slice of a sentinel-filled buffer at every 4-byte misalignment, untouched around it,
    also at B = 257 and with an out-of-range id;
  * ids -1 and C raise IndexError, B = 0 gives an empty tensor;
  * the product path on a small model (exact engine, 2 layers, T = 20, max_batch = 4) with layoutdm.refinement_weak_logits
    patched to raise: LayoutDM.sample(cond=refinement) runs and its tokens equal those of the same call handed the host-built
    weak_logits — greedy and seeded top-p, (1,S) cond -> 5 samples, 6 samples cut at max_batch, sample_from_layouts.

Every test here needs the export, which the parent commit does not have."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import spec as SP
from oracle import synth

from _stub_tokenizer import StubTokenizer  # noqa: E402

pytestmark = pytest.mark.gpu

CS = (1, 7, 64, 65, 135, 155, 192)
SS = (1, 4, 63, 64, 65, 125, 128, 150)
WEIGHTS = (3.0, -3.0, 0.1, -0.75)


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def case(Cn, S, B_seq, seed, dtype=torch.int64):
    """(table with negative entries and exact zeros, ids with 0 and C - 1 present)"""
    g = torch.Generator().manual_seed(seed)
    table = torch.randn((Cn, Cn), generator=g)
    table[torch.rand((Cn, Cn), generator=g) < 0.25] = 0.0
    seq = torch.randint(0, Cn, (B_seq, S), generator=g)
    seq[0, 0], seq[-1, -1] = 0, Cn - 1
    return table, seq.to(dtype)


def reference(table, seq, w, B):
    """refinement_weak_logits' expression on the CPU (+ duplicate_cond's repeat for a single conditioning layout)"""
    out = (table[seq.long()].permute(0, 2, 1) * w).contiguous()
    return out.repeat(B, 1, 1) if seq.shape[0] == 1 and B > 1 else out


@pytest.mark.parametrize("B", [1, 3, 257])
def test_kernel_equals_torch_indexing_bit_for_bit(cuda, B):
    from layout_dm_amd.binding import refinement_prior

    n = 0
    for Cn in CS:
        for S in SS:
            dt = torch.int32 if n % 2 else torch.int64
            w = WEIGHTS[n % len(WEIGHTS)]
            table, seq = case(Cn, S, B, seed=1000 * Cn + S, dtype=dt)
            # ids handed over on the device and (every third case) from the host
            got = refinement_prior(seq if n % 3 == 0 else seq.to(cuda), table.to(cuda), w, B)
            assert got.shape == (B, Cn, S) and got.dtype == torch.float32 and got.device == cuda and got.is_contiguous()
            want = reference(table, seq, w, B)
            assert torch.equal(bits(got), bits(want)), (Cn, S, B, dt, w)
            if w < 0 and Cn > 1:
                assert bool((torch.signbit(want) & (want == 0)).any())      # -0.0 is in play
            n += 1
    assert n == 56


def test_broadcast_int32_int64_and_a_side_stream(cuda):
    from layout_dm_amd.binding import refinement_prior

    side = torch.cuda.Stream(device=cuda)
    for Cn, S in ((155, 125), (135, 125), (7, 63), (1, 1), (192, 150)):
        for dt in (torch.int32, torch.int64):
            table, seq = case(Cn, S, 1, seed=Cn + S, dtype=dt)
            want = reference(table, seq, -3.0, 5)
            got = refinement_prior(seq.to(cuda), table.to(cuda), -3.0, 5)
            assert got.shape == (5, Cn, S) and torch.equal(bits(got), bits(want)), (Cn, S, dt)
            tab_d, seq_d = table.to(cuda), seq.to(cuda)
            torch.cuda.synchronize(cuda)
            with torch.cuda.stream(side):
                got = refinement_prior(seq_d, tab_d, -3.0, 5)
            side.synchronize()
            assert torch.equal(bits(got), bits(want)), (Cn, S, dt, "side stream")
    # other integer dtypes are taken as ids too
    table, seq = case(65, 64, 3, seed=9)
    assert torch.equal(bits(refinement_prior(seq.to(torch.int16), table.to(cuda), 0.1, 3)), bits(reference(table, seq, 0.1, 3)))


def test_sequence_beyond_the_staging_limit(cuda):
    """S > 1024 ids are read in place instead of from LDS: same result, same error report"""
    from layout_dm_amd.binding import refinement_prior

    for Cn, S, B in ((3, 1030, 2), (5, 4099, 3), (2, 1025, 1)):
        table, seq = case(Cn, S, B, seed=S)
        assert torch.equal(bits(refinement_prior(seq.to(cuda), table.to(cuda), -0.75, B)), bits(reference(table, seq, -0.75, B)))
        seq[B - 1, S - 1] = Cn
        with pytest.raises(IndexError):
            refinement_prior(seq.to(cuda), table.to(cuda), -0.75, B)


SENTINEL = -12345.625


@pytest.mark.parametrize("Cn,S,B,bad", [(155, 125, 3, None), (7, 63, 4, None), (1, 1, 2, None), (1, 3, 5, None), (65, 150, 2, None),
                                        (155, 125, 257, None), (135, 125, 257, 135), (155, 125, 3, -1)])
def test_guard_bands_around_an_interior_slice(cuda, Cn, S, B, bad):
    from layout_dm_amd.binding import refinement_prior

    table, seq = case(Cn, S, B, seed=77)
    want = reference(table, seq, 3.0, B)
    if bad is not None:
        seq[B - 1, S - 1] = bad
        seq[0, 0] = bad
    n = B * Cn * S
    tab_d, seq_d = table.to(cuda), seq.to(cuda)
    for lead in (64, 61, 62, 63):         # every misalignment of the output against 16 bytes
        buf = torch.full((lead + n + 64,), SENTINEL, dtype=torch.float32, device=cuda)
        out = buf[lead:lead + n].view(B, Cn, S)
        assert out.data_ptr() % 16 == 4 * (lead % 4)
        if bad is None:
            assert refinement_prior(seq_d, tab_d, 3.0, B, out=out) is out
        else:
            with pytest.raises(IndexError):
                refinement_prior(seq_d, tab_d, 3.0, B, out=out)
        host = buf.cpu()
        assert bool((host[:lead] == SENTINEL).all()) and bool((host[lead + n:] == SENTINEL).all()), (lead, "guard band touched")
        got = host[lead:lead + n].view(B, Cn, S)
        assert not bool((got == SENTINEL).any()), (lead, "a float was not written")
        if bad is None:
            assert torch.equal(bits(got), bits(want)), lead
        else:   # the bad ids' columns are +0.0, everything else is the prior
            w = want.clone()
            w[B - 1, :, S - 1] = 0.0
            w[0, :, 0] = 0.0
            assert torch.equal(bits(got), bits(w)), lead


def test_error_path_and_empty_batch(cuda):
    from layout_dm_amd.binding import refinement_prior

    table, seq = case(155, 125, 4, seed=3)
    tab_d = table.to(cuda)
    for bad in (-1, 155):
        for dt in (torch.int32, torch.int64):
            for where in ((0, 0), (3, 124), (2, 60)):
                s = seq.to(dt).clone()
                s[where] = bad
                with pytest.raises(IndexError, match="outside"):
                    refinement_prior(s.to(cuda), tab_d, 3.0, 4)
    s = seq[:1].clone()
    s[0, 17] = 155
    with pytest.raises(IndexError):
        refinement_prior(s, tab_d, 3.0, 5)                 # the broadcast form reports it too
    assert torch.equal(bits(refinement_prior(seq.to(cuda), tab_d, 3.0, 4)), bits(reference(table, seq, 3.0, 4)))   # and the next call is clean
    for empty in (seq[:0], seq[:1]):
        out = refinement_prior(empty.to(cuda), tab_d, 3.0, 0)
        assert out.shape == (0, 155, 125) and out.dtype == torch.float32 and out.device == cuda
    with pytest.raises(ValueError):
        refinement_prior(seq[:2].to(cuda), tab_d, 3.0, 4)   # neither B nor 1 rows
    with pytest.raises(ValueError):
        refinement_prior(seq.to(cuda), tab_d[:, :100], 3.0, 4)


def test_weak_logits_device_equals_the_host_function_and_caches_its_table(cuda):
    from layout_dm_amd.layoutdm import refinement_weak_logits, refinement_weak_logits_device

    for spec in (SP.RICO25, SP.PUBLAYNET):
        tok = StubTokenizer(spec)
        g = torch.Generator().manual_seed(spec.n_category)
        seq = torch.randint(0, spec.n_class, (3, spec.seq_len), generator=g)
        cache = {}
        for mode in ("uniform", "negative", "gaussian"):
            for lam in (3.0, 0.1, -3.0):
                cfg = {"refine_mode": mode, "refine_offset_ratio": 0.1, "refine_lambda": lam}
                want = refinement_weak_logits(tok, seq, cfg, {})
                for s in (seq, seq.to(cuda), seq.int().to(cuda)):
                    got = refinement_weak_logits_device(tok, s, cfg, 3, cache)
                    assert got.device == cuda and torch.equal(bits(got), bits(want)), (spec.name, mode, lam)
                one = refinement_weak_logits_device(tok, seq[1:2].to(cuda), cfg, 4, cache)
                assert torch.equal(bits(one), bits(want[1:2].repeat(4, 1, 1)))
            key = ("device", mode, 0.1, str(cuda))
            assert key in cache and cache[key].device == cuda
            kept = cache[key]
            refinement_weak_logits_device(tok, seq, {"refine_mode": mode, "refine_offset_ratio": 0.1}, 3, cache)
            assert cache[key] is kept                                  # one upload per (mode, ratio, device)


# ---- the product path ----------------------------------------------------------------------------------------------------
SMALL = dataclasses.replace(SP.RICO25, name="small", n_layer=2, n_step=20)
BACKBONE_CFG = {"_target_": "trainer.models.transformer_utils.TransformerEncoder",
                "encoder_layer": {"_target_": "trainer.models.transformer_utils.Block", "d_model": 512, "nhead": 8,
                                  "dim_feedforward": 2048, "dropout": 0.0, "batch_first": True, "norm_first": True,
                                  "timestep_type": "adalayernorm", "diffusion_step": 20},
                "num_layers": 2}
E = SMALL.max_elem


def cfg_of(name, **kw):
    cfg = {"name": name, "temperature": 1.0, "num_timesteps": 20, "refine_mode": "uniform", "refine_offset_ratio": 0.1,
           "refine_lambda": 3.0}
    cfg.update(kw)
    return cfg


def synth_layouts(B, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(1, E + 1, (B,), generator=g)
    mask = torch.arange(E)[None] < n[:, None]
    wh = 0.05 + 0.4 * torch.rand((B, E, 2), generator=g)
    xy = wh / 2 + (1 - wh) * torch.rand((B, E, 2), generator=g)
    return {"bbox": torch.cat([xy, wh], dim=-1) * mask[..., None], "label": torch.randint(0, SMALL.n_category, (B, E), generator=g) * mask,
            "mask": mask}


@pytest.fixture(scope="module")
def small(cuda):
    from layout_dm_amd import layoutdm

    host_prior = layoutdm.refinement_weak_logits        # the parent's product path, kept for the answer key
    tok = StubTokenizer(SMALL)
    m = layoutdm.LayoutDM(backbone_cfg=BACKBONE_CFG, tokenizer=tok, num_timesteps=20, q_type="constrained", max_batch=4,
                          precision="exact").to("cuda")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(SMALL, seed=1, perturb=True).items()})
    return m.eval(), tok, host_prior


@pytest.fixture()
def no_host_prior(monkeypatch):
    from layout_dm_amd import layoutdm

    def refuse(*_a, **_k):
        raise AssertionError("the host-side prior was called on the sampling path")

    monkeypatch.setattr(layoutdm, "refinement_weak_logits", refuse)


def conds(tok, B, seed, dev=None):
    from layout_dm_amd import task

    cond = task.get_cond(synth_layouts(B, seed), tok, "refinement", seed=seed)
    assert cond["type"] == "refinement" and "weak_logits" not in cond and cond["seq_orig"].shape == (B, SMALL.seq_len)
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) and dev is not None else v) for k, v in cond.items()}


@pytest.mark.parametrize("where", ["host", "device"])
def test_sample_runs_without_the_host_prior_and_gives_the_same_tokens(cuda, small, no_host_prior, where):
    m, tok, host_prior = small
    cond = conds(tok, 4, seed=5, dev=cuda if where == "device" else "cpu")
    for cfg, kw in ((cfg_of("deterministic"), {}), (cfg_of("top_p", top_p=0.9), {"seed": 11}),
                    (cfg_of("deterministic", refine_mode="negative"), {}), (cfg_of("top_p", top_p=0.9, refine_mode="gaussian"), {"seed": 12})):
        with_host = dict(cond, weak_logits=host_prior(tok, cond["seq_orig"], cfg, {}))
        want = m.model.sample(batch_size=4, cond=with_host, sampling_cfg=cfg, **kw)
        got = m.model.sample(batch_size=4, cond=cond, sampling_cfg=cfg, **kw)
        assert got.shape == (4, SMALL.seq_len) and torch.equal(got, want), (where, cfg["name"], cfg["refine_mode"])
        assert "weak_logits" not in cond                                   # the caller's dict is left alone
    # the prior matters on this model: without it the tokens differ (so equality above is not vacuous)
    cfg = cfg_of("deterministic")
    flat = dict(cond, weak_logits=torch.zeros((4, SMALL.n_class, SMALL.seq_len)))
    assert not torch.equal(m.model.sample(batch_size=4, cond=flat, sampling_cfg=cfg), m.model.sample(batch_size=4, cond=cond, sampling_cfg=cfg))


def test_single_conditioning_layout_and_batches_beyond_max_batch(cuda, small, no_host_prior):
    m, tok, host_prior = small
    for cfg, kw in ((cfg_of("deterministic"), {}), (cfg_of("top_p", top_p=0.9), {"seed": 21})):
        one = conds(tok, 1, seed=8)
        want = m.model.sample(batch_size=5, cond=dict(one, weak_logits=host_prior(tok, one["seq_orig"], cfg, {})), sampling_cfg=cfg, **kw)
        got = m.model.sample(batch_size=5, cond=one, sampling_cfg=cfg, **kw)
        assert got.shape == (5, SMALL.seq_len) and torch.equal(got, want), cfg["name"]
        six = conds(tok, 6, seed=9)
        want = m.model.sample(batch_size=6, cond=dict(six, weak_logits=host_prior(tok, six["seq_orig"], cfg, {})), sampling_cfg=cfg, **kw)
        got = m.model.sample(batch_size=6, cond=six, sampling_cfg=cfg, **kw)
        assert got.shape == (6, SMALL.seq_len) and torch.equal(got, want), cfg["name"]
    # a caller-supplied prior is used untouched
    six = conds(tok, 6, seed=9)
    mine = torch.zeros((6, SMALL.n_class, SMALL.seq_len))
    a = m.model.sample(batch_size=6, cond=dict(six, weak_logits=mine), sampling_cfg=cfg_of("deterministic"))
    b = m.model.sample(batch_size=6, cond=dict(six, weak_logits=mine.to(cuda)), sampling_cfg=cfg_of("deterministic"))
    assert torch.equal(a, b)
    # an id of seq_orig outside the vocabulary raises like the indexing did
    bad = conds(tok, 2, seed=3)
    bad["seq_orig"] = bad["seq_orig"].clone()
    bad["seq_orig"][1, 4] = SMALL.n_class
    with pytest.raises(IndexError):
        m.model.sample(batch_size=2, cond=bad, sampling_cfg=cfg_of("deterministic"))


def test_sample_from_layouts_refinement(cuda, small, no_host_prior):
    from layout_dm_amd import task

    m, tok, host_prior = small
    lay = synth_layouts(6, seed=13)
    for cfg, kw in ((cfg_of("deterministic"), {}), (cfg_of("top_p", top_p=0.9), {"seed": 4})):
        cond = task.get_cond({k: v.to(cuda) for k, v in lay.items()}, tok, "refinement", seed=21)
        assert cond["seq_orig"].is_cuda
        want = m.sample(batch_size=6, cond=dict(cond, weak_logits=host_prior(tok, cond["seq_orig"], cfg, {})), sampling_cfg=cfg, **kw)
        got = m.sample_from_layouts(lay, "refinement", cfg, cond_seed=21, **kw)
        for k in ("bbox", "label", "mask"):
            assert torch.equal(got[k], want[k]), (cfg["name"], k)
        assert torch.equal(got["mask"], lay["mask"]) and torch.equal(got["label"][got["mask"]], lay["label"][lay["mask"]])
