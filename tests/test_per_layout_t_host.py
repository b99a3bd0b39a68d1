"""Per-layout timesteps — CPU side.

* elbo_calls (layout_dm_amd/diffusion.py): the packing of the (draw, t, layout) triples of elbo() into engine calls.
* HipMaskAndReplaceDiffusion.loss() / elbo() over a stand-in engine (in the manner of tests/test_verified_logic.py): which engine
  calls they make — the counted criterion of the feature — and that rows, timesteps, layout indices and seeds reach them.
* The host build of csrc/ldm_vb_core.h with a timestep and a layout index per row (tests/cpu_vb_t_check.cpp: row_t / row_layout,
  what kernels_vb.hip does for the ldm_*_t entry points) against the single-t build (tests/cpu_vb_check.cpp) run at that row's
  t, row by row and bit for bit; also in the ASan + UBSan build."""
import math

import numpy as np
import pytest
import torch

import _hostbuild as HB
import _vb_cases as VC
from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion, elbo_calls
from oracle import spec as SP

SEED, FIRST = 20261020, 7


# ----------------------------------------------------------------------------- the packing
@pytest.mark.parametrize("B,T,n_draws,max_rows", [(4, 20, 1, 8), (3, 20, 2, 8), (8, 20, 1, 8), (5, 7, 1, 512)])
def test_elbo_calls_cover_every_triple_once(B, T, n_draws, max_rows):
    calls = elbo_calls(B, T, n_draws, max_rows)
    seen = []
    for c in calls:
        assert 1 <= len(c.t) == len(c.layout) <= max_rows
        assert isinstance(c.draw, int) and 0 <= c.draw < n_draws           # one draw — one Philox seed — per call
        # t-major inside a draw: row k of the call is pair start + k, which is where elbo() writes it
        assert [(int(t) * B + int(b)) for t, b in zip(c.t, c.layout)] == list(range(c.start, c.start + len(c.t)))
        seen += [(c.draw, int(t), int(b)) for t, b in zip(c.t, c.layout)]
    assert len(seen) == len(set(seen)) == n_draws * T * B
    assert set(seen) == {(d, t, b) for d in range(n_draws) for t in range(T) for b in range(B)}
    assert len(calls) == n_draws * math.ceil(T * B / max_rows)
    if B % max_rows == 0:                                                   # the single-t path's cuts: nothing changes there
        assert all(len(set(c.t.tolist())) == 1 for c in calls)


def test_elbo_calls_refuse_empty_shapes():
    for bad in ((0, 5, 1, 8), (4, 0, 1, 8), (4, 5, 0, 8), (4, 5, 1, 0)):
        with pytest.raises(ValueError):
            elbo_calls(*bad)


# ----------------------------------------------------------------------------- loss() / elbo() on a stand-in engine
S_FAKE = 10


def fake_sums(x0, t, xt_given):
    """(B,4) float64 'sums' that depend on the row's tokens, its timestep and whether x_t was given — nothing else"""
    base = x0.double().sum(1, keepdim=True) + torch.as_tensor(np.asarray(t), dtype=torch.float64).reshape(-1, 1) * 1000.0
    return base + torch.arange(4, dtype=torch.float64)[None] + (0.5 if xt_given else 0.0)


class FakeEngine:
    """What loss() / elbo() touch of binding.Engine, on the CPU.  A drawn x_t is x_0 + (seed + layout index + t) % 3: like the
    library's it depends on (seed, global layout index, t) alone, so the grouped and the per-layout path must agree on it."""

    def __init__(self, max_batch, per_layout_t=True):
        self.S, self.max_batch, self.batch_round = S_FAKE, max_batch, max_batch
        self.device = torch.device("cpu")
        self.per_layout_t = per_layout_t
        self.calls = []

    def _tok(self, t):
        return torch.as_tensor(t).to(torch.int32).contiguous()

    def _draw(self, x0, t, seed, layout):
        t = torch.as_tensor(np.asarray(t), dtype=torch.int64).reshape(-1)
        return x0 + ((seed + layout + t) % 3).int()[:, None]

    def q_sample(self, x0, t, seed=0, first_layout=0):
        self.calls.append(("q_sample", int(t), x0.shape[0]))
        return self._draw(x0, [t] * x0.shape[0], seed, first_layout + torch.arange(x0.shape[0]))

    def vb_step(self, x0, t, xt=None, seed=0, first_layout=0, out=None):
        self.calls.append(("vb_step", int(t), x0.shape[0], int(seed), int(first_layout)))
        assert x0.shape[0] <= self.max_batch
        if xt is None:
            xt = self._draw(x0, [t] * x0.shape[0], seed, first_layout + torch.arange(x0.shape[0]))
        out.copy_(fake_sums(xt, [t] * x0.shape[0], False))
        return out

    def vb_step_t(self, x0, t, xt=None, seed=0, first_layout=0, layout=None, out=None):
        assert self.per_layout_t, "an engine without the per-layout form raises (rc -4)"
        t = np.asarray(t)
        assert t.dtype == np.int32 and t.shape == (x0.shape[0],) and x0.shape[0] <= self.max_batch
        self.calls.append(("vb_step_t", tuple(t.tolist()), x0.shape[0], int(seed), int(first_layout), None if layout is None else tuple(int(v) for v in layout)))
        if xt is None:
            lay = torch.arange(x0.shape[0]) if layout is None else torch.as_tensor(np.asarray(layout, dtype=np.int64))
            xt = self._draw(x0, t, seed, first_layout + lay)
        out.copy_(fake_sums(xt, t, False))
        return out


def diffusion_over(engine, T=100):
    d = object.__new__(HipMaskAndReplaceDiffusion)      # (the constructor builds a GPU engine)
    d.engine, d.num_timesteps = engine, T
    d.Lt_history = d.Lt_count = None
    d.auxiliary_loss_weight, d.adaptive_auxiliary_loss = 0.1, True
    return d


@pytest.mark.parametrize("max_batch", [512, 64, 24])
@pytest.mark.parametrize("given_xt", [False, True])
def test_loss_makes_one_engine_call_per_window(max_batch, given_xt):
    B = 64
    g = torch.Generator().manual_seed(3)
    x0 = torch.randint(0, 50, (B, S_FAKE), generator=g).int()
    t = torch.randint(0, 100, (B,), generator=g)
    assert len(set(t.tolist())) >= 30
    pt = torch.full((B,), 0.01)
    xt = (x0 + 1) if given_xt else None
    eng = FakeEngine(max_batch)
    d = diffusion_over(eng)
    got = d.loss(x0, t=t, pt=pt, seed=5, x_t=xt, first_layout=11)
    assert len(eng.calls) == math.ceil(B / max_batch) and all(c[0] == "vb_step_t" for c in eng.calls)
    # t as given, window by window; the Philox layout index of a row is first_layout + its position in the batch
    assert sum((c[1] for c in eng.calls), ()) == tuple(t.tolist())
    offs = np.cumsum([0] + [c[2] for c in eng.calls])[:-1]
    assert [c[4] for c in eng.calls] == [11 + int(o) for o in offs] and all(c[5] is None for c in eng.calls)
    # the earlier path: one vb_step per distinct t (and, with drawn x_t, one whole-batch draw per distinct t) — the same values
    eng.calls.clear()
    old = d.loss(x0, t=t, pt=pt, seed=5, x_t=xt, first_layout=11, grouped=True)
    n_t = len(set(t.tolist()))
    assert len([c for c in eng.calls if c[0] == "vb_step"]) == n_t and not [c for c in eng.calls if c[0] == "vb_step_t"]
    assert len([c for c in eng.calls if c[0] == "q_sample"]) == (0 if given_xt else n_t * math.ceil(B / max_batch))
    assert set(got) == set(old) == {"kl_loss", "aux_loss"} and all(float(got[k]) == float(old[k]) for k in got)


def test_loss_groups_where_the_engine_has_no_per_layout_form():
    x0 = torch.arange(6 * S_FAKE).reshape(6, S_FAKE).int() % 50
    t = torch.tensor([3, 3, 0, 99, 0, 7])
    eng = FakeEngine(8, per_layout_t=False)
    got = diffusion_over(eng).loss(x0, t=t, pt=torch.full((6,), 0.01), seed=1)
    assert [c[0] for c in eng.calls].count("vb_step") == 4 and "vb_step_t" not in [c[0] for c in eng.calls]
    on = diffusion_over(FakeEngine(8)).loss(x0, t=t, pt=torch.full((6,), 0.01), seed=1)
    assert all(float(got[k]) == float(on[k]) for k in got)


@pytest.mark.parametrize("B,max_batch,n_draws", [(4, 8, 1), (3, 8, 2), (8, 8, 1), (16, 8, 1), (5, 512, 1)])
def test_elbo_packs_its_passes(B, max_batch, n_draws):
    T = 20
    x0 = (torch.arange(B * S_FAKE).reshape(B, S_FAKE) * 7 % 50).int()
    eng = FakeEngine(max_batch)
    got = diffusion_over(eng, T).elbo(x0, n_draws=n_draws, seed=9, first_layout=2)
    assert len(eng.calls) == n_draws * math.ceil(T * B / max_batch)
    if B % max_batch == 0:       # every call uniform in t: the single-t call, as before
        assert all(c[0] == "vb_step" for c in eng.calls)
    else:
        assert any(c[0] == "vb_step_t" for c in eng.calls)
        for c in (c for c in eng.calls if c[0] == "vb_step_t"):
            assert 9 <= c[3] < 9 + n_draws and c[4] == 2 and len(c[5]) == c[2] and all(0 <= b < B for b in c[5])
    # the T passes over the whole batch of an engine without the per-layout form give the same sum, added in the same order
    plain = FakeEngine(max_batch, per_layout_t=False)
    want = diffusion_over(plain, T).elbo(x0, n_draws=n_draws, seed=9, first_layout=2)
    assert len(plain.calls) == n_draws * T * math.ceil(B / max_batch)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))


# ----------------------------------------------------------------------------- the host build, per-row t against single t
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exes(request):
    san = request.param == "sanitized"
    return HB.host_program("cpu_vb_t_check", sanitize=san), HB.host_program("cpu_vb_check", sanitize=san)


def tail(t_rows, layout_rows):
    return np.asarray(t_rows, np.int32).tobytes() + np.asarray(layout_rows, np.uint64).tobytes()


@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_host_draw_with_per_row_t_equals_the_single_t_build(exes, tmp_path, ds, q_type):
    fx, spec = VC.fixture(), SP.SPECS[ds]
    per_row, single = exes
    x0 = fx[f"{VC.name(ds, q_type)}/x0"].astype(np.int32)
    B, S = x0.shape
    t_rows = [int(v) % spec.n_step for v in fx["t_mixed"][:B]]
    perm = list(reversed(range(B)))             # row b carries layout perm[b]: its x_0 and its Philox index
    rc, raw = HB.run_host_io(per_row, tmp_path, VC.payload(ds, q_type, 0, x0, seed=SEED, first_layout=FIRST) + tail(t_rows, range(B)), "draw")
    assert rc == 0
    err, got = VC.parse_draw(raw, B, S)
    rc, raw = HB.run_host_io(per_row, tmp_path, VC.payload(ds, q_type, 0, x0[perm], seed=SEED, first_layout=FIRST) + tail([t_rows[p] for p in perm], perm), "draw")
    assert rc == 0
    err_p, got_p = VC.parse_draw(raw, B, S)
    assert err == 0 and err_p == 0
    for t in sorted(set(t_rows)):
        rc, raw = HB.run_host_io(single, tmp_path, VC.payload(ds, q_type, t, x0, seed=SEED, first_layout=FIRST), "draw")
        assert rc == 0
        _, want = VC.parse_draw(raw, B, S)
        for b in (b for b in range(B) if t_rows[b] == t):
            assert np.array_equal(got[b], want[b]), (b, t)
            assert np.array_equal(got_p[perm.index(b)], want[b]), (b, t)
    assert len(set(t_rows)) > 1 and any(not np.array_equal(got[b], x0[b]) for b in range(B))


@pytest.mark.parametrize("ds,q_type", VC.MODELS)
@pytest.mark.parametrize("lse", [1, 0])
def test_host_terms_with_per_row_t_equal_the_single_t_build(exes, tmp_path, ds, q_type, lse):
    fx, spec = VC.fixture(), SP.SPECS[ds]
    per_row, single = exes
    p = f"{VC.name(ds, q_type)}/mixed/"
    x0 = fx[f"{VC.name(ds, q_type)}/x0"].astype(np.int32)
    xt = fx[p + "xt"].astype(np.int32)
    B, S = x0.shape
    t_rows = [int(v) for v in fx["t_mixed"][:B]]
    rows = np.random.default_rng(4).standard_normal((B, S, spec.n_class)).astype(np.float32) * 3   # (any logits: the terms' arithmetic is under test)
    rc, raw = HB.run_host_io(per_row, tmp_path, VC.payload(ds, q_type, 0, x0, xt, rows, lse=lse) + tail(t_rows, range(B)), "logits")
    assert rc == 0
    err, tok, sums = VC.parse_terms(raw, B, S)
    assert err == 0
    for t in sorted(set(t_rows)):
        rc, raw = HB.run_host_io(single, tmp_path, VC.payload(ds, q_type, t, x0, xt, rows, lse=lse), "logits")
        assert rc == 0
        _, tok1, sums1 = VC.parse_terms(raw, B, S)
        for b in (b for b in range(B) if t_rows[b] == t):
            assert np.array_equal(tok[:, b].view(np.int32), tok1[:, b].view(np.int32)), (b, t)
            assert np.array_equal(sums[b].view(np.int64), sums1[b].view(np.int64)), (b, t)
    assert len(set(t_rows)) > 1
