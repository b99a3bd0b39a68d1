"""Host side of the training seam (layout_dm_amd/training.py), no GPU: loss_coefficients against the scalars the reference's own
forward() returned (tests/golden/vb_grad, tools/make_vb_grad_golden.py), and the CPU rehearsal of tests/test_vb_grad_gpu.py's
training loop through the host program's gradient (tests/cpu_vb_grad_check.cpp)."""
import numpy as np
import pytest
import torch

import _hostbuild
import _vb_grad_cases as G
from layout_dm_amd.training import loss_coefficients

TRAIN_LR = 0.1   # the smallest of {1, 0.3, 0.1} at which the rehearsal below ends lower than it starts (367.7 -> 66.8; 1 and 0.3 end above 4800)


def selected(sums, t):
    """(B,) the token sums kl_loss and aux_loss weigh: nll at t == 0 (constrained.py:304-305, 322), else kl / aux"""
    first = t == 0
    return np.where(first, sums[:, 1], sums[:, 0]), np.where(first, sums[:, 1], sums[:, 2])


@pytest.mark.parametrize("model", list(G.MODELS))
def test_coefficients_reproduce_the_reference_scalars(model):
    """coefficients x the recorded float64 token sums == the float64 module's kl_loss / aux_loss to float64 rounding (the sum over
    B x S terms in another order: a few ulps), and the float32 module's scalars to float32 rounding"""
    fx, spec = G.fixture(), G.spec_of(model)
    for case in G.CASES:
        p = f"{model}/{case}/"
        t, sums = fx[p + "t"], fx[p + "sums64"]
        B, S = fx[p + "xt"].shape
        c = loss_coefficients(t, fx[p + "pt"], spec.n_step, G.AUX_WEIGHT, True, 1.0, 1.0, B, S)
        assert c.shape == (B, 2) and c.dtype == np.float64
        s_kl, s_aux = selected(sums, t)
        kl, aux = float((c[:, 0] * s_kl).sum()), float((c[:, 1] * s_aux).sum())
        assert abs(kl / float(fx[p + "kl_loss64"]) - 1) < 1e-14 and abs(aux / float(fx[p + "aux_loss64"]) - 1) < 1e-14, case
        assert abs(kl / float(fx[p + "kl_loss"]) - 1) < 1e-5 and abs(aux / float(fx[p + "aux_loss"]) - 1) < 1e-5, case


def test_t_zero_selects_the_decoder_nll():
    fx = G.fixture()
    p = "rico25_constrained/mixed/"
    t, sums = fx[p + "t"], fx[p + "sums64"]
    assert t[0] == 0 and (t[1:] != 0).all()
    s_kl, s_aux = selected(sums, t)
    assert s_kl[0] == sums[0, 1] == s_aux[0] and (s_kl[1:] == sums[1:, 0]).all() and (s_aux[1:] == sums[1:, 2]).all()
    # ... and the t0 case is the decoder nll alone: with the kl and aux sums scrambled the scalars do not move
    p = "rico25_constrained/t0/"
    t, sums = fx[p + "t"], fx[p + "sums64"].copy()
    c = loss_coefficients(t, fx[p + "pt"], 100, G.AUX_WEIGHT, True, 1.0, 1.0, *fx[p + "xt"].shape)
    sums[:, 0], sums[:, 2] = 1e9, -1e9
    s_kl, s_aux = selected(sums, t)
    assert abs(float((c[:, 0] * s_kl).sum()) / float(fx[p + "kl_loss64"]) - 1) < 1e-14
    assert abs(float((c[:, 1] * s_aux).sum()) / float(fx[p + "aux_loss64"]) - 1) < 1e-14


def test_coefficient_forms():
    t, pt = np.array([0, 1, 50, 99]), np.array([0.01, 0.02, 0.005, 0.04])
    B, S, T = 4, 20, 100
    c = loss_coefficients(t, pt, T, 0.1, True, 1.0, 1.0, B, S)
    assert np.allclose(c[:, 0], 1.0 / (B * S * pt), rtol=1e-15)
    w = (np.float32(1) - t.astype(np.float32) / np.float32(T)) + np.float32(1)          # float32 like the reference's (l.324)
    assert np.array_equal(c[:, 1], (w * np.float32(0.1)).astype(np.float64) / (B * S * pt))
    assert w[0] == 2 and abs(w[3] - 1.01) < 1e-6
    # adaptive=False: weight 1 at every t; aux_weight 0: no auxiliary term; the upstream gradients scale their own column
    flat = loss_coefficients(t, pt, T, 0.1, False, 1.0, 1.0, B, S)
    assert np.array_equal(flat[:, 1], np.float64(np.float32(0.1)) / (B * S * pt)) and np.array_equal(flat[:, 0], c[:, 0])
    assert (loss_coefficients(t, pt, T, 0.0, True, 1.0, 1.0, B, S)[:, 1] == 0).all()
    g = loss_coefficients(t, pt, T, 0.1, True, 3.0, -0.5, B, S)
    assert np.allclose(g[:, 0], 3.0 * c[:, 0], rtol=1e-15) and np.allclose(g[:, 1], -0.5 * c[:, 1], rtol=1e-15)
    assert loss_coefficients(t, pt, T, 0.1, True, 1.0, 1.0, B, S, dtype=np.float32).dtype == np.float32
    with pytest.raises(ValueError):
        loss_coefficients(t[:3], pt, T, 0.1, True, 1.0, 1.0, B, S)


class Stub(torch.nn.Module):
    """the stand-in transformer of the training tests: nn.Embedding -> nn.Linear, called as base.py:129 calls the reference's"""

    def __init__(self, C, T, D=32, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.emb, self.temb, self.lin = torch.nn.Embedding(C, D), torch.nn.Embedding(T, D), torch.nn.Linear(D, C)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)

    def forward(self, x, timestep=None):
        return {"logits": self.lin(self.emb(x) + self.temb(timestep)[:, None, :])}


def test_training_loop_rehearsal(tmp_path):
    """30 plain-SGD steps of the stub on the fixture's (x_0, x_t, t, pt) of rico25 `mixed`, d loss / d logits from the host
    program, at each step size of {1, 0.3, 0.1}: the smallest at which kl_loss + aux_loss stays finite and ends below where it
    started is TRAIN_LR, the step size of the GPU test.  (The loss carries 1 / pt ~ 100: at 1 and 0.3 plain SGD overshoots.)"""
    model, case = "rico25_constrained", "mixed"
    fx, spec = G.fixture(), G.spec_of(model)
    exe = _hostbuild.host_program("cpu_vb_grad_check")
    p = f"{model}/{case}/"
    x0, xt, t = fx[f"{model}/x0"], fx[p + "xt"], fx[p + "t"]
    B, S = xt.shape
    coef = G.coefficients(model, case)
    works = []
    for lr in (1.0, 0.3, 0.1):
        stub = Stub(spec.n_class, spec.n_step)
        opt = torch.optim.SGD(stub.parameters(), lr=lr)
        losses = []
        for _ in range(31):
            logits = stub(torch.from_numpy(xt.astype(np.int64)), timestep=torch.from_numpy(t.astype(np.int64)))["logits"]
            rc, raw = _hostbuild.run_host_io(exe, tmp_path, G.payload(model, x0, xt, logits.detach().numpy(), t, coef), "grad")
            assert rc == 0
            err, grad, _, sums = G.parse(raw, B, S, spec.n_class)
            assert err == 0
            s_kl, s_aux = selected(sums, t)
            losses.append(float((coef[:, 0] * s_kl).sum() + (coef[:, 1] * s_aux).sum()))
            opt.zero_grad()
            logits.backward(torch.from_numpy(grad.copy()))
            opt.step()
        print(f"lr {lr}: loss {losses[0]:.4f} -> {losses[30]:.4f}")
        if np.isfinite(losses).all() and losses[30] < losses[0]:
            works.append(lr)
    assert works and min(works) == TRAIN_LR
