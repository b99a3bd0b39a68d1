"""GPU: the training loss's gradient with respect to the logits (ldm_vb_grad, kernels_vb.hip vb_grad_k) and the autograd bridge
built on it (layout_dm_amd/training.py), on the fixture of the reference's own autograd (tests/golden/vb_grad).

Bar, per token row: 4 x that row's recorded float32-vs-float64 distance of the reference's own autograd (_vb_grad_cases.bars), against
the reference's float64 gradient.  The kernel evaluates the backward in float64 from the float32 logits and rounds once, as the host
program does; its double-precision exp / log are the device library's, the host program's glibc's.  Measured on an MI355X: on all
24 fixture cases every element has the host program's bits (0 of 523 440 differ), so the test asserts exactly that; the worst share
of the bar is 0.25 on every model (0.083 at t = 0), the host program's own."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import _hostbuild as HB
import _vb_grad_cases as G
from oracle import synth
from test_training_host import TRAIN_LR, Stub

pytestmark = pytest.mark.gpu

SMALL = dict(d_model=64, n_head=4, d_ff=128, n_layer=1)   # the denoiser is never run here: a small backbone loads fast
_DIFF = {}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


def diffusion(model, precision="exact"):
    """the HipMaskAndReplaceDiffusion of a fixture model (S = 20), once per session"""
    import dataclasses

    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    key = (model, precision)
    if key not in _DIFF:
        backbone = SMALL if precision == "exact" else {}
        spec, q_type = dataclasses.replace(G.spec_of(model), **backbone), G.MODELS[model][1]
        d = HipMaskAndReplaceDiffusion(n_category=spec.n_category, n_bin=spec.n_bin, max_elem=spec.max_elem, precision=precision,
                                       max_batch=8, q_type=q_type, **backbone)
        d.load_state_dict(synth.synth_state_dict(spec, seed=int(G.fixture()["weight_seed"]), perturb=True, q_type=q_type))
        _DIFF[key] = d
    return _DIFF[key]


def bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def case_tensors(model, case, dev):
    fx = G.fixture()
    p = f"{model}/{case}/"
    as_i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
    return (torch.from_numpy(G.arrays(model, case)[0]).to(dev), as_i32(fx[f"{model}/x0"]), as_i32(fx[p + "xt"]), fx[p + "t"],
            G.coefficients(model, case))


@pytest.mark.parametrize("model", list(G.MODELS))
def test_fixture_gradient(cuda, tmp_path, model):
    e = diffusion(model).engine
    exe = HB.host_program("cpu_vb_grad_check")
    spec = G.spec_of(model)
    for case in G.CASES:
        logits, x0, xt, t, coef = case_tensors(model, case, cuda)
        grad, sums = e.vb_grad(logits, x0, xt, t, coef)
        got = grad.cpu().numpy()
        share = G.share_of_bar(got, model, case)
        rc, raw = HB.run_host_io(exe, tmp_path, G.case_payload(model, case), "grad")
        assert rc == 0
        _, host, _, _ = G.parse(raw, *x0.shape, spec.n_class)
        differ = got.view(np.uint32) != host.view(np.uint32)
        print(f"{model}/{case}: worst share of the bar {share:.3f}; {int(differ.sum())} of {differ.size} elements differ from the host program's bits")
        assert np.isfinite(got).all() and (got[..., -1] == 0).all()
        assert share <= 1.0
        assert not differ.any()
        assert torch.equal(bits(sums), bits(e.vb_terms_t(logits, x0, xt, t))), case
        assert torch.equal(bits(e.vb_grad(logits, x0, xt, t, None, want_grad=False)[1]), bits(sums)), case


@pytest.mark.parametrize("model", ["rico25_constrained", "rico25_vanilla", "rico25b64_constrained"])
def test_repeat_and_batch_independence(cuda, model):
    e = diffusion(model).engine
    logits, x0, xt, t, coef = case_tensors(model, "sharp", cuda)
    grad, sums = e.vb_grad(logits, x0, xt, t, coef)
    again, sums2 = e.vb_grad(logits, x0, xt, t, coef)
    assert torch.equal(bits(grad), bits(again)) and torch.equal(bits(sums), bits(sums2))
    for cuts in ((2, 4), (1,) * 6):
        off = 0
        for n in cuts:
            g, s = e.vb_grad(logits[off:off + n], x0[off:off + n], xt[off:off + n], t[off:off + n], coef[off:off + n])
            assert torch.equal(bits(g), bits(grad[off:off + n])) and torch.equal(bits(s), bits(sums[off:off + n])), (cuts, off)
            off += n


def test_handle_independence(cuda):
    """a `fast` handle (fp16 denoiser, no per-layout timesteps of its own) gives the bits of the `exact` one: the kernel does not
    depend on the numerics mode"""
    model = "rico25_constrained"
    exact, fast = diffusion(model).engine, diffusion(model, "fast").engine
    for case in ("mixed", "sharp"):
        logits, x0, xt, t, coef = case_tensors(model, case, cuda)
        g0, s0 = exact.vb_grad(logits, x0, xt, t, coef)
        g1, s1 = fast.vb_grad(logits, x0, xt, t, coef)
        assert torch.equal(bits(g0), bits(g1)) and torch.equal(bits(s0), bits(s1))


def test_refusals(cuda):
    model = "rico25_constrained"
    e = diffusion(model).engine
    spec = G.spec_of(model)
    logits, x0, xt, t, coef = case_tensors(model, "mixed", cuda)
    want, _ = e.vb_grad(logits, x0, xt, t, coef)
    for bad in (-1, spec.n_step):
        tb = t.copy()
        tb[3] = bad
        with pytest.raises(RuntimeError, match="out of range"):
            e.vb_grad(logits, x0, xt, tb, coef)
    x0b = x0.clone()
    x0b[2, 7] = spec.mask_id
    with pytest.raises(ValueError, match="MASK"):
        e.vb_grad(logits, x0b, xt, t, coef)
    # the library call itself: -6, the refused token's row zero, every other row as before
    grad = torch.full_like(logits, float("nan"))
    sums = torch.empty((6, 4), dtype=torch.float64, device=cuda)
    ht = np.ascontiguousarray(t, np.int32)
    cd = torch.from_numpy(coef).to(cuda)
    rc = e.lib.ldm_vb_grad(e._h, logits.data_ptr(), x0b.data_ptr(), xt.data_ptr(), ht.ctypes.data_as(C.c_void_p), 6, cd.data_ptr(),
                           grad.data_ptr(), sums.data_ptr(), int(torch.cuda.current_stream(cuda).cuda_stream))
    assert rc == -6
    assert (grad[2, 7] == 0).all()
    keep = torch.ones(x0.shape, dtype=torch.bool, device=cuda)
    keep[2, 7] = False
    assert torch.equal(bits(grad[keep]), bits(want[keep]))


class Recording(torch.nn.Module):
    """a stub transformer that keeps its logits as a leaf-like tensor with retain_grad()"""

    def __init__(self, stub):
        super().__init__()
        self.stub = stub

    def forward(self, x, timestep=None):
        self.x, self.timestep = x, timestep
        self.logits = self.stub(x, timestep=timestep)["logits"]
        self.logits.retain_grad()
        return {"logits": self.logits}


def test_bridge(cuda):
    from layout_dm_amd.training import TrainableDiffusion, loss_coefficients

    model = "rico25_constrained"
    d = diffusion(model)
    spec, fx = G.spec_of(model), G.fixture()
    e, T = d.engine, spec.n_step
    x0 = torch.from_numpy(fx[f"{model}/x0"].astype(np.int64))
    B, S = x0.shape
    stub = Stub(spec.n_class, T).to(cuda)
    twin = copy.deepcopy(stub)
    td = TrainableDiffusion(d, Recording(stub))
    # a history that makes sample_time draw by importance (base.py:181), and what that draw will be
    g = torch.Generator().manual_seed(11)
    d.Lt_history, d.Lt_count = torch.rand(T, generator=g) * 4.0 + 0.01, torch.full((T,), 11.0)
    hist0, count0 = d.Lt_history.clone(), d.Lt_count.clone()
    torch.manual_seed(5)
    t_want, pt_want = d.sample_time(B)
    torch.manual_seed(5)
    try:
        outputs, losses = td(x0, is_train=True, seed=77)
        assert set(losses) == {"kl_loss", "aux_loss"} and set(outputs) == {"x_t", "t"}
        assert torch.equal(outputs["t"].cpu(), t_want) and outputs["x_t"].shape == (B, S)
        assert torch.equal(outputs["x_t"], e.q_sample_t(x0, t_want.numpy(), 77, 0))
        (losses["kl_loss"] + losses["aux_loss"]).backward()
        rec = td.transformer
        coef = loss_coefficients(t_want.numpy(), pt_want.numpy(), T, d.auxiliary_loss_weight, True, 1.0, 1.0, B, S)
        want, sums = e.vb_grad(rec.logits.detach(), x0, outputs["x_t"], t_want.numpy(), coef)
        assert torch.equal(bits(rec.logits.grad), bits(want))
        # the loss values are the coefficients times the sums
        sums = sums.cpu().numpy()
        first = t_want.numpy() == 0
        kl = float((coef[:, 0] * np.where(first, sums[:, 1], sums[:, 0])).sum())
        aux = float((coef[:, 1] * np.where(first, sums[:, 1], sums[:, 2])).sum())
        assert abs(losses["kl_loss"].item() / kl - 1) < 1e-6 and abs(losses["aux_loss"].item() / aux - 1) < 1e-6
        # parameter gradients: PyTorch's backward of the stub on that tensor
        twin(rec.x, timestep=rec.timestep)["logits"].backward(want)
        for (n, p), (_, q) in zip(stub.named_parameters(), twin.named_parameters()):
            assert p.grad is not None and torch.equal(bits(p.grad), bits(q.grad)), n
        # Lt_history / Lt_count (constrained.py:307-311), by hand: the gathers read the old buffer, a repeated t keeps its last write
        kl_loss = (np.where(first, sums[:, 1], sums[:, 0]) / S).astype(np.float32)
        hist, count = hist0.clone(), count0.clone()
        for b in range(B):
            tb = int(t_want[b])
            hist[tb] = torch.tensor(0.1) * torch.tensor(kl_loss[b]) ** 2 + torch.tensor(0.9) * hist0[tb]
            count[tb] += 1
        assert torch.equal(d.Lt_count, count) and torch.allclose(d.Lt_history, hist, rtol=1e-6, atol=0)
        assert not torch.equal(d.Lt_history, hist0)
        # is_train=False: no aux loss, and the gradient is the kl column's alone
        pt_all = d.time_weights()                                  # (the history has moved: so have the weights)
        torch.manual_seed(5)
        stub.zero_grad()
        outputs, losses = td(x0, is_train=False, seed=77)
        assert set(losses) == {"kl_loss"}
        losses["kl_loss"].backward()
        pt2 = pt_all.gather(0, outputs["t"].cpu())
        coef =loss_coefficients(outputs["t"].cpu().numpy(), pt2.numpy(), T, d.auxiliary_loss_weight, True, 1.0, 0.0, B, S)
        want, _ = e.vb_grad(rec.logits.detach(), x0, outputs["x_t"], outputs["t"].cpu().numpy(), coef)
        assert torch.equal(bits(rec.logits.grad), bits(want))
    finally:
        d.Lt_history, d.Lt_count = None, None


def test_it_trains(cuda):
    """30 plain-SGD steps on fixed (x_0, t, x_t) at the step size the CPU rehearsal chose (test_training_host.TRAIN_LR = 0.1)"""
    from layout_dm_amd.training import TrainableDiffusion

    model = "rico25_constrained"
    d = diffusion(model)
    spec = G.spec_of(model)
    x0 = torch.from_numpy(G.fixture()[f"{model}/x0"].astype(np.int64))
    td = TrainableDiffusion(d, Stub(spec.n_class, spec.n_step).to(cuda))
    opt = torch.optim.SGD(td.parameters(), lr=TRAIN_LR)
    losses = []
    try:
        for _ in range(31):
            d.Lt_history, d.Lt_count = None, None       # (uniform t, pt = 1 / T: the same draw every step)
            torch.manual_seed(9)
            _, out = td(x0, seed=123)
            loss = out["kl_loss"] + out["aux_loss"]
            losses.append(loss.item())
            opt.zero_grad()
            loss.backward()
            opt.step()
    finally:
        d.Lt_history, d.Lt_count = None, None
    print(f"kl_loss + aux_loss: {losses[0]:.4f} -> {losses[30]:.4f}")
    assert np.isfinite(losses).all() and losses[30] < losses[0]
