"""The training seam: the reference's diffusion loss (constrained.py:232-333, vanilla.py:160-240) as a differentiable function of
the logits it is computed from.  Everything behind the logits — log-softmax and clamp, the two posteriors, kl / decoder nll /
auxiliary kl, the t == 0 selection and the importance weights — is one HIP launch each way (ldm_vb_grad: kernels_vb.hip vb_grad_k,
arithmetic in ldm_vb_core.h token_grad); the transformer in front of the logits is the caller's torch module, and its backward is
PyTorch's.  No optimiser, scheduler, data loading or checkpoint writing here, and nothing syncs torch weights into a HIP engine.

    loss_coefficients   (B,2) per-layout weights of the token sums in the two loss scalars, on the host
    DiffusionLoss       torch.autograd.Function: logits -> (kl_loss, aux_loss); backward is one ldm_vb_grad call
    TrainableDiffusion  nn.Module with the reference's forward(x, is_train) -> (outputs, losses)
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np
import torch


def loss_coefficients(t, pt, T: int, aux_weight: float, adaptive: bool, g_kl: float, g_aux: float, B: int, S: int,
                      dtype=np.float64) -> np.ndarray:
    """(B,2) coefficients c with  g_kl * kl_loss + g_aux * aux_loss = sum_b c[b,0] * (t_b == 0 ? nll_b : kl_b) + c[b,1] *
    (t_b == 0 ? nll_b : aux_b)  over the per-layout token SUMS (constrained.py:299-330): c[b,0] = g_kl / (B S pt_b), c[b,1] =
    g_aux w_b aux_weight / (B S pt_b), w_b = (1 - t_b / T) + 1 when adaptive, else 1.  w_b aux_weight is evaluated in float32 as
    the reference evaluates it (an integer tensor divided by T, times a Python float: float32 whatever the module's dtype), the
    rest in float64, which is what ldm_vb_grad takes: a coefficient rounded to float32 moves every element of the gradient by up
    to 6e-8 of itself, more than the reference's own float32 autograd keeps to its float64 one on many rows."""
    t = np.asarray(t).reshape(-1).astype(np.int64)
    pt = np.asarray(pt).reshape(-1).astype(np.float64)
    if t.size != B or pt.size != B:
        raise ValueError(f"t and pt must hold {B} values, one per layout")
    w = (np.float32(1) - t.astype(np.float32) / np.float32(T)) + np.float32(1) if adaptive else np.ones(B, np.float32)
    wa = (w * np.float32(aux_weight)).astype(np.float64)
    den = float(B) * float(S) * pt
    return np.stack([float(g_kl) / den, float(g_aux) * wa / den], axis=1).astype(dtype)


@dataclasses.dataclass
class LossConfig:
    """What DiffusionLoss needs besides the tensors.  aux: whether the auxiliary loss is returned (auxiliary_loss_weight != 0 and
    is_train, constrained.py:316).  sums: set by forward — the call's (B,4) float64 per-layout token sums kl, nll, aux, hits."""
    T: int
    aux_weight: float = 0.1
    adaptive: bool = True
    aux: bool = True
    sums: Optional[torch.Tensor] = None


def _windows(B: int, n: int):
    return [(off, min(n, B - off)) for off in range(0, B, n)]


class DiffusionLoss(torch.autograd.Function):
    """(logits (B,S,C) float32 on the engine's device, x0, xt (B,S) tokens, t (B,) timesteps and pt (B,) their sampling
    probabilities on the host, engine, cfg: LossConfig) -> (kl_loss, aux_loss) 0-dim float32 tensors on the logits' device —
    (kl_loss,) alone when cfg.aux is False or cfg.aux_weight is 0, like loss().  forward is the values-only ldm_vb_grad call;
    backward one ldm_vb_grad call with the coefficients built on the host from the two upstream scalars."""

    @staticmethod
    def forward(ctx, logits, x0, xt, t, pt, engine, cfg):
        B, S = x0.shape
        t = np.asarray(torch.as_tensor(t).cpu().numpy(), np.int64).reshape(-1)
        pt = np.asarray(torch.as_tensor(pt).cpu().numpy(), np.float64).reshape(-1)
        x0, xt = engine._tok(x0), engine._tok(xt)
        logits = logits.detach().to(device=engine.device, dtype=torch.float32).contiguous()
        sums = torch.empty((B, 4), dtype=torch.float64, device=engine.device)
        for off, n in _windows(B, engine.max_batch):
            sums[off:off + n] = engine.vb_grad(logits[off:off + n], x0[off:off + n], xt[off:off + n], t[off:off + n], None,
                                               want_grad=False)[1]
        cfg.sums = sums
        aux = bool(cfg.aux) and cfg.aux_weight != 0
        ctx.save_for_backward(logits, x0, xt)
        ctx.t, ctx.pt, ctx.engine, ctx.cfg, ctx.aux = t, pt, engine, cfg, aux
        c = torch.from_numpy(loss_coefficients(t, pt, cfg.T, cfg.aux_weight, cfg.adaptive, 1.0, 1.0, B, S)).to(engine.device)
        first = torch.from_numpy(t == 0).to(engine.device)
        kl = (c[:, 0] * torch.where(first, sums[:, 1], sums[:, 0])).sum().float()
        if not aux:
            return (kl,)
        return kl, (c[:, 1] * torch.where(first, sums[:, 1], sums[:, 2])).sum().float()

    @staticmethod
    def backward(ctx, g_kl, g_aux=None):
        logits, x0, xt = ctx.saved_tensors
        engine, cfg = ctx.engine, ctx.cfg
        B, S = x0.shape
        g = torch.stack([g_kl, g_aux if ctx.aux else torch.zeros_like(g_kl)]).double().cpu().numpy()   # the one read-back
        coef = torch.from_numpy(loss_coefficients(ctx.t, ctx.pt, cfg.T, cfg.aux_weight, cfg.adaptive, g[0], g[1], B, S)).to(engine.device)
        grad = torch.empty_like(logits)
        for off, n in _windows(B, engine.max_batch):
            grad[off:off + n] = engine.vb_grad(logits[off:off + n], x0[off:off + n], xt[off:off + n], ctx.t[off:off + n],
                                               coef[off:off + n])[0]
        return grad, None, None, None, None, None, None


class TrainableDiffusion(torch.nn.Module):
    """The reference's training seam (LayoutDM.forward -> self.model(inputs["seq"])) on the MI355X: built from a
    HipMaskAndReplaceDiffusion — its schedule, vocabulary, Lt_history / Lt_count, sample_time and forward noising draw — and a
    caller-supplied torch module called as base.py:129 calls it, transformer(x_t, timestep=t) -> {"logits": (B,S,C)}.

    forward(x, is_train=True, seed=None) -> (outputs, losses) with the reference's keys (constrained.py:232-333):
        t, pt = inner.sample_time(B); x_t ~ q(x_t | x_0) by ldm_q_sample_t (the project's Philox stream keyed by seed, layout
        index, t and position — not the reference's Gumbel stream; seed None draws the key from torch's global CPU generator);
        the transformer under autograd; DiffusionLoss; the reference's Lt_history / Lt_count update (l.307-311: 0.1 / 0.9 running
        mean of the per-layout kl_loss squared, detached) on the inner object's buffers; is_train=False drops the aux loss (l.316).
    outputs = {"x_t": x_t, "t": t}.  The reference's outputs["probs"] — exp of the (B,C,S) model posterior — is NOT materialised:
    the loss never forms that tensor.  The accuracy bookkeeping (diffusion_acc_list / diffusion_keep_list) is not kept either.
    The draw needs an engine with per-layout timesteps (Engine.per_layout_t: every engine but `fast` on the reference's
    backbone).  The inner object's own HIP denoiser is not run and does not see the transformer's weights: load_state_dict it
    with them, as today, to sample from what was trained."""

    def __init__(self, inner, transformer: torch.nn.Module):
        super().__init__()
        self.transformer = transformer
        self._inner = [inner]   # (not a submodule, and not in the state dict)

    @property
    def inner(self):
        return self._inner[0]

    def forward(self, x, is_train: bool = True, seed: Optional[int] = None):
        inner = self.inner
        eng, T = inner.engine, inner.num_timesteps
        x0 = eng._tok(torch.as_tensor(x))
        B = x0.shape[0]
        t, pt = inner.sample_time(B)
        seed = inner._draw_seed(seed)
        tn = t.numpy().astype(np.int32)
        parts = [eng.q_sample_t(x0[off:off + n], tn[off:off + n], seed, off) for off, n in _windows(B, eng.max_batch)]
        x_t = torch.cat(parts) if len(parts) > 1 else parts[0]
        t_dev = t.to(eng.device)
        logits = self.transformer(x_t.long(), timestep=t_dev)["logits"]
        cfg = LossConfig(T=T, aux_weight=inner.auxiliary_loss_weight, adaptive=inner.adaptive_auxiliary_loss, aux=bool(is_train))
        out = DiffusionLoss.apply(logits, x0, x_t, t, pt, eng, cfg)
        losses = {"kl_loss": out[0]}
        if len(out) > 1:
            losses["aux_loss"] = out[1]
        # constrained.py:304-311 on the host buffers, float32 like the reference's
        sums = cfg.sums.cpu()
        kl_loss = (torch.where(t == 0, sums[:, 1], sums[:, 0]) / eng.S).float()
        if inner.Lt_history is None or inner.Lt_count is None:
            inner.Lt_history, inner.Lt_count = torch.zeros(T), torch.zeros(T)
        Lt2 = kl_loss.pow(2)
        inner.Lt_history.scatter_(0, t, 0.1 * Lt2 + 0.9 * inner.Lt_history.gather(0, t))
        inner.Lt_count.scatter_add_(0, t, torch.ones_like(Lt2))
        return {"x_t": x_t, "t": t_dev}, losses
