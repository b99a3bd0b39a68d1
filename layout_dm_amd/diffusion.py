"""Host-side mirror of the reference's diffusion class for the sampling path.

`HipMaskAndReplaceDiffusion` exposes the public surface the reference's callers use on
`ConstrainedMaskAndReplaceDiffusion` (trainer/models/categorical_diffusion/constrained.py:27,
base.py:293-371): construct from the model geometry, `load_state_dict` with the reference's
checkpoint keys, `.sample(batch_size, cond, sampling_cfg, get_intermediate_results)` returning a
CPU LongTensor (B,S).  Everything numeric runs in libldm_hip.so; this file only does what
`sample()` does on the host in the reference: the timestep list, skip-step bookkeeping, cond
duplication and dtype plumbing.
"""
from __future__ import annotations

import itertools
import logging
from typing import Dict, List, NamedTuple, Optional, Union

import numpy as np
import torch

from .binding import Engine
from .selection import FP16_MAX_CLASSES, RUNGS, THROUGHPUT_CLASS  # noqa: F401  (theirs, under the names they had here)
from .selection import Selector, selection_message, selection_report

_seed_counter = itertools.count()
# the reference's entry point logs at INFO (trainer/test.py:38); `precision="auto"` says here which engine a checkpoint got and why
logger = logging.getLogger("layout_dm_amd")

POS_EMBS = ("elem_attr", "default")   # ElementPositionalEmbedding | PositionalEmbedding (nn_lib.py:73-127)
INSTANCE_NORM_TYPES = ("adainnorm", "adainnorm_abs")
TIMESTEP_TYPES = ("adalayernorm", "adalayernorm_abs", None) + INSTANCE_NORM_TYPES


def check_timestep_type(timestep_type) -> None:
    """Raises for what Block accepts (transformer_utils.py:124-132) but nobody can run, and for anything else unknown."""
    if timestep_type in ("adalayernorm_mlp", "adainnorm_mlp"):
        raise NotImplementedError(
            f"timestep_type={timestep_type}: not supported, and the reference cannot run it either — its embedding MLP starts with "
            "nn.Linear(1, d_model / 2) and is fed the integer (Long) timestep, which raises a dtype error on the first forward pass")
    if timestep_type not in TIMESTEP_TYPES:
        raise NotImplementedError(f"timestep_type={timestep_type}: one of {sorted(map(str, TIMESTEP_TYPES))}")


def variant_name(pos_emb: str, timestep_type) -> Optional[str]:
    """What names a denoiser variant in reports, or None for the default (elem_attr positions, adalayernorm)."""
    parts = ([f"pos_emb={pos_emb}"] if pos_emb != "elem_attr" else []) + \
            ([f"timestep_type={timestep_type}"] if timestep_type != "adalayernorm" else [])
    return ", ".join(parts) or None


def _cfg_get(cfg, key, default=None):
    if cfg is None:
        return default
    if hasattr(cfg, "get"):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def schedule_and_seed(num_timesteps: int, sampling_cfg, seed: Optional[int]):
    """(t_model, t_post, seed) of one sampling call: the schedule sampling_cfg asks for, and the Philox key — `seed`, or one drawn
    from torch's global CPU generator.  Deterministic decoding draws nothing — and must not advance that generator either: the
    reference's argmax path consumes no random numbers (helpers/sampling.py:110-111), and test.py's get_cond of the NEXT batch
    reads that stream."""
    t_model, t_post = timestep_schedule(num_timesteps, int(_cfg_get(sampling_cfg, "num_timesteps", num_timesteps)),
                                        float(_cfg_get(sampling_cfg, "time_difference", 0.0) or 0.0))
    if seed is None:
        seed = 0 if str(_cfg_get(sampling_cfg, "name")) == "deterministic" else int(torch.randint(0, 2 ** 62, (1,)).item())
    return t_model, t_post, seed


def batch_cuts(B: int, max_batch: int, round_: int) -> List[int]:
    """Sizes of the calls a batch of B layouts is cut into when it exceeds max_batch.  The reference caps a call at 512
    (test.py splits 1000 into 512 + 488); here a call costs whole ROUNDS of `round_` layouts (Engine.batch_round: one
    workgroup per layout per compute unit), so the cuts are the largest multiple of the round that fits max_batch — 1000
    layouts under max_batch = 600 are 512 + 488 (4 rounds), not 600 + 400 (5)."""
    if B <= max_batch:
        return [B] if B > 0 else []
    step = (max_batch // round_) * round_ or max_batch
    return [step] * (B // step) + ([B % step] if B % step else [])


class ElboCall(NamedTuple):
    """One engine call of elbo(): rows start .. start + len(t) - 1 of draw `draw`'s (t, layout) pairs in t-major order."""
    draw: int
    start: int          # index of the call's first row among the draw's T * B pairs: pair i is (t = i // B, layout = i % B)
    t: np.ndarray       # (n,) int32 timestep of every row
    layout: np.ndarray  # (n,) int64 layout of every row


def elbo_calls(B: int, T: int, n_draws: int, max_rows: int) -> List[ElboCall]:
    """The engine calls elbo() makes on an engine with per-layout timesteps: the (draw, t, layout) triples flattened t-major
    (layout fastest) and cut into calls of at most max_rows rows.  Rows of a call share a draw — the Philox seed is per call.
    With B a multiple of max_rows every call is uniform in t (the cuts of the single-t path)."""
    if B < 1 or T < 1 or n_draws < 1 or max_rows < 1:
        raise ValueError("B, T, n_draws and max_rows must be >= 1")
    calls = []
    for d in range(n_draws):
        for start in range(0, T * B, max_rows):
            i = np.arange(start, min(start + max_rows, T * B), dtype=np.int64)
            calls.append(ElboCall(d, start, (i // B).astype(np.int32), i % B))
    return calls


def timestep_schedule(num_timesteps: int, num_timesteps_eval: int, time_difference: float = 0.0):
    """(t_model list, t_post list) exactly as base.py:310-315 + 218-240 derive them:
    diffusion_list = [int(i*T/T_eval)], skip_step = delta_t - 1, noise_t = clamp(t - int(T*td)),
    posterior evaluated at noise_t - skip_step when noise_t > skip_step."""
    assert num_timesteps_eval <= num_timesteps  # base.py:311
    t_model, t_post = [], []
    prev = num_timesteps
    for i in range(num_timesteps_eval - 1, -1, -1):
        t = int(i * num_timesteps / num_timesteps_eval)
        delta = prev - t
        if delta <= 0:
            raise NotImplementedError  # base.py:361-362
        skip = delta - 1
        noise_t = t
        if time_difference > 0.0:
            noise_t = min(max(t - int(num_timesteps * time_difference), 0), num_timesteps - 1)
        if skip > 0 and noise_t > skip:
            noise_t = noise_t - skip
        t_model.append(t)
        t_post.append(noise_t)
        prev = t
    return t_model, t_post


class HipMaskAndReplaceDiffusion:
    """MI355X implementation behind the reference's Seam-2."""

    def __init__(self, *, n_category: int, n_bin: int = 32, max_elem: int = 25, n_attr: int = 5,
                 d_model: int = 464, n_head: int = 8, d_ff: int = 1856, n_layer: int = 4,
                 num_timesteps: int = 100, precision: str = "exact", max_batch: int = 512, chunk: int = 0,
                 device: Optional[int] = None, use_graph: bool = True, q_type: str = "constrained", lanes: int = 0,
                 verifier: str = "split", auxiliary_loss_weight: float = 1e-1, pos_emb: str = "elem_attr",
                 timestep_type: Optional[str] = "adalayernorm"):
        # q_type: Q_TYPES of models/layoutdm.py:20-23 — "constrained" (constrained.py) or "vanilla" (vanilla.py)
        # precision / verifier: selection.py — an engine's name, "<name>_verified", or "auto": load_state_dict measures the fp16
        # engine on the checkpoint and selects
        # pos_emb / timestep_type: the denoiser variants of the reference's constructor (nn_lib.py:73-127, transformer_utils.py:124-156).
        # The library reads pos_emb, the *_abs sinusoid and timestep_type None from the checkpoint's key set and serves them on every
        # engine; the two adainnorm kinds (instance norm over a layout's rows: the state dict does not tell them from adalayernorm)
        # reach ldm_create_variant and run on the reference-precision engines only — auto then IS its verifier engine
        if pos_emb not in POS_EMBS:
            raise NotImplementedError(f"pos_emb={pos_emb}: one of {sorted(POS_EMBS)}")
        check_timestep_type(timestep_type)
        self.pos_emb, self.timestep_type = pos_emb, timestep_type
        self.instance_norm = timestep_type in INSTANCE_NORM_TYPES
        self.wide_vocab = n_category + 4 * n_bin + 2 > FP16_MAX_CLASSES
        self.precision = precision
        self.auto = precision == "auto"
        self.auto_tolerance = 1e-3
        self.verifier_tolerance = 5e-4     # split vs a small fp32-MFMA probe engine: half the north star's tolerance (two valid fp32-level
                                           # engines differ by 4.2e-4 on the "wide" point, where the reference's own f32 noise floor is 1.2e-4)

        def mk(prec, mb=max_batch):
            return Engine(n_category=n_category, n_bin=n_bin, max_elem=max_elem, n_attr=n_attr, d_model=d_model, n_head=n_head,
                          d_ff=d_ff, n_layer=n_layer, n_step=num_timesteps, precision=prec, max_batch=mb, chunk=chunk,
                          device=device, q_type=q_type, lanes=lanes, timestep_type=timestep_type)

        self._selector = sel = Selector(mk, precision, verifier, self.auto_tolerance, self.verifier_tolerance, self.wide_vocab,
                                        timestep_type if self.instance_norm else None)
        # which engine runs: load_state_dict alone changes these, from what the selector returns
        self.engine, self.verified = sel.primary, sel.v_fast
        self.selected_precision, self.verifier = sel.selected, verifier
        self._v_fast, self._v_rung = sel.v_fast, sel.v_rung    # the fp16 pair (or None) and the pairs of the rungs auto has built so far
        self.verifier_check: Dict[str, object] = {}
        self.selection_report: Dict[str, object] = {}
        self.q_type = q_type
        self.num_timesteps = num_timesteps
        self.num_classes = self.engine.C
        self.max_token_length = self.engine.S
        self.use_graph = use_graph
        self.mask_id = self.engine.mask_id
        self.pad_id = self.engine.pad_id
        # held-out loss (loss / evaluate): base.py:43,99,106-107.  The two history buffers of the checkpoint stay on the host
        # (time_weights reads them; nothing here writes them)
        self.auxiliary_loss_weight = float(auxiliary_loss_weight)
        self.adaptive_auxiliary_loss = True
        self.Lt_history: Optional[torch.Tensor] = None
        self.Lt_count: Optional[torch.Tensor] = None

    RUNGS = RUNGS

    # -- nn.Module-ish surface used by the reference's callers --------------------------------
    @property
    def device(self) -> torch.device:
        return self.engine.device

    def to(self, *_a, **_k):
        return self

    def eval(self):
        return self

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        for k, v in state_dict.items():                         # (keys with or without 'model.module.')
            if k.rsplit(".", 1)[-1] in ("Lt_history", "Lt_count"):
                setattr(self, k.rsplit(".", 1)[-1], torch.as_tensor(v).detach().to("cpu", torch.float32).reshape(-1).clone())
        selector = getattr(self, "_selector", None)
        if selector is None:                                    # (the host half alone, without engines: the history is all it loads)
            return self
        sel = selector.load(state_dict)
        self.engine, self.verified, self.selected_precision = sel.engine, sel.verified, sel.selected
        self.verifier, self.verifier_check = sel.verifier, sel.verifier_check
        self.selection_report = selection_report(sel, variant_name(self.pos_emb, self.timestep_type))
        logger.info(selection_message(sel))   # one INFO record per loaded checkpoint: which engine runs, and why
        return self

    def close(self) -> None:
        """Release every engine this object built (the handles own GBs of workspace)."""
        self._selector.close()

    @property
    def calibration(self) -> Dict[str, float]:
        """fp16-engine-vs-verifier logits error measured at load time (precision fast_verified / auto; mixed_verified: the mixed
        engine's), else {}."""
        return dict(self._v_fast.calibration) if self._v_fast is not None else {}

    # -- the hot path ----------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, batch_size: Optional[int] = 1, cond: Optional[Dict] = None, sampling_cfg=None,
               get_intermediate_results: bool = False, seed: Optional[int] = None, first_layout: int = 0,
               return_device_tensor: bool = False, **kwargs) -> Union[torch.Tensor, List[torch.Tensor]]:
        """BaseMaskAndReplaceDiffusion.sample (base.py:293-371).  Extra keyword arguments
        (`cond_type=...` from test.py:195-200) are accepted and ignored like the reference does.

        seed: Philox key for the stochastic samplers.  None -> drawn from torch's global CPU
        generator, so `set_seed()` (helpers/util.py:10-13) keeps runs reproducible.
        first_layout: global index of row 0 (batch sharding across calls / GPUs)."""
        eng = self.engine
        if cond and cond.get("type") == "relation":
            raise NotImplementedError(
                "cond=relation needs the relation graph (cond['batch_w_canvas']) turned into the kernel's CSR form: use "
                "layout_dm_amd.relation.sample_with_relation, which LayoutDM.sample does (the logit adjustment of "
                "logit_adjustment.py:88-126 then runs inside ldm_sample_loop)")
        t_model, t_post, seed = schedule_and_seed(self.num_timesteps, sampling_cfg, seed)
        B = int(batch_size)
        if B == 0:  # an empty shard (distributed.shard_range with fewer layouts than ranks)
            empty = torch.empty((0, eng.S), dtype=torch.int32, device=eng.device)
            if get_intermediate_results:
                return [empty.long().cpu() for _ in t_model]
            return empty if return_device_tensor else empty.long().cpu()
        if cond:
            seq = torch.as_tensor(cond["seq"])
            if seq.size(0) == 1 and B > 1:  # duplicate_cond, helpers/task.py:235-248
                cond = dict(cond)
                for k, v in list(cond.items()):
                    # only what still has the single-layout batch dimension (a caller may hand over tensors that
                    # are already per-sample, e.g. a (B,C,S) refinement prior)
                    if isinstance(v, torch.Tensor) and v.dim() > 0 and v.size(0) == 1:
                        cond[k] = v.repeat([B] + [1] * (v.dim() - 1))
                seq = cond["seq"]
            assert seq.size(0) == B, "cond['seq'] batch does not match batch_size"
            tokens = seq.to(device=eng.device, dtype=torch.int32).contiguous().clone()
        else:
            tokens = torch.full((B, eng.S), eng.mask_id, dtype=torch.int32, device=eng.device)
        outs, inters = [], []
        off = 0
        for n in batch_cuts(B, eng.max_batch, eng.batch_round):  # the reference caps a call at 512 (Converter); we cut
            sub = None
            if cond:
                sub = {k: (v[off:off + n] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.size(0) == B else v)
                       for k, v in cond.items()}
            if (self.verified is not None and self.engine is self.verified.fast
                    and _cfg_get(sampling_cfg, "name") == "deterministic"):
                tk, inter = self.verified.sample_loop(tokens[off:off + n].contiguous(), t_model, t_post, cond=sub,
                                                      intermediates=get_intermediate_results)
            else:
                tk, inter = eng.sample_loop(tokens[off:off + n].contiguous(), t_model, t_post, sampling_cfg, cond=sub,
                                            seed=seed, first_layout=first_layout + off,
                                            intermediates=get_intermediate_results, use_graph=self.use_graph)
            outs.append(tk)
            inters.append(inter)
            off += n
        out = torch.cat(outs) if len(outs) > 1 else outs[0]
        if get_intermediate_results:
            inter = torch.cat(inters, dim=1) if len(inters) > 1 else inters[0]
            return [x.long().cpu() for x in inter]
        if return_device_tensor:
            return out
        return out.long().cpu()

    # -- scoring given layouts: forward() as evaluation (constrained.py:232-333, vanilla.py:160-240) --------------------
    def _draw_seed(self, seed: Optional[int]) -> int:
        return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)

    def _cut(self, B: int):
        eng, off = self.engine, 0
        for n in batch_cuts(B, eng.max_batch, eng.batch_round):
            yield off, n
            off += n

    def time_weights(self) -> torch.Tensor:
        """pt_all of sample_time("importance") (base.py:179-198): (T,) float32 on the host from the checkpoint's Lt_history /
        Lt_count, or 1 / T everywhere while some timestep has been visited 10 times or fewer (or the checkpoint has no history)."""
        T = self.num_timesteps
        if not self._has_history():
            return torch.from_numpy(np.full(T, np.float32(1) / np.float32(T), np.float32))
        # float32 like the reference's buffers: weight of t = sqrt(running mean of L_t^2), floored; t = 0 (the decoder term,
        # on another scale than the kl terms) is sampled as often as t = 1; normalised to probabilities
        w = np.sqrt(self.Lt_history.numpy().astype(np.float32) + np.float32(1e-10)) + np.float32(1e-4)
        w[0] = w[1]
        return torch.from_numpy(w / w.sum(dtype=np.float32))

    def _has_history(self) -> bool:
        """every timestep visited more than 10 times during training (base.py:181), so that Lt_history means something"""
        return self.Lt_history is not None and self.Lt_count is not None and bool((self.Lt_count.numpy() > 10).all())

    def sample_time(self, b: int):
        """(t (b,) int64, pt (b,) float32) on the host like base.py:179-198 draws them (torch's global CPU generator)."""
        pt_all = self.time_weights()
        if not self._has_history():
            t = torch.randint(0, self.num_timesteps, (b,)).long()
        else:
            t = torch.multinomial(pt_all, num_samples=b, replacement=True)
        return t, pt_all.gather(0, t)

    @torch.no_grad()
    def q_sample(self, x0: torch.Tensor, t: int, seed: int = 0, first_layout: int = 0) -> torch.Tensor:
        """x_t ~ q(x_t | x_0) for the whole batch at one t (Engine.q_sample), (B,S) int32 on the device."""
        eng = self.engine
        x0 = eng._tok(torch.as_tensor(x0))
        parts = [eng.q_sample(x0[off:off + n], t, seed, first_layout + off) for off, n in self._cut(x0.shape[0])]
        return torch.cat(parts) if len(parts) > 1 else parts[0]

    @torch.no_grad()
    def vb_terms(self, x0: torch.Tensor, t: int, x_t: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                 first_layout: int = 0) -> Dict[str, torch.Tensor]:
        """The variational bound's terms of ONE timestep for given layouts x0 (B,S): per-layout float64 tensors on the device,
        every value a mean over the layout's S tokens (mean_except_batch) —
            kl           KL(q(x_{t-1} | x_t, x_0) || p_theta(x_{t-1} | x_t))       constrained.py:289-299
            decoder_nll  -log p_theta(x_0 | x_t)                                   constrained.py:301-302
            kl_aux       KL(x_0 || p_theta(x_0 | x_t)) over the non-[MASK] classes   constrained.py:317-321
            x0_acc       share of tokens whose most likely x_0 is the true one     constrained.py:269-277
        x_t: the noised state to score at, or None: drawn, x_t ~ q(x_t | x_0), with a Philox stream keyed by (seed,
        first_layout + b, t, position) — not the reference's Gumbel-argmax stream on torch's generator, which cannot be
        reproduced; seed None draws the key from torch's global CPU generator.  Evaluation only: no gradient exists."""
        eng = self.engine
        x0 = eng._tok(torch.as_tensor(x0))
        if x_t is not None:
            x_t = eng._tok(torch.as_tensor(x_t))
            assert x_t.shape == x0.shape
        seed = 0 if x_t is not None else self._draw_seed(seed)
        sums = torch.empty((x0.shape[0], 4), dtype=torch.float64, device=eng.device)
        self._vb_sums(x0, t, x_t, seed, first_layout, sums)
        mean = sums / eng.S                                     # the 1 / S of mean_except_batch (one elementwise launch)
        return {"kl": mean[:, 0], "decoder_nll": mean[:, 1], "kl_aux": mean[:, 2], "x0_acc": mean[:, 3]}

    def _vb_sums(self, x0, t, x_t, seed, first_layout, out) -> None:
        """Engine.vb_step of a staged (B,S) int32 device batch, cut by batch_cuts, into out (B,4) float64 on the device."""
        eng = self.engine
        for off, n in self._cut(x0.shape[0]):
            eng.vb_step(x0[off:off + n], t, xt=None if x_t is None else x_t[off:off + n], seed=seed,
                        first_layout=first_layout + off, out=out[off:off + n])

    @torch.no_grad()
    def elbo(self, x0: torch.Tensor, n_draws: int = 1, seed: Optional[int] = None, first_layout: int = 0) -> torch.Tensor:
        """Per-layout variational bound on -log p(x_0) in nats per token, (B,) float64 on the device: the sum over t = 0 .. T - 1
        of the reference's kl_loss term (constrained.py:304-305: decoder_nll at t = 0, kl otherwise) at one drawn x_t per t,
        averaged over n_draws independent draws (Philox keys seed, seed + 1, ...).  On an engine with per-layout timesteps
        (Engine.per_layout_t) the T * B (t, layout) pairs of a draw are packed t-major into calls of up to max_batch rows
        (elbo_calls): ceil(T * B / max_batch) denoiser passes per draw — 1 at B = 4, T = 100, max_batch = 512 — each row with the
        bits its single-t call gives it; a call whose rows share one t (every call when B is a multiple of max_batch) is the
        single-t call itself.  Elsewhere the whole batch goes through each t: T passes per draw.  The reference's bound carries no prior term L_T = KL(q(x_T | x_0) || p(x_T)), so neither
        does this one (L_T does not depend on the model: it shifts every checkpoint's bound alike).  A stochastic estimate: compare checkpoints or layouts under the same seed."""
        if n_draws < 1:
            raise ValueError("n_draws must be >= 1")
        seed = self._draw_seed(seed)
        eng, T = self.engine, self.num_timesteps
        x0 = eng._tok(torch.as_tensor(x0))                       # staged once for all T passes
        sums = torch.empty((int(n_draws) * T, x0.shape[0], 4), dtype=torch.float64, device=eng.device)
        B = x0.shape[0]
        if B and eng.per_layout_t:
            # x0 tiled so that the rows of any call — layouts (start + k) % B, k = 0 .. n - 1 — are one contiguous slice of it
            reps = -(-(B - 1 + min(eng.max_batch, T * B)) // B)
            tiled = x0.repeat(reps, 1) if reps > 1 else x0
            for c in elbo_calls(B, T, int(n_draws), eng.max_batch):
                n, b0 = len(c.t), int(c.layout[0])
                out = sums[c.draw * T:(c.draw + 1) * T].view(T * B, 4)[c.start:c.start + n]   # (t-major: the call's rows are contiguous)
                if int(c.t[0]) == int(c.t[-1]):
                    eng.vb_step(tiled[b0:b0 + n], int(c.t[0]), seed=seed + c.draw, first_layout=first_layout + b0, out=out)
                else:
                    eng.vb_step_t(tiled[b0:b0 + n], c.t, seed=seed + c.draw, first_layout=first_layout, layout=c.layout, out=out)
        else:
            for d in range(int(n_draws)):
                for t in range(T):
                    self._vb_sums(x0, t, None, seed + d, first_layout, sums[d * T + t])
        # one elementwise launch for the token means (the values vb_terms returns), then the T terms of a draw are added on
        # the host in their order, t = 0 first: B x T float64 additions, exactly the sum of the vb_terms calls
        mean = (sums / eng.S).cpu().numpy()
        total = np.zeros(x0.shape[0])
        for i in range(mean.shape[0]):
            total = total + mean[i, :, 1 if i % T == 0 else 0]
        if n_draws > 1:
            total = total / int(n_draws)
        return torch.from_numpy(total).to(eng.device)

    @torch.no_grad()
    def loss(self, x0: torch.Tensor, t: Optional[torch.Tensor] = None, pt: Optional[torch.Tensor] = None,
             seed: Optional[int] = None, x_t: Optional[torch.Tensor] = None, first_layout: int = 0,
             grouped: bool = False) -> Dict[str, torch.Tensor]:
        """The reference's losses of one batch, {"kl_loss", "aux_loss"} (constrained.py:304-330 with adaptive_auxiliary_loss; no
        "aux_loss" when auxiliary_loss_weight is 0), as float64 scalars on the host.  t (B,) per-layout timesteps and pt their
        sampling probabilities: None -> sample_time() / time_weights()[t].  x_t: given states (B,S), else drawn per layout at
        its own t (vb_terms' stream: a layout's draw depends on seed, its global index and its t alone).
        Cost: on an engine with per-layout timesteps (Engine.per_layout_t: every engine but `fast` on the reference's backbone)
        the batch is ONE Engine.vb_step_t call per batch_cuts window — the draw, one denoiser pass per chunk with every layout
        at its own t, the terms and one error-word read-back: a batch of 64 is one call whatever its t.  Elsewhere, and with
        grouped=True (the earlier path, kept for comparison: same bits), layouts are grouped by t on the host, one denoiser
        pass per distinct value; ldm_q_sample takes ONE t per call, so with drawn x_t the whole batch is noised once per
        distinct t and the group picked out of it (a batch of 64 at ~45 distinct t: 45 small draw launches and 45 vb_step
        calls, each with its error-word read-back)."""
        eng = self.engine
        x0 = eng._tok(torch.as_tensor(x0))
        B, T = x0.shape[0], self.num_timesteps
        if t is None:
            t, pt_drawn = self.sample_time(B)
            pt = pt_drawn if pt is None else pt
        t = torch.as_tensor(t).to("cpu", torch.int64).reshape(-1)
        if t.numel() != B or int(t.min()) < 0 or int(t.max()) >= T:
            raise ValueError(f"t must be ({B},) timesteps in [0, {T})")
        pt = self.time_weights().gather(0, t) if pt is None else torch.as_tensor(pt).to("cpu").reshape(-1)
        if x_t is not None:
            x_t = eng._tok(torch.as_tensor(x_t))
        seed = 0 if x_t is not None else self._draw_seed(seed)
        if not grouped and eng.per_layout_t:
            part = torch.empty((B, 4), dtype=torch.float64, device=eng.device)
            tn32 = t.numpy().astype(np.int32)
            for off, n in self._cut(B):
                eng.vb_step_t(x0[off:off + n], tn32[off:off + n], xt=None if x_t is None else x_t[off:off + n], seed=seed,
                              first_layout=first_layout + off, out=part[off:off + n])
            sums = part.cpu()
        else:
            sums = torch.empty((B, 4), dtype=torch.float64)
            for tv in sorted(set(t.tolist())):
                idx = (t == tv).nonzero().reshape(-1)
                idx_d = idx.to(eng.device)
                xt_all = x_t if x_t is not None else self.q_sample(x0, tv, seed, first_layout)
                x0_g, xt_g = x0.index_select(0, idx_d), xt_all.index_select(0, idx_d)
                part = torch.empty((idx.numel(), 4), dtype=torch.float64, device=eng.device)
                for off, n in self._cut(idx.numel()):
                    eng.vb_step(x0_g[off:off + n], tv, xt=xt_g[off:off + n], out=part[off:off + n])
                sums[idx] = part.cpu()
        # B scalars from here on, on the host in float64
        mean = sums.numpy() / eng.S
        tn, ptn = t.numpy(), pt.double().numpy()
        first = tn == 0
        kl_loss = np.where(first, mean[:, 1], mean[:, 0])                                # constrained.py:304-305
        out = {"kl_loss": torch.tensor(float((kl_loss / ptn).mean()), dtype=torch.float64)}
        if self.auxiliary_loss_weight != 0:
            kl_aux_loss = np.where(first, mean[:, 1], mean[:, 2])                        # l.322
            w = (1 - tn / T) + 1.0 if self.adaptive_auxiliary_loss else 1.0              # l.323-326
            out["aux_loss"] = torch.tensor(float((w * self.auxiliary_loss_weight * kl_aux_loss / ptn).mean()), dtype=torch.float64)
        return out
