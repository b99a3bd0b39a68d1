"""Drop-in replacement for the reference's model class on the sampling path.

    config.yaml:   model: {_target_: layout_dm_amd.layoutdm.LayoutDM, _partial_: true, q_type: constrained}

Mirrors trainer/models/layoutdm.py:26-126 (LayoutDM) + trainer/models/base_model.py:124-150
(aggregate_sampling_settings) for everything the `test` entry point touches
(trainer/test.py:113-118,144-150,195-228): constructor signature, `.to()`, `.eval()`,
`.load_state_dict()` with the checkpoint's `model.module.*` keys, `.tokenizer`,
`.aggregate_sampling_settings()`, `.sample()` -> {"bbox","label","mask"} via the caller's own
tokenizer, and `.model.sample()` (notebooks/demo.ipynb) -> LongTensor tokens.
Training (`forward`, losses, optimizer groups) is out of scope and raises.

The tokenizer is the reference's own `LayoutSequenceTokenizer` object (or anything duck-typing its
properties): host-side encode/decode is reused as is, only the T-step reverse
loop runs in libldm_hip.so.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .diffusion import POS_EMBS, HipMaskAndReplaceDiffusion, _cfg_get, check_timestep_type


def _find(cfg, key):
    """get_dim_model-style recursive lookup (trainer/models/common/util.py:21-33)."""
    result = None
    items = cfg.items() if hasattr(cfg, "items") else []
    for k, v in items:
        if k == key:
            result = v
        elif hasattr(v, "items"):
            x = _find(v, key)
            if x:
                result = x
    return result


# ---- pure host logic (no GPU, no handle): unit-tested on the CPU against the reference's own objects -----------
def aggregate_sampling_settings(tokenizer, sampling_cfg, args):
    """base_model.py:124-150 + layoutdm.py:90-97: fold the test-time CLI args into sampling_cfg."""
    if args.cond == "refinement" and args.refine_lambda > 0.0:
        sampling_cfg.refine_mode = args.refine_mode
        sampling_cfg.refine_offset_ratio = args.refine_offset_ratio
        sampling_cfg.refine_lambda = args.refine_lambda
    if args.cond == "relation" and args.relation_lambda > 0.0:
        sampling_cfg.relation_mode = args.relation_mode
        sampling_cfg.relation_lambda = args.relation_lambda
        sampling_cfg.relation_tau = args.relation_tau
        sampling_cfg.relation_num_update = args.relation_num_update
    if "num_timesteps" not in sampling_cfg:
        if "eos" in tokenizer.special_tokens:
            sampling_cfg.num_timesteps = tokenizer.max_token_length
        else:
            sampling_cfg.num_timesteps = args.num_timesteps
    if args.time_difference > 0:
        sampling_cfg.time_difference = args.time_difference
    return sampling_cfg


def refinement_prior_table(tokenizer, mode: str, ratio: float) -> torch.Tensor:
    """The (C,C) [token, class] table of `_index_to_smoothed_log_onehot` (helpers/task.py:154-201) before the
    refine_lambda weight: identity outside the bbox sub-vocabularies, a neighbourhood indicator (uniform / negative)
    or a negative squared distance (gaussian) between cluster centres inside each of them."""
    C, N = tokenizer.N_total, tokenizer.N_bbox_per_var
    bbt = tokenizer.bbox_tokenizer
    table = torch.zeros((C, C))
    table.fill_diagonal_(1.0)
    shared = bbt.shared_bbox_vocab == "xywh"
    for i, k in enumerate(bbt.var_names):
        sl = slice(tokenizer.N_category, tokenizer.N_category + N) if shared else \
            slice(tokenizer.N_category + i * N, tokenizer.N_category + (i + 1) * N)
        centers = torch.from_numpy(bbt.clustering_models[f"{k}-{N}"].cluster_centers_).view(-1)
        ii, jj = torch.meshgrid(centers, centers, indexing="ij")
        if mode == "uniform":
            table[sl, sl] = (torch.abs(ii - jj) < ratio).float()
        elif mode == "negative":
            table[sl, sl] = (torch.abs(ii - jj) >= ratio).float()
        elif mode == "gaussian":
            table[sl, sl] = -1.0 * (ii - jj) ** 2
        else:
            raise NotImplementedError(mode)
    return table.float()


def _refine_settings(sampling_cfg):
    """(mode, ratio, signed weight): refine_lambda, negated for refine_mode="negative" (helpers/task.py:210-214)."""
    mode = _cfg_get(sampling_cfg, "refine_mode", "uniform")
    ratio = float(_cfg_get(sampling_cfg, "refine_offset_ratio", 0.1))
    w = float(_cfg_get(sampling_cfg, "refine_lambda", 3.0))
    if mode == "negative":
        w *= -1.0
    return mode, ratio, w


def _cached_prior_table(tokenizer, mode: str, ratio: float, cache: Optional[dict]) -> torch.Tensor:
    key = (mode, ratio)
    if cache is None or cache.get("key") != key:
        table = refinement_prior_table(tokenizer, mode, ratio)
        if cache is not None:
            cache["key"], cache["table"] = key, table
    else:
        table = cache["table"]
    return table


def refinement_weak_logits(tokenizer, seq_orig: torch.Tensor, sampling_cfg, cache: Optional[dict] = None):
    """cond["weak_logits"] of set_additional_conditions_for_refinement (helpers/task.py:204-224): (B,C,S), on the host."""
    mode, ratio, w = _refine_settings(sampling_cfg)
    table = _cached_prior_table(tokenizer, mode, ratio, cache)
    return (table[seq_orig.cpu().long()].permute(0, 2, 1) * w).contiguous()


def refinement_weak_logits_device(tokenizer, seq_orig: torch.Tensor, sampling_cfg, batch_size: int,
                                  cache: Optional[dict] = None, device=None) -> torch.Tensor:
    """The same tensor built on the GPU (binding.refinement_prior, kernels_refine.hip), bit for bit: (batch_size,C,S) float32
    on the device.  seq_orig is taken from wherever it lives — a CPU tensor costs the upload of its ids (250 KB at B = 512
    instead of the 40 MB prior), a device tensor no host transfer at all — as (batch_size,S) or, one conditioning layout
    for batch_size samples (duplicate_cond), (1,S).  The (C,C) table of refinement_prior_table is built once on the host
    and its device copy kept in `cache` per (mode, ratio, device); refine_lambda goes to the kernel as its weight.
    device: where to build it (default: seq_orig's GPU, else the current one).  No CPU path."""
    from . import binding

    if not torch.cuda.is_available():
        raise RuntimeError("layout_dm_amd.layoutdm.refinement_weak_logits_device needs a ROCm GPU (MI355X); there is no CPU path")
    mode, ratio, w = _refine_settings(sampling_cfg)
    seq_orig = torch.as_tensor(seq_orig)
    if device is None:
        device = seq_orig.device if seq_orig.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    key = ("device", mode, ratio, str(device))
    table_dev = cache.get(key) if cache is not None else None
    if table_dev is None:
        table_dev = _cached_prior_table(tokenizer, mode, ratio, cache).to(device).contiguous()
        if cache is not None:
            cache[key] = table_dev
    return binding.refinement_prior(seq_orig, table_dev, w, int(batch_size))


def device_decode_plan(tokenizer):
    """(ok, centres): whether ids -> {bbox,label,mask} can run in kernels_decode.hip for this tokenizer (c-x-y-w-h,
    stacked x-y-w-h bbox vocabulary, no bos/eos) and the (4,n_bin) float64 cluster centres for kmeans / percentile
    quantisation (None for linear bins, whose decode is closed-form: bbox_tokenizer.py:117-168)."""
    try:
        bbt = tokenizer.bbox_tokenizer
        special = list(tokenizer.special_tokens)
        ok = ("bos" not in special and "eos" not in special and list(tokenizer.var_names) == ["c", "x", "y", "w", "h"]
              and bbt.shared_bbox_vocab == "x-y-w-h" and list(bbt.var_names) == ["x", "y", "w", "h"]
              and list(getattr(bbt, "_var_order", ["x", "y", "w", "h"])) == ["x", "y", "w", "h"])
        if ok and bbt.bbox_quantization == "linear":
            return True, None
        if ok and bbt.bbox_quantization in ("kmeans", "percentile"):
            import numpy as np

            N = tokenizer.N_bbox_per_var
            cs = [np.asarray(bbt.clustering_models[f"{k}-{N}"].cluster_centers_, dtype=np.float64).reshape(-1)
                  for k in ("x", "y", "w", "h")]
            if all(c.shape == (N,) for c in cs):
                return True, torch.from_numpy(np.stack(cs))
    except AttributeError:
        pass
    return False, None


class _ModuleShim:
    """Gives `model.model.module` / `model.model.sample` the shapes the reference exposes through
    CustomDataParallel (models/common/nn_lib.py:17-23)."""

    def __init__(self, inner: HipMaskAndReplaceDiffusion, owner: "LayoutDM"):
        self.module = inner
        self._owner = owner

    def sample(self, *a, **k):
        return self._owner._sample_tokens(*a, **k)

    def __getattr__(self, name):
        return getattr(self.module, name)


class LayoutDM:
    def __init__(self, backbone_cfg, tokenizer, transformer_type: str = "flattened", pos_emb: str = "elem_attr",
                 num_timesteps: int = 100, auxiliary_loss_weight: float = 1e-1, q_type: str = "single",
                 seq_type: str = "poset", precision: str = "auto", max_batch: int = 512, device: Optional[int] = None,
                 **kwargs) -> None:
        # precision (not a reference argument): "auto" (default, r05) = the fp16 engine is measured against the
        # reference-precision engine on the loaded checkpoint and kept — with verified greedy decoding — only inside the
        # north star's 1e-3 logits tolerance, else the hybrid engine (mixed with the FFN / head in plain fp16), else the mixed engine (hi + lo
        # activations x fp16 weights) under the same test, else the reference-precision engine; "fast" / "fast_verified" / "hybrid" /
        # "hybrid_verified" / "mixed" / "mixed_verified" / "split" / "exact" pick an engine unconditionally
        if q_type not in ("constrained", "vanilla"):  # Q_TYPES, layoutdm.py:20-23
            raise NotImplementedError(f"q_type={q_type}: constrained (LayoutDM default, experiment/layoutdm.yaml:18) "
                                      "or vanilla")
        if transformer_type == "aggregated":
            raise NotImplementedError(
                "transformer_type=aggregated: not supported, and the reference cannot instantiate it either — base.py:85-93 calls "
                "CategoricalAggregatedTransformer with arguments its constructor (nn_lib.py:408-415) does not take")
        if transformer_type != "flattened":
            raise NotImplementedError(f"transformer_type={transformer_type}: only flattened")
        if pos_emb not in POS_EMBS:  # base.py:70-84
            raise NotImplementedError(f"pos_emb={pos_emb}: elem_attr (LayoutDM default) or default (experiment/vqdiffusion.yaml)")
        assert seq_type in ["set", "poset"]
        # make sure MASK is the last vocabulary (layoutdm.py:46)
        assert tokenizer.id_to_name(tokenizer.N_total - 1) == "mask"
        assert list(tokenizer.var_names) == ["c", "x", "y", "w", "h"], "var_order must be c-x-y-w-h"
        self.tokenizer = tokenizer
        self.pos_emb, self.seq_type = pos_emb, seq_type
        mult = 29 / 32  # shrink(backbone_cfg, 29/32), layoutdm.py:54 + common/util.py:36-44
        d_model = int(mult * _find(backbone_cfg, "d_model"))
        d_ff = int(mult * _find(backbone_cfg, "dim_feedforward"))
        n_head = int(_find(backbone_cfg, "nhead"))
        n_layer = int(_find(backbone_cfg, "num_layers"))
        ttype = _find(backbone_cfg, "timestep_type")
        check_timestep_type(ttype)  # Block, transformer_utils.py:124-156: the *_mlp kinds stay refused
        dstep = int(_find(backbone_cfg, "diffusion_step") or num_timesteps)
        assert dstep == num_timesteps
        inner = HipMaskAndReplaceDiffusion(
            n_category=tokenizer.N_category, n_bin=tokenizer.N_bbox_per_var, max_elem=tokenizer.max_seq_length,
            n_attr=tokenizer.N_var_per_element, d_model=d_model, n_head=n_head, d_ff=d_ff, n_layer=n_layer,
            num_timesteps=num_timesteps, precision=precision, max_batch=max_batch, device=device, q_type=q_type,
            auxiliary_loss_weight=auxiliary_loss_weight, pos_emb=pos_emb, timestep_type=ttype)
        assert inner.num_classes == tokenizer.N_total and inner.max_token_length == tokenizer.max_token_length
        self.model = _ModuleShim(inner, self)
        self._refine_table = None
        # inside the reference's own test.py main() (class swapped by layout_dm_amd.test_entry) on a GPU: its per-batch
        # cond=relation score runs on the device too
        from .reference_hooks import install_violation_dropin

        install_violation_dropin(type(self))

    # ---- nn.Module-ish surface ------------------------------------------------------------------
    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("layout_dm_amd accelerates sampling only; train with the reference")
        return self

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        self.model.module.load_state_dict(state_dict)
        return self

    def forward(self, *a, **k):
        raise NotImplementedError("training forward is out of scope (SURVEY §2.1 #10)")

    __call__ = forward

    # ---- held-out layouts: the variational bound and main.evaluate's loss (no gradients) --------------------------------
    def _seq_of(self, seq_or_layouts) -> torch.Tensor:
        if isinstance(seq_or_layouts, dict):
            if "seq" in seq_or_layouts:
                return torch.as_tensor(seq_or_layouts["seq"])
            return self.encode(seq_or_layouts)["seq"]     # raw {"bbox", "label", "mask"}: tokenizer.encode on the GPU
        return torch.as_tensor(seq_or_layouts)

    def score(self, seq_or_layouts, n_draws: int = 1, seed: Optional[int] = None, first_layout: int = 0) -> torch.Tensor:
        """Per-layout variational bound on -log p(layout) in nats per token, (B,) float64 on the device
        (HipMaskAndReplaceDiffusion.elbo: sum over t of the reference's kl_loss term at one drawn x_t per t; no prior term
        L_T, like the reference's bound).  seq_or_layouts: (B,S) ids, {"seq": ids} or raw {"bbox", "label", "mask"}.
        Lower is better explained; the same seed makes two checkpoints (or two candidate layouts) comparable."""
        return self.model.module.elbo(self._seq_of(seq_or_layouts), n_draws=n_draws, seed=seed, first_layout=first_layout)

    def evaluate_loss(self, seq_or_layouts, batch_size: int = 64, seed: Optional[int] = None) -> float:
        """main.evaluate (trainer/main.py:271-294) on held-out layouts: the mean over batches of kl_loss + aux_loss — the
        number that picks best_model.pt and is written to result.json as test_loss.  It INCLUDES the auxiliary term:
        LayoutDM.forward calls the diffusion with is_train=True even under evaluate().  One t per layout per batch
        (sample_time on torch's global CPU generator, like the reference), x_t from the Philox stream keyed by
        (seed, index of the layout in `seq`, t, position).  forward() itself stays unavailable: there is no gradient."""
        seq = self._seq_of(seq_or_layouts)
        inner = self.model.module
        seed = inner._draw_seed(seed)
        total, steps = 0.0, 0
        for off in range(0, seq.shape[0], int(batch_size)):
            losses = inner.loss(seq[off:off + int(batch_size)], seed=seed, first_layout=off)
            total += float(sum(v.item() for v in losses.values()))
            steps += 1
        if steps == 0:
            raise ValueError("evaluate_loss: no layouts")
        return total / steps

    # ---- base_model.py:124-150 + layoutdm.py:90-97 -------------------------------------------------
    def aggregate_sampling_settings(self, sampling_cfg, args):
        return aggregate_sampling_settings(self.tokenizer, sampling_cfg, args)

    # ---- refinement prior: helpers/task.py:154-224 --------------------------------------------------
    def _weak_logits(self, seq_orig: torch.Tensor, sampling_cfg) -> torch.Tensor:
        if self._refine_table is None:
            self._refine_table = {}
        return refinement_weak_logits(self.tokenizer, seq_orig, sampling_cfg, self._refine_table)

    # ---- sampling --------------------------------------------------------------------------------
    def _sample_tokens(self, batch_size: Optional[int] = 1, cond: Optional[Dict] = None, sampling_cfg=None,
                       get_intermediate_results: bool = False, **kwargs):
        inner = self.model.module
        if cond:
            cond = dict(cond)  # the reference mutates the caller's dict (base.py:328-336); we do not
            ctype = cond.get("type", None)
            if ctype == "refinement" and "weak_logits" not in cond:
                # set_additional_conditions_for_refinement (helpers/task.py:204-224) runs on the cond as given —
                # (1,S) for a single conditioning layout — and duplicate_cond repeats the result once, in sample()
                # — here as the kernel's broadcast form: (1,S) ids -> (batch_size,C,S), built on the device (kernels_refine.hip)
                if self._refine_table is None:
                    self._refine_table = {}
                seq_orig = torch.as_tensor(cond["seq_orig"])
                if inner.engine.device.type == "cuda":
                    cond["weak_logits"] = refinement_weak_logits_device(
                        self.tokenizer, seq_orig, sampling_cfg, int(batch_size) if seq_orig.size(0) == 1 else seq_orig.size(0),
                        self._refine_table, device=inner.engine.device)
                else:
                    # the prior lives where the engine does.  binding.Engine exists on a GPU only (it raises without one), so this
                    # is a stand-in engine on the host: tests/test_entry_reference_main.py drives the plumbing above the C-ABI so
                    cond["weak_logits"] = self._weak_logits(seq_orig, sampling_cfg)
            if ctype == "relation":
                from .relation import sample_with_relation

                return sample_with_relation(inner, batch_size, cond, sampling_cfg, self.tokenizer,
                                            get_intermediate_results=get_intermediate_results, **kwargs)
        return inner.sample(batch_size=batch_size, cond=cond, sampling_cfg=sampling_cfg,
                            get_intermediate_results=get_intermediate_results, **kwargs)

    # ---- raw layouts in: layout_dm_amd/task.py -------------------------------------------------------------
    def encode(self, layouts: Dict) -> Dict[str, torch.Tensor]:
        """tokenizer.encode of {"bbox", "label", "mask"} on the GPU (task.encode): {"seq" int64, "mask" bool}."""
        from . import task

        return task.encode(self.tokenizer, layouts["bbox"], layouts["label"], layouts["mask"])

    def sample_from_layouts(self, layouts: Dict, cond_type: str, sampling_cfg=None, *, keep=None, noise=None, selection=None,
                            edge_ratio: float = 0.1, cond_seed: Optional[int] = None, first_layout: int = 0, **kwargs):
        """get_cond (task.get_cond, kernels_cond.hip) -> refinement prior -> sampling -> decode, the tokens staying on the
        device: `sample(batch_size=B, cond=task.get_cond(layouts, ...), ...)` with the layouts moved to the GPU first.
        cond_seed keys the builder's own draws; every other keyword (seed, ...) goes to sample()."""
        from . import task

        dev = self.model.module.engine.device
        on_dev = {k: torch.as_tensor(layouts[k]).to(dev) for k in ("bbox", "label", "mask")}
        cond = task.get_cond(on_dev, self.tokenizer, cond_type, keep=keep, noise=noise, selection=selection,
                             edge_ratio=edge_ratio, seed=cond_seed, first_layout=first_layout)
        return self.sample(batch_size=on_dev["bbox"].shape[0], cond=cond, sampling_cfg=sampling_cfg, cond_type=cond_type,
                           first_layout=first_layout, **kwargs)

    def _device_decode_centres(self):
        if getattr(self, "_decode_plan", None) is None:
            self._decode_plan = device_decode_plan(self.tokenizer)
        return self._decode_plan

    def sample(self, batch_size: Optional[int] = 1, cond: Optional[Dict] = None, sampling_cfg=None, **kwargs):
        """layoutdm.py:77-88: ids -> tokenizer.decode -> {"bbox","label","mask"} (CPU tensors).  The decode runs on
        the GPU (Engine.decode) when the tokenizer is the LayoutDM one; any other tokenizer configuration falls back
        to the caller's own `tokenizer.decode` on the host, exactly like the reference."""
        kwargs.pop("get_intermediate_results", None)
        ok, centres = self._device_decode_centres()
        if ok:
            ids = self._sample_tokens(batch_size=batch_size, cond=cond, sampling_cfg=sampling_cfg,
                                      return_device_tensor=True, **kwargs)
            out = self.model.module.engine.decode(ids, centres)
            return {k: v.cpu() for k, v in out.items()}
        ids = self._sample_tokens(batch_size=batch_size, cond=cond, sampling_cfg=sampling_cfg, **kwargs).cpu()
        return self.tokenizer.decode(ids)
