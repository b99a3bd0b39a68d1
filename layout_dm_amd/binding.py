"""ctypes binding of libldm_hip.so (include/ldm_hip.h) — the only way Python reaches the HIP path.

PyTorch is used for device memory and streams only: tensors are handed over as raw
`data_ptr()`s together with the current HIP stream handle.  There is no CPU / eager fallback:
if the shared library or a GPU is missing every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libldm_hip.so")
ABI_VERSION = 5

PREC_EXACT_F32, PREC_FAST_F16, PREC_SPLIT_F16, PREC_MIXED_F16, PREC_HYBRID_F16 = 0, 1, 2, 3, 4
PRECISIONS = {"exact": PREC_EXACT_F32, "fast": PREC_FAST_F16, "split": PREC_SPLIT_F16, "mixed": PREC_MIXED_F16, "hybrid": PREC_HYBRID_F16,
              "f32": PREC_EXACT_F32, "f16": PREC_FAST_F16, "f16x3": PREC_SPLIT_F16, "f16x2": PREC_MIXED_F16}
SAMPLERS = {"deterministic": 0, "random": 1, "top_p": 2, "top_k": 3, "gumbel": 4}

EXPORTS = (
    "ldm_create", "ldm_create_variant", "ldm_destroy", "ldm_last_error", "ldm_load_weight", "ldm_finalize_weights",
    "ldm_denoise_logits", "ldm_posterior", "ldm_sample_tokens", "ldm_sample_step", "ldm_sample_loop",
    "ldm_decode_layouts", "ldm_relation_update", "ldm_set_tie_report", "ldm_get_tie_flags",
    "ldm_last_loop_ms", "ldm_set_profiling", "ldm_profile_count", "ldm_profile_get", "ldm_profile_reset",
    "ldm_abi_version", "ldm_get_layout", "ldm_describe", "ldm_dev_step0_flags", "ldm_dev_graph_cache",
    # FID feature extractor (bound in layout_dm_amd/fid.py)
    "ldm_fid_create", "ldm_fid_destroy", "ldm_fid_last_error", "ldm_fid_load_weight", "ldm_fid_finalize",
    "ldm_fid_features", "ldm_prdc", "ldm_layout_metrics",
    # average IoU / DocSim / Max-IoU (bound in layout_dm_amd/metrics.py)
    "ldm_eval_average_iou", "ldm_eval_docsim", "ldm_eval_max_iou_pairs",
    # relation violation score (bound in layout_dm_amd/metrics.py)
    "ldm_relation_violation", "ldm_relation_violation_dense",
    # cond= inputs from raw layouts (bound in layout_dm_amd/task.py)
    "ldm_encode_cond", "ldm_relation_graph",
    # cond=refinement prior (refinement_prior below)
    "ldm_refinement_prior",
    # generated layouts as pictures (bound in layout_dm_amd/visualization.py)
    "ldm_render_layouts", "ldm_render_grid_shape",
    # coordinate bins from raw boxes (bound in layout_dm_amd/clustering.py)
    "ldm_cluster_workspace_bytes", "ldm_cluster_sort", "ldm_kmeans1d_fit", "ldm_kmeans1d_lloyd", "ldm_percentile_fit",
    "ldm_nearest_centre", "ldm_dev_cluster_stages",
    # scoring given layouts (Engine.q_sample / vb_terms / vb_step)
    "ldm_q_sample", "ldm_vb_terms", "ldm_vb_step",
    # ... at a timestep per layout (Engine.denoise_logits_t / q_sample_t / vb_terms_t / vb_step_t)
    "ldm_denoise_logits_t", "ldm_q_sample_t", "ldm_vb_terms_t", "ldm_vb_step_t",
    # the training loss's gradient with respect to the logits (Engine.vb_grad; layout_dm_amd/training.py)
    "ldm_vb_grad",
)


class LdmConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "n_category", "n_bin", "max_elem", "n_attr", "d_model", "n_head", "d_ff",
        "n_layer", "n_step", "precision", "max_batch", "chunk", "q_type", "lanes")]


Q_TYPES = {"constrained": 0, "vanilla": 1}  # models/layoutdm.py:20-23
NORM1_LAYER, NORM1_INSTANCE = 0, 1          # include/ldm_hip.h LDM_NORM1_*
# timestep_type of the backbone's Block (models/transformer_utils.py:124-132) -> the norm1 kind ldm_create_variant takes.  What else a
# variant changes (the *_abs sinusoid, None's plain LayerNorm) the library reads from the checkpoint's key set.
TIMESTEP_TYPES = {"adalayernorm": NORM1_LAYER, "adalayernorm_abs": NORM1_LAYER, None: NORM1_LAYER,
                  "adainnorm": NORM1_INSTANCE, "adainnorm_abs": NORM1_INSTANCE}


class LdmRelation(C.Structure):  # include/ldm_hip.h: ldm_relation
    _fields_ = [("d_edge_offsets", C.c_void_p), ("d_edge_src", C.c_void_p), ("d_edge_dst", C.c_void_p),
                ("d_edge_attr", C.c_void_p), ("d_centres", C.c_void_p), ("canvas_bins", C.c_int32 * 4),
                ("relation_lambda", C.c_float), ("num_update", C.c_int32), ("n_graph_total", C.c_int32)]


class LdmSampler(C.Structure):
    _fields_ = [("kind", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32)]


class LdmCond(C.Structure):
    _fields_ = [("d_cond_seq", C.c_void_p), ("d_strong_mask", C.c_void_p), ("d_weak_logits", C.c_void_p),
                ("pad_disable", C.c_int32)]


_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libldm_hip.so and declare the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("LDM_HIP_LIB") or LIB_PATH  # LDM_HIP_LIB: dev A/B of two builds on one GPU box
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not found: the MI355X HIP extension is not built (run `python -m layout_dm_amd.build` "
            "or __graft_entry__.build()). There is no CPU fallback.")
    if path is None and not os.environ.get("LDM_HIP_LIB"):
        # build provenance: the prebuilt library must come from THIS tree's sources (a snapshot pushed to a GPU box carries both)
        from . import build as _build

        want, have = _build.source_digest(), _build.built_digest(p)
        if have != want:
            #  one builder at a time: under torchrun every rank arrives here at once, and the ranks that wait find the
            # library rebuilt when they get the lock; the link goes to a temporary name and is renamed into place (build.build)
            import fcntl
            import sys

            os.makedirs(os.path.join(os.path.dirname(p), "build"), exist_ok=True)
            with open(os.path.join(os.path.dirname(p), "build", ".lock"), "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    if _build.built_digest(p) != want:
                        print(f"layout_dm_amd: {os.path.basename(p)} is stale against this tree's sources - rebuilding with hipcc "
                              "(a minute or two; python -m layout_dm_amd.build does the same ahead of time)", file=sys.stderr, flush=True)
                        _build.build(verbose=False)
                except Exception as e:  # no hipcc on this machine
                    raise RuntimeError(f"{p} was built from other sources (library {have}, tree {want}) and could not be rebuilt: {e}") from e
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
    lib = C.CDLL(p)
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    lib.ldm_abi_version.restype = C.c_int
    lib.ldm_create.argtypes = [C.POINTER(LdmConfig), i32, C.POINTER(vp)]
    lib.ldm_create_variant.argtypes = [C.POINTER(LdmConfig), i32, i32, C.POINTER(vp)]
    lib.ldm_destroy.argtypes = [vp]
    lib.ldm_destroy.restype = None
    lib.ldm_last_error.argtypes = [vp]
    lib.ldm_last_error.restype = C.c_char_p
    lib.ldm_load_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(C.c_int64), i32]
    lib.ldm_finalize_weights.argtypes = [vp]
    lib.ldm_denoise_logits.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.ldm_posterior.argtypes = [vp, vp, vp, i32, i32, C.POINTER(LdmCond), vp, vp]
    lib.ldm_sample_tokens.argtypes = [vp, vp, C.POINTER(LdmCond), C.POINTER(LdmSampler), u64, u64, i32, i32, vp, vp]
    lib.ldm_sample_step.argtypes = [vp, vp, vp, i32, i32, C.POINTER(LdmCond), C.POINTER(LdmRelation),
                                    C.POINTER(LdmSampler), u64, u64, i32, i32, vp]
    lib.ldm_sample_loop.argtypes = [vp, vp, C.POINTER(LdmCond), C.POINTER(LdmRelation), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), i32, C.POINTER(LdmSampler), u64, u64, i32, vp, i32, vp]
    lib.ldm_decode_layouts.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.ldm_relation_update.argtypes = [vp, vp, vp, C.POINTER(LdmRelation), i32, i32, vp]
    lib.ldm_set_tie_report.argtypes = [vp, C.c_float, C.c_float]
    lib.ldm_get_tie_flags.argtypes = [vp, vp, i32, i32, vp]
    lib.ldm_dev_step0_flags.argtypes = [vp, vp, i32]
    lib.ldm_dev_graph_cache.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ldm_last_loop_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.ldm_set_profiling.argtypes = [vp, i32]
    lib.ldm_profile_count.argtypes = [vp]
    lib.ldm_profile_get.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ldm_profile_reset.argtypes = [vp]
    lib.ldm_get_layout.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ldm_describe.argtypes = [vp, C.c_char_p, i32]
    lib.ldm_layout_metrics.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.ldm_eval_average_iou.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    lib.ldm_eval_docsim.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp]
    lib.ldm_eval_max_iou_pairs.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp, i32, C.c_int64, i32, vp, vp, vp]
    graph = [vp, C.c_int64, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]  # canvas, n_nodes, CSR, first_node, counts, out, edge_out, err, stream
    lib.ldm_relation_violation.argtypes = [vp, i32, C.c_int64] + graph
    lib.ldm_relation_violation_dense.argtypes = [vp, i32, vp, i32, i32, vp] + graph
    lib.ldm_encode_cond.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]
    lib.ldm_relation_graph.argtypes = [vp, i32, vp, vp, i32, i32, i32, vp, C.c_double, u64, u64] + [vp] * 13
    lib.ldm_refinement_prior.argtypes = [vp, i32, i32, i32, i32, i32, vp, C.c_float, vp, vp, vp]
    lib.ldm_render_layouts.argtypes = [vp, i32, vp, vp, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ldm_render_grid_shape.argtypes = [i32, i32, i32, i32, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    i64, sz, f64 = C.c_int64, C.c_size_t, C.c_double
    lib.ldm_cluster_workspace_bytes.argtypes = [i32, i64, i32, i32, C.POINTER(sz)]
    lib.ldm_cluster_sort.argtypes = [vp, i32, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]
    lib.ldm_kmeans1d_fit.argtypes = [vp, vp, vp, i32, i64, vp, vp, i32, i32, i32, u64, i32, f64, vp, vp, vp, vp, vp, sz, vp]
    lib.ldm_kmeans1d_lloyd.argtypes = [vp, vp, vp, i32, i64, vp, vp, i32, vp, i32, f64, vp, vp, vp, vp, vp, sz, vp]
    lib.ldm_percentile_fit.argtypes = [vp, i32, i64, vp, vp, vp, i32, vp, vp, sz, vp]
    lib.ldm_nearest_centre.argtypes = [vp, i64, vp, i32, i32, vp, vp]
    lib.ldm_dev_cluster_stages.argtypes = [vp, i64, i32, u64, i32, i32, i32, f64] + [vp] * 13 + [sz, vp, vp]
    lib.ldm_q_sample.argtypes = [vp, vp, i32, u64, u64, i32, vp, vp]
    lib.ldm_vb_terms.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp]
    lib.ldm_vb_step.argtypes = [vp, vp, vp, i32, u64, u64, i32, vp, vp]
    lib.ldm_denoise_logits_t.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.ldm_q_sample_t.argtypes = [vp, vp, vp, vp, u64, u64, i32, vp, vp]
    lib.ldm_vb_terms_t.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.ldm_vb_step_t.argtypes = [vp, vp, vp, vp, vp, u64, u64, i32, vp, vp]
    lib.ldm_vb_grad.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    for name in EXPORTS:
        if name not in ("ldm_destroy", "ldm_last_error") and not name.startswith("ldm_fid_"):
            getattr(lib, name).restype = C.c_int
    if lib.ldm_abi_version() != ABI_VERSION:
        raise RuntimeError("libldm_hip.so ABI version mismatch — rebuild the extension")
    if path is None:
        _lib = lib
    return lib


def make_sampler(cfg) -> LdmSampler:
    """sampling_cfg (DictConfig / dict / attr object with the reference's field names,
    helpers/sampling.py:13-59) -> ldm_sampler."""
    get = (lambda k, d=None: cfg.get(k, d)) if hasattr(cfg, "get") else (lambda k, d=None: getattr(cfg, k, d))
    name = get("name")
    if name not in SAMPLERS:
        raise NotImplementedError(f"sampling '{name}'")  # sampling.py:117-118
    return LdmSampler(SAMPLERS[name], float(get("temperature", 1.0)), float(get("top_p", 1.0) or 1.0),
                      int(get("top_k", 1) or 1))


def _stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def refinement_prior(seq_orig: torch.Tensor, table_dev: torch.Tensor, weight: float, B: int,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cond["weak_logits"] of cond=refinement on the device (ldm_refinement_prior, kernels_refine.hip): the (B,C,S) float32
    tensor `table_dev[seq_orig].permute(0, 2, 1) * weight`, bit for bit.  seq_orig: (B,S) or — one conditioning layout for B
    samples — (1,S) ids, int64 or int32, on any device (a CPU tensor is uploaded: S ids per layout); table_dev: the (C,C)
    float32 [token][class] table on the GPU, refine_lambda NOT applied.  Runs on the current stream of the table's device.
    out: a contiguous (B,C,S) float32 tensor of that device to fill (any 4-byte aligned view), else one is allocated.
    An id outside [0, C) raises IndexError like the indexing it replaces (this reads the error word: one synchronisation)."""
    if not torch.cuda.is_available() or not table_dev.is_cuda:
        raise RuntimeError("layout_dm_amd.binding.refinement_prior needs a ROCm GPU (MI355X); there is no CPU path")
    lib = load_library()
    dev = table_dev.device
    if table_dev.dim() != 2 or table_dev.shape[0] != table_dev.shape[1] or table_dev.dtype != torch.float32:
        raise ValueError(f"table_dev must be (C,C) float32; got {tuple(table_dev.shape)} {table_dev.dtype}")
    seq = torch.as_tensor(seq_orig)
    if seq.dim() != 2 or seq.shape[1] < 1 or seq.shape[0] not in (1, int(B)):
        raise ValueError(f"seq_orig must be ({B},S) or (1,S), S >= 1; got {tuple(seq.shape)}")
    if seq.dtype not in (torch.int32, torch.int64):
        seq = seq.long()
    seq = seq.to(dev).contiguous()
    table = table_dev.contiguous()
    C_, S = int(table.shape[0]), int(seq.shape[1])
    if out is None:
        out = torch.empty((int(B), C_, S), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (int(B), C_, S) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({B},{C_},{S}) float32 tensor on {dev}")
    if int(B) == 0:
        return out
    err = torch.empty(1, dtype=torch.int32, device=dev)   # (zeroed by the call)
    with torch.cuda.device(dev):
        rc = lib.ldm_refinement_prior(seq.data_ptr(), int(seq.dtype == torch.int64), int(seq.shape[0]), int(B), S, C_,
                                      table.data_ptr(), float(weight), out.data_ptr(), err.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_refinement_prior failed ({rc})")
    if int(err.item()) & 1:   # (synchronises: seq / table temporaries are done with)
        raise IndexError(f"refinement prior: an id of seq_orig is outside [0, {C_})")
    return out


class Engine:
    """One libldm_hip handle = one model replica on one GPU."""

    def __init__(self, *, n_category: int, n_bin: int = 32, max_elem: int = 25, n_attr: int = 5,
                 d_model: int = 464, n_head: int = 8, d_ff: int = 1856, n_layer: int = 4, n_step: int = 100,
                 precision="exact", max_batch: int = 512, chunk: int = 0, device: Optional[int] = None,
                 q_type: str = "constrained", lanes: int = 0, timestep_type: Optional[str] = "adalayernorm"):
        if q_type not in Q_TYPES:
            raise NotImplementedError(f"q_type={q_type}: one of {sorted(Q_TYPES)}")
        if timestep_type not in TIMESTEP_TYPES:
            raise NotImplementedError(f"timestep_type={timestep_type}: one of {sorted(map(str, TIMESTEP_TYPES))}")
        self.timestep_type = timestep_type
        if not torch.cuda.is_available():
            raise RuntimeError("layout_dm_amd needs a ROCm GPU (MI355X); there is no CPU path")
        self.lib = load_library()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        prec = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
        self.cfg = LdmConfig(ABI_VERSION, n_category, n_bin, max_elem, n_attr, d_model, n_head, d_ff, n_layer,
                             n_step, prec, max_batch, chunk, Q_TYPES[q_type], lanes)
        self.q_type = q_type
        self.S = max_elem * n_attr
        self.n_attr, self.n_bin, self.n_category = n_attr, n_bin, n_category
        self.C = n_category + 4 * n_bin + 2
        self.T = n_step
        self.pad_id, self.mask_id = self.C - 2, self.C - 1
        self.max_batch = max_batch
        h = C.c_void_p()
        if TIMESTEP_TYPES[timestep_type] == NORM1_LAYER:
            rc = self.lib.ldm_create(C.byref(self.cfg), self.device_index, C.byref(h))
        else:
            rc = self.lib.ldm_create_variant(C.byref(self.cfg), TIMESTEP_TYPES[timestep_type], self.device_index, C.byref(h))
        if rc != 0:
            raise RuntimeError(f"ldm_create failed ({rc}): {self.lib.ldm_last_error(None).decode()}")
        self._h = h
        self._keep = {}  # tensors referenced by cached graphs must stay alive
        ck, ln = C.c_int(), C.c_int()
        self._check(self.lib.ldm_get_layout(self._h, C.byref(ck), C.byref(ln)), "ldm_get_layout")
        self.chunk, self.lanes = int(ck.value), int(ln.value)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.ldm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.ldm_last_error(self._h).decode()}")

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict: Dict[str, "torch.Tensor | np.ndarray"]):
        """Reference checkpoint (keys of SURVEY App. C, with or without 'model.module.')."""
        for k, v in state_dict.items():
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            a = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(self.lib.ldm_load_weight(self._h, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim),
                        f"ldm_load_weight({k})")
        self._check(self.lib.ldm_finalize_weights(self._h), "ldm_finalize_weights")
        self._round = None

    @property
    def batch_round(self) -> int:
        """Layouts per "round" of a sampling call (ldm_describe `round`): the one-launch loop runs one workgroup per layout
        on the device's compute units (256 on the MI355X), the per-step path `chunk` layouts on each of its lanes — a call
        costs whole rounds, so B = round + 1 costs what B = 2 * round costs (bench.py `batch_shapes`)."""
        if getattr(self, "_round", None) is None:
            self._round = max(1, int(self.describe().get("round", "256")))
        return self._round

    # ------------------------------------------------------------------ helpers
    def _tok(self, t: torch.Tensor) -> torch.Tensor:
        if t.device != self.device or t.dtype != torch.int32 or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.int32).contiguous()
        return t

    def make_cond(self, cond: Optional[dict], B: int):
        """cond dict of the reference (base.py:243-284 consumers) -> (ldm_cond, keep-alive list)."""
        if not cond:
            return None, []
        keep = []
        lc = LdmCond()
        seq = self._tok(torch.as_tensor(cond["seq"]))
        assert seq.shape == (B, self.S), f"cond['seq'] must be ({B},{self.S})"
        keep.append(seq)
        lc.d_cond_seq = seq.data_ptr()
        if "mask" in cond and cond["mask"] is not None:
            m = torch.as_tensor(cond["mask"]).to(device=self.device, dtype=torch.uint8).contiguous()
            keep.append(m)
            lc.d_strong_mask = m.data_ptr()
        if cond.get("type") == "refinement":
            wl = torch.as_tensor(cond["weak_logits"]).to(device=self.device, dtype=torch.float32).contiguous()
            assert wl.shape == (B, self.C, self.S)
            # weak_mask is by construction ~mask broadcast over classes (helpers/task.py:216)
            keep.append(wl)
            lc.d_weak_logits = wl.data_ptr()
        lc.pad_disable = 1 if cond.get("type") in ("c", "cwh", "refinement", "relation") else 0
        return lc, keep

    # ------------------------------------------------------------------ parity hooks
    def denoise_logits(self, tokens: torch.Tensor, t: int) -> torch.Tensor:
        tokens = self._tok(tokens)
        B = tokens.shape[0]
        out = torch.empty((B, self.S, self.C), dtype=torch.float32, device=self.device)
        self._check(self.lib.ldm_denoise_logits(self._h, tokens.data_ptr(), int(t), B, out.data_ptr(),
                                                _stream_ptr(self.device)), "ldm_denoise_logits")
        return out

    def posterior(self, logits: torch.Tensor, tokens: torch.Tensor, t_post: int, cond: Optional[dict] = None):
        tokens = self._tok(tokens)
        B = tokens.shape[0]
        logits = logits.to(device=self.device, dtype=torch.float32).contiguous()
        lc, keep = self.make_cond(cond, B)
        out = torch.empty((B, self.C, self.S), dtype=torch.float32, device=self.device)
        self._check(self.lib.ldm_posterior(self._h, logits.data_ptr(), tokens.data_ptr(), int(t_post), B,
                                           C.byref(lc) if lc else None, out.data_ptr(), _stream_ptr(self.device)),
                    "ldm_posterior")
        torch.cuda.current_stream(self.device).synchronize() if keep else None
        return out

    def sample_tokens(self, logp: torch.Tensor, sampling_cfg, seed: int = 0, first_layout: int = 0, step: int = 0,
                      cond: Optional[dict] = None):
        """helpers/sampling.py:81-130 on (B,C,S) log-probabilities.  cond (optional): {"seq", "type"} — the [PAD]
        disabling of base.py:272-284 for cond types c / cwh / refinement / relation."""
        logp = logp.to(device=self.device, dtype=torch.float32).contiguous()
        B = logp.shape[0]
        s = make_sampler(sampling_cfg)
        lc, keep = self.make_cond({"seq": cond["seq"], "type": cond.get("type")}, B) if cond else (None, [])
        out = torch.empty((B, self.S), dtype=torch.int32, device=self.device)
        self._check(self.lib.ldm_sample_tokens(self._h, logp.data_ptr(), C.byref(lc) if lc else None, C.byref(s), seed,
                                               first_layout, step, B, out.data_ptr(), _stream_ptr(self.device)),
                    "ldm_sample_tokens")
        if keep:
            torch.cuda.current_stream(self.device).synchronize()
        return out

    # ------------------------------------------------------------------ scoring given layouts
    def _check_tokens(self, rc: int, what: str):
        if rc == -6:   # a token the kernels refused (include/ldm_hip.h): the reference's index_to_log_onehot asserts
            raise ValueError(f"{what}: {self.lib.ldm_last_error(self._h).decode()}")
        self._check(rc, what)

    def q_sample(self, x0: torch.Tensor, t: int, seed: int = 0, first_layout: int = 0) -> torch.Tensor:
        """x_t ~ q(x_t | x_0) (constrained.py:223-230): (B,S) ids -> (B,S) int32 on the device.  One Philox uniform per
        token keyed by (seed, first_layout + b, t, position): the tokens do not depend on how a batch is cut over calls."""
        x0 = self._tok(x0)
        out = torch.empty_like(x0)
        self._check_tokens(self.lib.ldm_q_sample(self._h, x0.data_ptr(), int(t), int(seed), int(first_layout), x0.shape[0],
                                                 out.data_ptr(), _stream_ptr(self.device)), "ldm_q_sample")
        return out

    def vb_terms(self, logits: torch.Tensor, x0: torch.Tensor, xt: torch.Tensor, t: int, per_token: bool = False):
        """The bound's terms of timestep t from the denoiser's logits (B,S,C) of (xt, t): (B,4) float64 per-layout SUMS
        over the tokens of kl, decoder nll, auxiliary kl and x_0 hits (include/ldm_hip.h ldm_vb_terms); per_token: also the
        (3,B,S) float32 kl / nll / aux of every token."""
        x0, xt = self._tok(x0), self._tok(xt)
        B = x0.shape[0]
        assert xt.shape == x0.shape == (B, self.S) and tuple(logits.shape) == (B, self.S, self.C)
        logits = logits.to(device=self.device, dtype=torch.float32).contiguous()
        sums = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        tok = torch.empty((3, B, self.S), dtype=torch.float32, device=self.device) if per_token else None
        self._check_tokens(self.lib.ldm_vb_terms(self._h, logits.data_ptr(), x0.data_ptr(), xt.data_ptr(), int(t), B,
                                                 sums.data_ptr(), tok.data_ptr() if per_token else None,
                                                 _stream_ptr(self.device)), "ldm_vb_terms")
        return (sums, tok) if per_token else sums

    def vb_step(self, x0: torch.Tensor, t: int, xt: Optional[torch.Tensor] = None, seed: int = 0, first_layout: int = 0,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """q_sample (xt None; else the given state) -> this engine's denoiser pass -> vb_terms: (B,4) float64 sums."""
        x0 = self._tok(x0)
        B = x0.shape[0]
        if xt is not None:
            xt = self._tok(xt)
            assert xt.shape == x0.shape
        if out is None:
            out = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        assert out.shape == (B, 4) and out.dtype == torch.float64 and out.is_contiguous() and out.device == self.device
        self._check_tokens(self.lib.ldm_vb_step(self._h, x0.data_ptr(), xt.data_ptr() if xt is not None else None, int(t),
                                                int(seed), int(first_layout), B, out.data_ptr(), _stream_ptr(self.device)),
                           "ldm_vb_step")
        return out

    # ------------------------------------------------------------------ ... at a timestep per layout
    @property
    def per_layout_t(self) -> bool:
        """This engine's denoiser takes a timestep per layout (ldm_describe per_layout_t): every engine but `fast` on the
        reference's backbone, whose stack kernel takes one set of AdaLN rows per launch.  Where it is False the *_t calls
        raise (rc -4)."""
        if getattr(self, "_per_layout_t", None) is None:
            self._per_layout_t = self.describe().get("per_layout_t", "0") == "1"
        return self._per_layout_t

    def _host_t(self, t, B: int):
        """(B,) timesteps -> a host int32 array the call reads before it returns (the library checks the range)"""
        t = np.ascontiguousarray(torch.as_tensor(t).cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t), dtype=np.int32).reshape(-1)
        if t.size != B:
            raise ValueError(f"t must hold {B} timesteps, one per layout; got {t.size}")
        return t

    def _host_layout(self, layout, B: int):
        if layout is None:
            return None
        layout = np.ascontiguousarray(torch.as_tensor(layout).cpu().numpy() if isinstance(layout, torch.Tensor) else np.asarray(layout),
                                      dtype=np.uint64).reshape(-1)
        if layout.size != B:
            raise ValueError(f"layout must hold {B} layout indices, one per row; got {layout.size}")
        return layout

    def denoise_logits_t(self, tokens: torch.Tensor, t) -> torch.Tensor:
        """denoise_logits with t (B,) per-layout timesteps in one pass: row b has the bits of denoise_logits(tokens, t[b])[b]."""
        tokens = self._tok(tokens)
        B = tokens.shape[0]
        ht = self._host_t(t, B)
        out = torch.empty((B, self.S, self.C), dtype=torch.float32, device=self.device)
        self._check(self.lib.ldm_denoise_logits_t(self._h, tokens.data_ptr(), ht.ctypes.data_as(C.c_void_p), B, out.data_ptr(),
                                                  _stream_ptr(self.device)), "ldm_denoise_logits_t")
        return out

    def q_sample_t(self, x0: torch.Tensor, t, seed: int = 0, first_layout: int = 0, layout=None) -> torch.Tensor:
        """q_sample with t (B,) per-layout timesteps.  layout (B,) or None: the layout index of row b in the Philox key is
        first_layout + (layout[b] if given, else b) — row b equals q_sample(x0, t[b], seed, first_layout)[layout[b] or b]
        wherever x0's row is that layout's."""
        x0 = self._tok(x0)
        B = x0.shape[0]
        ht, hl = self._host_t(t, B), self._host_layout(layout, B)
        out = torch.empty_like(x0)
        self._check_tokens(self.lib.ldm_q_sample_t(self._h, x0.data_ptr(), ht.ctypes.data_as(C.c_void_p),
                                                   hl.ctypes.data_as(C.c_void_p) if hl is not None else None, int(seed), int(first_layout),
                                                   B, out.data_ptr(), _stream_ptr(self.device)), "ldm_q_sample_t")
        return out

    def vb_terms_t(self, logits: torch.Tensor, x0: torch.Tensor, xt: torch.Tensor, t, per_token: bool = False):
        """vb_terms with t (B,) per-layout timesteps: row b has the bits of vb_terms(.., t[b])[b]."""
        x0, xt = self._tok(x0), self._tok(xt)
        B = x0.shape[0]
        assert xt.shape == x0.shape == (B, self.S) and tuple(logits.shape) == (B, self.S, self.C)
        ht = self._host_t(t, B)
        logits = logits.to(device=self.device, dtype=torch.float32).contiguous()
        sums = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        tok = torch.empty((3, B, self.S), dtype=torch.float32, device=self.device) if per_token else None
        self._check_tokens(self.lib.ldm_vb_terms_t(self._h, logits.data_ptr(), x0.data_ptr(), xt.data_ptr(), ht.ctypes.data_as(C.c_void_p),
                                                   B, sums.data_ptr(), tok.data_ptr() if per_token else None,
                                                   _stream_ptr(self.device)), "ldm_vb_terms_t")
        return (sums, tok) if per_token else sums

    def vb_step_t(self, x0: torch.Tensor, t, xt: Optional[torch.Tensor] = None, seed: int = 0, first_layout: int = 0,
                  layout=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """vb_step with t (B,) per-layout timesteps (and layout (B,) Philox layout indices, see q_sample_t): ONE denoiser pass per
        chunk for layouts at different t; (B,4) float64 sums, row b with the bits of vb_step(.., t[b])[b]."""
        x0 = self._tok(x0)
        B = x0.shape[0]
        ht, hl = self._host_t(t, B), self._host_layout(layout, B)
        if xt is not None:
            xt = self._tok(xt)
            assert xt.shape == x0.shape
        if out is None:
            out = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        assert out.shape == (B, 4) and out.dtype == torch.float64 and out.is_contiguous() and out.device == self.device
        self._check_tokens(self.lib.ldm_vb_step_t(self._h, x0.data_ptr(), xt.data_ptr() if xt is not None else None,
                                                  ht.ctypes.data_as(C.c_void_p), hl.ctypes.data_as(C.c_void_p) if hl is not None else None,
                                                  int(seed), int(first_layout), B, out.data_ptr(), _stream_ptr(self.device)),
                           "ldm_vb_step_t")
        return out

    def vb_grad(self, logits: torch.Tensor, x0: torch.Tensor, xt: torch.Tensor, t, coef, want_grad: bool = True):
        """(grad | None, sums): d/dlogits (B,S,C) float32 of sum_b coef[b,0] (t_b == 0 ? nll_b : kl_b) + coef[b,1] (t_b == 0 ? nll_b :
        aux_b) over the token sums (include/ldm_hip.h ldm_vb_grad; coef (B,2) float64: training.loss_coefficients), and the (B,4)
        float64 sums with vb_terms_t's bits on an exact handle.  t (B,) per-layout timesteps.  want_grad=False: the sums alone
        (coef may be None).  Runs no denoiser; every handle takes it."""
        x0, xt = self._tok(x0), self._tok(xt)
        B = x0.shape[0]
        assert xt.shape == x0.shape == (B, self.S) and tuple(logits.shape) == (B, self.S, self.C)
        ht = self._host_t(t, B)
        logits = logits.to(device=self.device, dtype=torch.float32).contiguous()
        sums = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        grad = None
        if want_grad:
            coef = torch.as_tensor(coef).to(device=self.device, dtype=torch.float64).contiguous()
            assert tuple(coef.shape) == (B, 2)
            grad = torch.empty((B, self.S, self.C), dtype=torch.float32, device=self.device)
        self._check_tokens(self.lib.ldm_vb_grad(self._h, logits.data_ptr(), x0.data_ptr(), xt.data_ptr(), ht.ctypes.data_as(C.c_void_p), B,
                                                coef.data_ptr() if want_grad else None, grad.data_ptr() if want_grad else None,
                                                sums.data_ptr(), _stream_ptr(self.device)), "ldm_vb_grad")
        return grad, sums

    # ------------------------------------------------------------------ hot path
    def sample_step(self, tokens: torch.Tensor, t_model: int, sampling_cfg, t_post: Optional[int] = None,
                    cond: Optional[dict] = None, seed: int = 0, first_layout: int = 0, step: int = 0, relation=None):
        """relation: (LdmRelation, keep-alives) from make_relation for cond["type"] == "relation"."""
        tokens = self._tok(tokens)
        B = tokens.shape[0]
        s = make_sampler(sampling_cfg)
        lc, keep = self.make_cond(cond, B)
        out = torch.empty_like(tokens)
        self._check(self.lib.ldm_sample_step(self._h, tokens.data_ptr(), out.data_ptr(), int(t_model),
                                             int(t_model if t_post is None else t_post),
                                             C.byref(lc) if lc else None, C.byref(relation[0]) if relation else None,
                                             C.byref(s), seed, first_layout, step, B,
                                             _stream_ptr(self.device)), "ldm_sample_step")
        if keep:
            torch.cuda.current_stream(self.device).synchronize()
        return out

    def sample_loop(self, tokens: torch.Tensor, t_model: Sequence[int], t_post: Sequence[int], sampling_cfg,
                    cond: Optional[dict] = None, seed: int = 0, first_layout: int = 0,
                    intermediates: bool = False, use_graph: bool = True, lc_keep=None, relation=None):
        """In-place T-step loop on `tokens` (B,S) int32 cuda. Returns (tokens, intermediates|None).
        relation: (LdmRelation, keep-alives) from make_relation — the whole cond=relation loop (posterior ->
        logit adjustment -> [PAD] disable -> draw per step) then runs inside the same launch sequence / hipGraph."""
        tokens = self._tok(tokens)
        B = tokens.shape[0]
        n = len(t_model)
        s = make_sampler(sampling_cfg)
        if lc_keep is not None:
            lc, keep = lc_keep
        else:
            lc, keep = self.make_cond(cond, B)
        inter = torch.empty((n, B, self.S), dtype=torch.int32, device=self.device) if intermediates else None
        tm = (C.c_int32 * n)(*[int(x) for x in t_model])
        tp = (C.c_int32 * n)(*[int(x) for x in t_post])
        self._check(self.lib.ldm_sample_loop(self._h, tokens.data_ptr(), C.byref(lc) if lc else None,
                                             C.byref(relation[0]) if relation else None, tm, tp, n,
                                             C.byref(s), seed, first_layout, B,
                                             inter.data_ptr() if inter is not None else None,
                                             1 if use_graph else 0, _stream_ptr(self.device)), "ldm_sample_loop")
        if keep and lc_keep is None:
            torch.cuda.current_stream(self.device).synchronize()
        return tokens, inter

    # ------------------------------------------------------------------ near-tie report (deterministic decoding)
    def set_tie_report(self, tie_rel: float, tie_abs: float = 0.0):
        """Deterministic steps / loops mark, per (step, layout), whether some token was decided with a lead over the
        runner-up below max(tie_rel * max |logit of the token|, tie_abs) (include/ldm_hip.h); 0, 0 disables."""
        self._check(self.lib.ldm_set_tie_report(self._h, float(tie_rel), float(tie_abs)), "ldm_set_tie_report")

    def tie_flags(self, n_steps: int, B: int) -> torch.Tensor:
        """(n_steps, B) uint8 flags of the most recent deterministic call."""
        out = torch.empty((n_steps, B), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ldm_get_tie_flags(self._h, out.data_ptr(), int(n_steps), int(B), _stream_ptr(self.device)),
                    "ldm_get_tie_flags")
        return out

    def step0_flags(self, B: int) -> np.ndarray:
        """Development hook: (B,) uint8, 1 where a layout of the most recent sample_loop call read its first step's logits
        from the handle's step-0 table (an all-[MASK] start on the one-launch loop) instead of running the denoiser."""
        out = np.zeros(int(B), dtype=np.uint8)
        self._check(self.lib.ldm_dev_step0_flags(self._h, out.ctypes.data_as(C.c_void_p), int(B)), "ldm_dev_step0_flags")
        return out

    def graph_cache(self):
        """Development hook: (entries, captures) of the handle's cache of captured sampling loops — graphs held now (at most 8
        keys) and keys captured since the engine was created.  A sample_loop call that replays a cached key changes neither."""
        entries, captures = C.c_int(), C.c_int()
        self._check(self.lib.ldm_dev_graph_cache(self._h, C.byref(entries), C.byref(captures)), "ldm_dev_graph_cache")
        return int(entries.value), int(captures.value)

    # ------------------------------------------------------------------ cond=relation
    def make_relation(self, graph, centres, canvas_bins, relation_lambda: float, num_update: int, n_graph_total: int):
        """Device-side description of cond["batch_w_canvas"] for ldm_relation_update.  graph: object / dict with
        y (nodes,), edge_index (2,E) global node ids, edge_attr (E,), batch (nodes,) — torch_geometric DataBatch
        fields (helpers/task.py:112-114).  Returns (LdmRelation, keep-alive tensors)."""
        from .relation import graph_to_csr

        B = int(n_graph_total)
        csr = getattr(graph, "csr", None)
        if csr is not None and csr["edge_off"].numel() == B + 1:
            # task.relation_graph built the graph in this form on the device: nothing to rebuild.  The CSR is taken as it is,
            # without graph_to_csr's checks: task.RelationGraph keeps it and its DataBatch view read-only for that reason
            off, src_l, dst_l, ea = csr["edge_off"], csr["src"], csr["dst"], csr["attr"]
        else:
            off, src_l, dst_l, ea = graph_to_csr(graph, B)
        dev = self.device
        keep = [off.to(dev), src_l.to(dev), dst_l.to(dev), ea.to(dev),
                torch.as_tensor(centres, dtype=torch.float64).float().reshape(4, self.n_bin).contiguous().to(dev)]
        rel = LdmRelation(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(),
                          keep[4].data_ptr(), (C.c_int32 * 4)(*[int(x) for x in canvas_bins]),
                          float(relation_lambda), int(num_update), B)
        return rel, keep

    def relation_update(self, logp: torch.Tensor, cond_seq: torch.Tensor, rel, t: int, layout_offset: int = 0):
        """In-place logit adjustment of `logp` (B,C,S) float32 cuda (logit_adjustment.update, l.88-126)."""
        assert logp.is_cuda and logp.dtype == torch.float32 and logp.is_contiguous()
        lr, keep = rel
        cond_seq = self._tok(cond_seq)
        if layout_offset:   # a window of the plan: `logp` / `cond_seq` hold layouts layout_offset .. of it (the step stays the plan's)
            from .relation import _relation_window

            assert 0 < layout_offset and layout_offset + logp.shape[0] <= lr.n_graph_total, "window outside the relation plan"
            lr, keep = _relation_window(rel, int(layout_offset))
        self._check(self.lib.ldm_relation_update(self._h, logp.data_ptr(), cond_seq.data_ptr(), C.byref(lr), int(t),
                                                 logp.shape[0], _stream_ptr(self.device)), "ldm_relation_update")
        torch.cuda.current_stream(self.device).synchronize()  # cond_seq copy / keep-alives may be temporaries
        return logp

    # ------------------------------------------------------------------ result packaging
    def decode(self, tokens: torch.Tensor, centres: Optional[torch.Tensor] = None):
        """ids (B,S) -> {"bbox" (B,E,4), "label" (B,E) int64, "mask" (B,E) bool} on the device
        (LayoutSequenceTokenizer.decode + BboxTokenizer.decode, layout_tokenizer.py:255-266 /
        bbox_tokenizer.py:117-168).  centres: None = linear bins (float32 boxes); (4,n_bin) float64
        cluster centres in x,y,w,h order = kmeans/percentile (float64 boxes, like the reference)."""
        tokens = self._tok(tokens)
        B = tokens.shape[0]
        E = self.S // self.n_attr
        f64 = centres is not None
        if f64:
            centres = torch.as_tensor(centres, dtype=torch.float64).to(self.device).contiguous()
            assert centres.numel() == 4 * self.n_bin, "centres must be (4, n_bin)"
        bbox = torch.empty((B, E, 4), dtype=torch.float64 if f64 else torch.float32, device=self.device)
        label = torch.empty((B, E), dtype=torch.int64, device=self.device)
        mask = torch.empty((B, E), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ldm_decode_layouts(self._h, tokens.data_ptr(), B, centres.data_ptr() if f64 else None,
                                                1 if f64 else 0, bbox.data_ptr(), label.data_ptr(),
                                                mask.data_ptr(), _stream_ptr(self.device)), "ldm_decode_layouts")
        if f64:
            torch.cuda.current_stream(self.device).synchronize()  # `centres` must outlive the kernel
        return {"bbox": bbox, "label": label, "mask": mask.bool()}

    # ------------------------------------------------------------------ introspection
    def describe(self) -> Dict[str, str]:
        """What this handle runs (ldm_describe): numerics mode, kernel family, loop structure, chunk / lanes, near-tie
        thresholds and the development knobs the LIBRARY honoured (LDM_DEV=1 only) — not what os.environ says."""
        cap = 1024
        while True:
            buf = C.create_string_buffer(cap)
            n = self.lib.ldm_describe(self._h, buf, cap)
            if n < 0:
                raise RuntimeError("ldm_describe failed")
            if n < cap:
                break
            cap = n + 1   # (returns the length needed: the honoured-knob list is unbounded)
        out = {}
        for kv in buf.value.decode().split(";"):
            k, _, v = kv.partition("=")
            if k == "knobs":
                out[k] = buf.value.decode().split("knobs=", 1)[1]
                break
            out[k] = v
        # the step-0 logits cache of the one-launch loop: on / off and its (first timestep, S) keys, oldest first
        out["step0_cache"] = {"enabled": out.pop("step0_cache", "off") == "on",
                              "entries": [[int(x) for x in e.split(":")] for e in out.pop("step0_entries", "").split(",") if e]}
        return out

    def last_loop_ms(self) -> float:
        ms = C.c_float()
        self._check(self.lib.ldm_last_loop_ms(self._h, C.byref(ms)), "ldm_last_loop_ms")
        return float(ms.value)

    def set_profiling(self, on: bool):
        self._check(self.lib.ldm_set_profiling(self._h, 1 if on else 0), "ldm_set_profiling")

    def profile(self, reset: bool = False):
        n = self.lib.ldm_profile_count(self._h)
        rows = []
        for i in range(n):
            name, ms, cnt, fl, by = C.c_char_p(), C.c_double(), C.c_int64(), C.c_double(), C.c_double()
            self.lib.ldm_profile_get(self._h, i, C.byref(name), C.byref(ms), C.byref(cnt), C.byref(fl), C.byref(by))
            rows.append({"name": name.value.decode(), "ms": ms.value, "launches": cnt.value, "flops": fl.value,
                         "bytes": by.value})
        if reset:
            self.lib.ldm_profile_reset(self._h)
        return rows
