"""cond= inputs from raw layouts, on the GPU: `LayoutSequenceTokenizer.encode` (helpers/layout_tokenizer.py:208-253 +
helpers/bbox_tokenizer.py:84-115), `get_cond` (helpers/task.py:27-151) and the relation transforms AddCanvasElement +
AddRelationConstraints (data/util.py:111-177, use_v1=False) of the reference, without torch_geometric, hydra or its datasets.

    layouts = {"bbox": (B,E,4) float32 | float64, "label": (B,E) int64, "mask": (B,E) bool}     # dense, host or device
    cond = get_cond(layouts, tokenizer, "refinement")
    out = model.sample(batch_size=B, cond=cond, sampling_cfg=cfg)

`ldm_encode_cond` runs encode and the cond rule in one kernel, `ldm_relation_graph` walks the element pairs of every layout
(kernels_cond.hip; arithmetic in csrc/ldm_cond_core.h, checked bit for bit against the reference on the host and on the device).
Scope: the LayoutDM tokenizer configuration the device-side decode assumes — c-x-y-w-h, stacked x-y-w-h vocabulary, [pad, mask],
pad_until_max, no bos / eos, sort_by=None — with linear, percentile or kmeans bins.

kmeans: a coordinate goes to the nearest sorted centre by |float32(x) - c| evaluated in float64, the lowest index on a tie.
sklearn's `predict` evaluates c^2 - 2xc through BLAS in float32 and cannot be reproduced bit for bit AT a midpoint between two
centres; away from midpoints the two agree.

Randomness.  The reference draws the partial keep mask with `random` / `torch.rand`, the refinement noise with `torch.normal` and
the sampled relations with `random.Random.sample`.  Pass `keep=`, `noise=` or `selection=` to supply them.  Otherwise the kernels
draw them with the package's Philox4x32-10 keyed by (seed, first_layout + layout index, purpose, slot): the same DISTRIBUTIONS as
the reference's, not its streams (as DESIGN section 4 says of torch.multinomial), and independent of how a batch is cut or how
many ranks share it.

There is no CPU fallback: without the built library or a GPU every function raises.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .binding import _stream_ptr, load_library

COND_TYPES = ["c", "cwh", "partial", "gt", "random", "refinement", "relation"]   # task.py:16-24
RULES = {"gt": 0, "c": 1, "cwh": 2, "partial": 3, "refinement": 4, "relation": 5}   # LDM_COND_* of include/ldm_hip.h
QUANT = {"linear": 0, "percentile": 1, "kmeans": 2}                                 # LDM_QUANT_*
ERR_PREFIX, ERR_NON_FINITE, ERR_LABEL = 1, 2, 4
MAX_ELEM = 32


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("layout_dm_amd.task needs a ROCm GPU (MI355X); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def tokenizer_geometry(tokenizer):
    """Pure host logic: (n_category, n_bin, max_elem, quant name, (4,n_bin) float64 centres | None) of a tokenizer the kernels
    cover; NotImplementedError for any other configuration."""
    bbt = tokenizer.bbox_tokenizer
    special = list(tokenizer.special_tokens)
    if (special != ["pad", "mask"] or list(tokenizer.var_names) != ["c", "x", "y", "w", "h"]
            or bbt.shared_bbox_vocab != "x-y-w-h" or list(bbt.var_names) != ["x", "y", "w", "h"]
            or list(getattr(bbt, "_var_order", ["x", "y", "w", "h"])) != ["x", "y", "w", "h"]):
        raise NotImplementedError("task.encode: var_order c-x-y-w-h, stacked x-y-w-h vocabulary, special tokens [pad, mask]")
    if not getattr(tokenizer, "pad_until_max", True) or getattr(tokenizer, "sort_by", None) not in (None, "None", "none"):
        raise NotImplementedError("task.encode: pad_until_max with sort_by=None")
    quant = str(bbt.bbox_quantization)
    if quant not in QUANT:
        raise NotImplementedError(f"bbox_quantization={quant}")
    N, E = int(tokenizer.N_bbox_per_var), int(tokenizer.max_seq_length)
    if tokenizer.N_total != tokenizer.N_category + 4 * N + 2:
        raise NotImplementedError("task.encode: vocabulary is not n_category + 4 * n_bin + [pad, mask]")
    if not 1 <= E <= MAX_ELEM or not 1 <= N <= 128:
        raise NotImplementedError(f"task.encode: at most {MAX_ELEM} elements and 128 bins (got {E}, {N})")
    centres = None
    if quant != "linear":
        cs = [np.asarray(bbt.clustering_models[f"{k}-{N}"].cluster_centers_, dtype=np.float64).reshape(-1) for k in "xywh"]
        if any(c.shape != (N,) for c in cs):
            raise NotImplementedError("task.encode: cluster centres must be one-dimensional")
        centres = torch.from_numpy(np.sort(np.stack(cs), axis=1))   # bbox_tokenizer.py:62-68 sorts them
    return int(tokenizer.N_category), N, E, quant, centres


def _dense(layouts: Dict, E: int, dev: torch.device):
    """(bbox float32|float64 (B,E,4), label int64 (B,E), mask uint8 (B,E)) contiguous on `dev`, padded to E slots."""
    bbox, label, mask = (torch.as_tensor(layouts[k]) for k in ("bbox", "label", "mask"))
    if bbox.dim() != 3 or bbox.shape[-1] != 4 or tuple(label.shape) != tuple(bbox.shape[:2]) or label.shape != mask.shape:
        raise ValueError(f"layouts: bbox (B,S,4), label (B,S), mask (B,S); got {tuple(bbox.shape)}, {tuple(label.shape)}, "
                         f"{tuple(mask.shape)}")
    if bbox.shape[1] > E:
        raise ValueError(f"layouts hold {bbox.shape[1]} element slots, the tokenizer {E}")
    dt = torch.float64 if bbox.dtype == torch.float64 else torch.float32
    bbox = bbox.to(device=dev, dtype=dt)
    label = label.to(device=dev, dtype=torch.int64)
    mask = mask.to(device=dev).ne(0).to(torch.uint8)
    pad = E - bbox.shape[1]
    if pad:   # _pad_until, layout_tokenizer.py:87-94
        bbox = torch.nn.functional.pad(bbox, (0, 0, 0, pad))
        label = torch.nn.functional.pad(label, (0, pad))
        mask = torch.nn.functional.pad(mask, (0, pad))
    return bbox.contiguous(), label.contiguous(), mask.contiguous()


def _raise_for(err: int, what: str):
    if err & ERR_PREFIX:
        raise ValueError(f"{what}: a layout's mask is not a prefix of its row (layout_tokenizer.py:230-232 asserts this)")
    if err & ERR_NON_FINITE:
        raise ValueError(f"{what}: a valid element has a non-finite coordinate")
    if err & ERR_LABEL:
        raise ValueError(f"{what}: a valid element's label is outside [0, n_category)")
    if err:
        raise RuntimeError(f"{what}: device error flags {err}")


def _own_seed(seed: Optional[int]) -> int:
    """None -> drawn from torch's global CPU generator, so torch.manual_seed keeps runs reproducible (as diffusion.sample)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)


def encode_cond(geometry, bbox, label, mask, rule: str = "gt", *, keep=None, noise=None, seed: int = 0, first_layout: int = 0,
                want_noise: bool = False, check: bool = True):
    """ldm_encode_cond on dense device tensors (see _dense).  -> dict of DEVICE tensors: seq int32 (B,5E), mask uint8 (B,5E),
    num_element int32 (B), seq_orig int32 (refinement), noise float32 (B,E,4) (refinement with want_noise), err int32 (1).
    check=True reads the error word back and raises (one device-to-host read); check=False leaves that to the caller."""
    n_category, N, E, quant, centres = geometry
    dev = bbox.device
    B = bbox.shape[0]
    S = 5 * E
    seq = torch.empty((B, S), dtype=torch.int32, device=dev)
    cm = torch.empty((B, S), dtype=torch.uint8, device=dev)
    num = torch.empty(B, dtype=torch.int32, device=dev)
    orig = torch.empty((B, S), dtype=torch.int32, device=dev) if rule == "refinement" else None
    nz_out = torch.empty((B, E, 4), dtype=torch.float32, device=dev) if rule == "refinement" and want_noise else None
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if centres is not None:
        centres = centres.to(device=dev, dtype=torch.float64).contiguous()
    if keep is not None:
        keep = torch.as_tensor(keep).to(dev).ne(0).to(torch.uint8)
        if keep.shape[0] != B or keep.dim() != 2 or keep.shape[1] > E:
            raise ValueError(f"keep must be (B, <= {E}); got {tuple(keep.shape)}")
        keep = torch.nn.functional.pad(keep, (0, E - keep.shape[1])).contiguous()
    if noise is not None:
        noise = torch.as_tensor(noise).to(device=dev, dtype=torch.float32)
        if noise.dim() != 3 or noise.shape[0] != B or noise.shape[1] > E or noise.shape[2] != 4:
            raise ValueError(f"noise must be (B, <= {E}, 4); got {tuple(noise.shape)}")
        noise = torch.nn.functional.pad(noise, (0, 0, 0, E - noise.shape[1])).contiguous()
    ptr = lambda t: t.data_ptr() if t is not None else None
    lib = load_library()
    with torch.cuda.device(dev):
        rc = lib.ldm_encode_cond(bbox.data_ptr(), int(bbox.dtype == torch.float64), label.data_ptr(), mask.data_ptr(), B, E,
                                 n_category, N, QUANT[quant], ptr(centres), RULES[rule], ptr(keep), ptr(noise), int(seed),
                                 int(first_layout), seq.data_ptr(), cm.data_ptr(), ptr(orig), num.data_ptr(), ptr(nz_out),
                                 err.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_encode_cond failed ({rc})")
    if check:
        _raise_for(int(err.item()), "task.encode")   # the error check costs one device-to-host read (a synchronisation)
    # check=False: nothing is read back; the caller reads `err` when it suits it (_raise_for).  The temporaries above go back to
    # torch's caching allocator, which hands them out again only in stream order: no synchronisation is needed for them.
    return {"seq": seq, "mask": cm, "num_element": num, "seq_orig": orig, "noise": nz_out, "err": err}


def encode(tokenizer, bbox, label, mask) -> Dict[str, torch.Tensor]:
    """tokenizer.encode({"bbox", "label", "mask"}) (layout_tokenizer.py:208-253): {"seq" int64 (B,5E), "mask" bool (B,5E)}
    on the device `bbox` lives on."""
    out_dev = torch.as_tensor(bbox).device
    geometry = tokenizer_geometry(tokenizer)
    b, l, m = _dense({"bbox": bbox, "label": label, "mask": mask}, geometry[2], _device() if out_dev.type != "cuda" else out_dev)
    r = encode_cond(geometry, b, l, m, "gt")
    return {"seq": r["seq"].long().to(out_dev), "mask": r["mask"].bool().to(out_dev)}


class RelationGraph:
    """cond["batch_w_canvas"] without torch_geometric: the DataBatch fields the consumers read — x (nodes,4), y (nodes,),
    batch (nodes,), edge_index (2,E) GLOBAL node ids, edge_attr (E,), attr["has_canvas_element"] — and `csr`, the per-layout
    device arrays they were built from (edge_off, src, dst, attr int32; first_node int64; canvas uint8).

    The fields are read-only properties: `csr` and the DataBatch view describe the same graph, and Engine.make_relation samples
    under `csr` as it is, without the checks relation.graph_to_csr makes on a foreign graph.  To change a graph (filter edges,
    edit edge_attr), build a plain dict {"y", "batch", "edge_index", "edge_attr", "x"} from the edited tensors: every consumer
    takes that form and derives the CSR from it.  Do not edit the tensors in place."""

    def __init__(self, x, y, batch, edge_index, edge_attr, n_graph: int, csr: Dict[str, torch.Tensor]):
        self._fields = {"x": x, "y": y, "batch": batch, "edge_index": edge_index, "edge_attr": edge_attr}
        self._n_graph = int(n_graph)
        self._attr = {"has_canvas_element": torch.ones(self._n_graph, dtype=torch.bool, device=y.device)}
        self._csr = dict(csr)

    x = property(lambda self: self._fields["x"])
    y = property(lambda self: self._fields["y"])
    batch = property(lambda self: self._fields["batch"])
    edge_index = property(lambda self: self._fields["edge_index"])
    edge_attr = property(lambda self: self._fields["edge_attr"])
    num_graphs = property(lambda self: self._n_graph)
    attr = property(lambda self: self._attr)
    csr = property(lambda self: self._csr)

    def to(self, device) -> "RelationGraph":
        """The same graph with its DataBatch fields on `device` (what torch_geometric's batch.to(device) does); `csr` stays on
        the GPU it was built on."""
        device = torch.device(device)
        if all(t.device == device for t in self._fields.values()):
            return self
        f = {k: v.to(device) for k, v in self._fields.items()}
        return RelationGraph(f["x"], f["y"], f["batch"], f["edge_index"], f["edge_attr"], self._n_graph, self._csr)


def relation_graph(layouts: Dict, tokenizer, *, selection=None, edge_ratio: float = 0.1, seed: Optional[int] = None,
                   first_layout: int = 0, _dense_inputs=None, _pending_err=None) -> RelationGraph:
    """AddCanvasElement + AddRelationConstraints(edge_ratio) of every layout, collated (data/util.py:111-177).
    selection (B,2,E+1,E+1) bool: [kind: 0 size, 1 loc][i][j] — relation `kind` of the node pair i < j (node 0 = the canvas) is
    one of the sampled ones; None = drawn: exactly int(2 * C(n+1, 2) * edge_ratio) per layout, uniformly without replacement."""
    geometry = tokenizer_geometry(tokenizer)
    n_category, _, E = geometry[:3]
    out_dev = torch.as_tensor(layouts["bbox"]).device
    dev = out_dev if out_dev.type == "cuda" else _device()
    bbox, label, mask = _dense_inputs if _dense_inputs is not None else _dense(layouts, E, dev)
    B = bbox.shape[0]
    if B < 1:
        raise ValueError("relation_graph: empty batch")
    if not 0.0 <= float(edge_ratio) <= 1.0:
        raise ValueError(f"edge_ratio={edge_ratio}")
    P = (E + 1) * E // 2
    if selection is not None:
        selection = torch.as_tensor(selection).to(dev).ne(0).to(torch.uint8).contiguous()
        if tuple(selection.shape) != (B, 2, E + 1, E + 1):
            raise ValueError(f"selection must be ({B},2,{E + 1},{E + 1}); got {tuple(selection.shape)}")
    else:
        seed = _own_seed(seed)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    work, off, src, dst, attr = i32(B, 2 * P + 1), i32(B + 1), i32(B * P), i32(B * P), i32(B * P)
    first, y, batch = i64(B), i64(B * (E + 1)), i64(B * (E + 1))
    x = torch.empty((B * (E + 1), 4), dtype=bbox.dtype, device=dev)
    canvas = torch.empty(B * (E + 1), dtype=torch.uint8, device=dev)
    totals, err = i32(2), torch.zeros(1, dtype=torch.int32, device=dev)
    lib = load_library()
    with torch.cuda.device(dev):
        rc = lib.ldm_relation_graph(bbox.data_ptr(), int(bbox.dtype == torch.float64), label.data_ptr(), mask.data_ptr(), B, E,
                                    n_category, selection.data_ptr() if selection is not None else None, float(edge_ratio),
                                    int(seed or 0), int(first_layout), work.data_ptr(), off.data_ptr(), src.data_ptr(),
                                    dst.data_ptr(), attr.data_ptr(), first.data_ptr(), x.data_ptr(), y.data_ptr(),
                                    batch.data_ptr(), canvas.data_ptr(), totals.data_ptr(), err.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_relation_graph failed ({rc})")
    # the one device-to-host read: edge_index has shape (2, n_edge).  The error words travel with it (get_cond's encode included)
    words = [totals, err] + ([_pending_err] if _pending_err is not None else [])
    n_edge, n_nodes, e, *pending = torch.cat(words).tolist()
    if pending:
        _raise_for(pending[0], "task.encode")
    _raise_for(e, "task.relation_graph")
    src, dst, attr = src[:n_edge], dst[:n_edge], attr[:n_edge]
    x, y, batch, canvas = x[:n_nodes], y[:n_nodes], batch[:n_nodes], canvas[:n_nodes]
    counts = (off[1:] - off[:-1]).long()
    base = torch.repeat_interleave(first, counts, output_size=n_edge)
    edge_index = torch.stack([src.long() + base, dst.long() + base])
    csr = {"edge_off": off, "src": src, "dst": dst, "attr": attr, "first_node": first, "canvas": canvas}
    mv = lambda t: t.to(out_dev)
    return RelationGraph(mv(x), mv(y), mv(batch), mv(edge_index), mv(attr.long()), B, csr)


def get_cond(layouts: Dict, tokenizer, cond_type: str = "c", *, keep=None, noise=None, selection=None, edge_ratio: float = 0.1,
             seed: Optional[int] = None, first_layout: int = 0) -> Dict:
    """get_cond(batch, tokenizer, cond_type, model_type="LayoutDM") of the reference (helpers/task.py:27-151) from dense
    layouts.  The result has its keys and dtypes — seq int64, mask bool, type, num_element int64 (c / cwh / refinement /
    relation), seq_orig (refinement), batch_w_canvas (relation: a RelationGraph) — with tensors on the device of
    layouts["bbox"], and goes into `LayoutDM.sample(cond=...)` as it is.

    keep (B,E) bool: the elements cond=partial keeps (the reference's returned cond["mask"][:, ::5]); noise (B,E,4) float32: what
    cond=refinement adds to the boxes; selection: see relation_graph.  Each None = drawn on the device from `seed`
    (None = from torch's global CPU generator) and the layout's global index first_layout + b; see the module docstring.

    Every call makes exactly one device-to-host read: the error word (a bad input raises ValueError here, as the reference
    asserts in encode), which for cond=relation travels with the edge total that sizes edge_index."""
    if cond_type not in COND_TYPES:
        raise ValueError(f"cond_type={cond_type}: one of {COND_TYPES}")
    if cond_type == "random":
        raise NotImplementedError(
            "cond_type=random: helpers/mask.py sample_mask ranks torch.rand scores through batch_topk_mask; its rule is not restated "
            "here (no fixture pins its tie and ordering behaviour)")
    geometry = tokenizer_geometry(tokenizer)
    out_dev = torch.as_tensor(layouts["bbox"]).device
    dev = out_dev if out_dev.type == "cuda" else _device()
    bbox, label, mask = _dense(layouts, geometry[2], dev)
    draws = (cond_type == "partial" and keep is None) or (cond_type == "refinement" and noise is None) or \
        (cond_type == "relation" and selection is None)
    if draws:
        seed = _own_seed(seed)
    r = encode_cond(geometry, bbox, label, mask, cond_type, keep=keep if cond_type == "partial" else None,
                    noise=noise if cond_type == "refinement" else None, seed=int(seed or 0), first_layout=first_layout,
                    check=cond_type != "relation")   # relation: its error word is read together with the edge total
    cond = {"seq": r["seq"].long().to(out_dev), "mask": r["mask"].bool().to(out_dev)}
    if cond_type == "refinement":
        cond["seq_orig"] = r["seq_orig"].long().to(out_dev)
    if cond_type == "relation":
        cond["batch_w_canvas"] = relation_graph(layouts, tokenizer, selection=selection, edge_ratio=edge_ratio, seed=seed,
                                                first_layout=first_layout, _dense_inputs=(bbox, label, mask), _pending_err=r["err"])
    cond["type"] = cond_type
    if cond_type in ("c", "cwh", "refinement", "relation"):
        cond["num_element"] = r["num_element"].long().to(out_dev)
    return cond


def selection_from_edges(edge_index, edge_attr, batch, n_graph: int, max_elem: int) -> torch.Tensor:
    """The (B,2,E+1,E+1) selection that reproduces a reference graph: a sampled relation is never UNKNOWN, so bit 0 (size) /
    bit 4 (loc) of edge_attr clear = the kind was sampled for that pair."""
    batch = torch.as_tensor(batch).long().cpu()
    ei = torch.as_tensor(edge_index).long().cpu().reshape(2, -1)
    ea = torch.as_tensor(edge_attr).long().cpu().reshape(-1)
    first = torch.cat([batch.new_zeros(1), torch.bincount(batch, minlength=n_graph).cumsum(0)])[:-1]
    g = batch[ei[0]]
    sel = torch.zeros((n_graph, 2, max_elem + 1, max_elem + 1), dtype=torch.bool)
    i, j = ei[0] - first[g], ei[1] - first[g]
    sel[g, 0, i, j] = (ea & 1) == 0
    sel[g, 1, i, j] = (ea & 16) == 0
    return sel


def layouts_from_list(items, max_elem: int, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """[(bbox (n,4), label (n,)), ...] — the `results` / `inputs` lists of a result pickle — to dense layouts."""
    B = len(items)
    bbox = torch.zeros((B, max_elem, 4), dtype=dtype)
    label = torch.zeros((B, max_elem), dtype=torch.int64)
    mask = torch.zeros((B, max_elem), dtype=torch.bool)
    for b, (bx, lb) in enumerate(items):
        n = len(lb)
        if n > max_elem:
            raise ValueError(f"layout {b} has {n} elements, the tokenizer holds {max_elem}")
        if n:
            bbox[b, :n] = torch.as_tensor(np.asarray(bx)).reshape(n, 4).to(dtype)
            label[b, :n] = torch.as_tensor(np.asarray(lb)).reshape(n).long()
            mask[b, :n] = True
    return {"bbox": bbox, "label": label, "mask": mask}
