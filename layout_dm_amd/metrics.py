"""Alignment / overlap metrics of generated layouts on the MI355X — drop-in for `compute_alignment` / `compute_overlap`
of the reference's evaluation (trainer/helpers/metric.py:98-203; eval.py:153-155,203-205 calls them on every generated
batch and sums each entry over the layouts).

    from layout_dm_amd.metrics import compute_alignment, compute_overlap     # same signatures, same dictionary keys

Inputs are what `LayoutDM.sample` / `Engine.decode` return: `bbox` (B,S,4) (xc, yc, w, h), `mask` (B,S) bool.  Tensors
already on the device stay there (the decode kernel's output feeds the metrics kernel directly); CPU tensors are copied
over.  One launch of `layout_metrics_k` (one wavefront per layout) computes all six scores; results come back as float32
tensors on the input's device.  No CPU fallback: without the extension or a GPU this raises.

The IoU-family metrics of eval.py (metric.py:300-507; eval.py:173-176,211-215) are here too, with the reference's names:

    from layout_dm_amd.metrics import compute_average_iou, compute_maximum_iou, compute_docsim

over lists of (bbox ndarray, label ndarray) layouts, plus tensor forms `average_iou(bbox, mask)` and
`docsim(bbox_gt, label_gt, mask_gt, bbox_gen, label_gen, mask_gen)` for what Engine.decode leaves on the device.

The relation violation score the sampling entry point computes after every cond=relation batch (metric.py:62-95;
test.py:230-254) is `compute_violation(bbox_flatten, data)`, with `relation_violation(bbox, mask, data)` for the dense
output of Engine.decode and `relation_detect(bbox_flatten, data)` for the per-edge detections.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from .binding import _stream_ptr, load_library

KEYS = ("alignment-ACLayoutGAN", "alignment-LayoutGAN++", "alignment-NDN",
        "overlap-ACLayoutGAN", "overlap-LayoutGAN++", "overlap-LayoutGAN")


def layout_metrics(bbox: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(B,6) float32 on the GPU: the six scores of every layout in the order of KEYS (ldm_layout_metrics)."""
    if not torch.cuda.is_available():
        raise RuntimeError("layout_dm_amd.metrics needs a ROCm GPU (MI355X); there is no CPU path")
    lib = load_library()
    dev = bbox.device if bbox.is_cuda else torch.device("cuda", torch.cuda.current_device())
    b = bbox.to(device=dev, dtype=torch.float32).contiguous()
    m = mask.to(device=dev, dtype=torch.uint8).contiguous()
    if b.dim() != 3 or b.shape[-1] != 4 or m.shape != b.shape[:2]:
        raise ValueError(f"bbox must be (B,S,4) and mask (B,S); got {tuple(bbox.shape)}, {tuple(mask.shape)}")
    B, S = m.shape
    out = torch.empty((B, len(KEYS)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.ldm_layout_metrics(b.data_ptr(), m.data_ptr(), B, S, out.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_layout_metrics failed ({rc}): 1 <= S <= 256 elements per layout" if rc == -1
                           else f"ldm_layout_metrics failed ({rc})")
    torch.cuda.current_stream(dev).synchronize()   # (b / m may be temporaries)
    return out


def _as_dict(out: torch.Tensor, lo: int, like: torch.Tensor) -> Dict[str, torch.Tensor]:
    out = out if like.is_cuda else out.cpu()
    return {k: out[:, lo + i].contiguous() for i, k in enumerate(KEYS[lo:lo + 3])}


def compute_alignment(bbox: torch.Tensor, mask: torch.Tensor) -> Dict[str, torch.Tensor]:
    """helpers/metric.py:98-149."""
    return _as_dict(layout_metrics(bbox, mask), 0, bbox)


def compute_overlap(bbox: torch.Tensor, mask: torch.Tensor) -> Dict[str, torch.Tensor]:
    """helpers/metric.py:152-203."""
    return _as_dict(layout_metrics(bbox, mask), 3, bbox)


# ------------------------------------------------------------------------------------------------------------------------
# Average IoU, Max-IoU and DocSim (helpers/metric.py:300-507; eval.py:173-176,211-215): drop-ins with the reference's names,
# signatures and return types over what test.py pickles, `layouts` = [(bbox ndarray (n,4) xc yc w h, label ndarray (n,))].
# The kernels (kernels_eval_iou.hip) compute in float64 if a layout set is float64 (LayoutDM's kmeans decode) and in float32
# otherwise (the dataset side), like numpy.  `disable_parallel` / `n_jobs` are accepted and ignored.  No CPU fallback.

EVAL_MAX_ELEMENTS = 32   # elements per layout (the reference's datasets have <= 25)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("layout_dm_amd.metrics needs a ROCm GPU (MI355X); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _set_dtype(layouts) -> np.dtype:
    return np.dtype(np.float64) if any(np.asarray(b).dtype == np.float64 for b, _ in layouts) else np.dtype(np.float32)


def _pack(layouts, S: int, dtype, order=None):
    """(R,S,4) boxes, (R,S) int64 labels, (R,) int32 counts, elements first in their rows (sorted stably by label if order)"""
    R = len(layouts)
    box = np.zeros((R, S, 4), dtype)
    lab = np.zeros((R, S), np.int64)
    n = np.zeros(R, np.int32)
    for r, (b, l) in enumerate(layouts):
        b, l = np.asarray(b).reshape(-1, 4), np.asarray(l).reshape(-1)
        if order:
            o = np.argsort(l, kind="stable")
            b, l = b[o], l[o]
        k = len(l)
        box[r, :k], lab[r, :k], n[r] = b, l, k
    return box, lab, n


def _check_elements(S: int):
    if S > EVAL_MAX_ELEMENTS:
        raise ValueError(f"at most {EVAL_MAX_ELEMENTS} elements per layout (got {S})")


def average_iou(bbox: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(B,2) float64 on the GPU: {BLT, VTN} average IoU of every layout (ldm_eval_average_iou).  bbox (B,S,4) float32 or
    float64 (xc, yc, w, h) as Engine.decode / LayoutDM.sample leave them, mask (B,S) bool; device tensors stay there."""
    dev = bbox.device if bbox.is_cuda else _device()
    if bbox.dim() != 3 or bbox.shape[-1] != 4 or tuple(mask.shape) != tuple(bbox.shape[:2]):
        raise ValueError(f"bbox must be (B,S,4) and mask (B,S); got {tuple(bbox.shape)}, {tuple(mask.shape)}")
    f64 = bbox.dtype == torch.float64
    b = bbox.to(device=dev, dtype=torch.float64 if f64 else torch.float32).contiguous()
    m = mask.to(device=dev, dtype=torch.uint8).contiguous()
    B, S = m.shape
    _check_elements(S)
    out = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    lib = load_library()
    with torch.cuda.device(dev):
        rc = lib.ldm_eval_average_iou(b.data_ptr(), int(f64), m.data_ptr(), B, max(S, 1), out.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_eval_average_iou failed ({rc})")
    torch.cuda.current_stream(dev).synchronize()
    return out


def compute_average_iou(layouts, disable_parallel: bool = True, n_jobs=None) -> Dict[str, float]:
    """helpers/metric.py:374-431."""
    S = max([len(l) for _, l in layouts] + [1])
    _check_elements(S)
    box, _, n = _pack(layouts, S, _set_dtype(layouts))
    mask = np.arange(S)[None, :] < n[:, None]
    out = average_iou(torch.from_numpy(box), torch.from_numpy(mask)).cpu().numpy()
    return {"average_iou-BLT": np.array(out[:, 0]).mean().item(), "average_iou-VTN": np.array(out[:, 1]).mean().item()}


def _docsim_launch(dev, b1, l1, n1, b2, l2, n2) -> torch.Tensor:
    B, S = l1.shape
    _check_elements(S)
    out = torch.zeros(B, dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = load_library()
    with torch.cuda.device(dev):
        rc = lib.ldm_eval_docsim(b1.data_ptr(), int(b1.dtype == torch.float64), l1.data_ptr(), n1.data_ptr(), b2.data_ptr(),
                                 int(b2.dtype == torch.float64), l2.data_ptr(), n2.data_ptr(), B, max(S, 1), out.data_ptr(),
                                 err.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_eval_docsim failed ({rc})")
    if int(err.item()) != 0:
        raise ValueError("DocSim: the similarity matrix contains invalid numeric entries (NaN / inf boxes)")
    return out


def _compact(bbox: torch.Tensor, label: torch.Tensor, mask: torch.Tensor, dev):
    """valid elements first in each row, in their order (a stable sort of ~mask on the device), + counts"""
    m = mask.to(device=dev, dtype=torch.bool)
    o = torch.sort((~m).to(torch.uint8), dim=1, stable=True).indices
    b = torch.gather(bbox.to(dev), 1, o[..., None].expand(-1, -1, 4))
    f64 = bbox.dtype == torch.float64
    return (b.to(torch.float64 if f64 else torch.float32).contiguous(),
            torch.gather(label.to(device=dev, dtype=torch.int64), 1, o).contiguous(), m.sum(1).to(torch.int32).contiguous())


def docsim(bbox_gt, label_gt, mask_gt, bbox_gen, label_gen, mask_gen) -> torch.Tensor:
    """(B,) float64 on the GPU: DocSim of every (gt[b], generated[b]) pair (ldm_eval_docsim), from padded tensors
    (B,S,4) / (B,S) / (B,S) bool such as Engine.decode leaves them; both sides must have the same B and S."""
    dev = bbox_gen.device if bbox_gen.is_cuda else _device()
    if bbox_gt.shape != bbox_gen.shape or bbox_gt.dim() != 3 or bbox_gt.shape[-1] != 4:
        raise ValueError(f"both sides must be (B,S,4); got {tuple(bbox_gt.shape)}, {tuple(bbox_gen.shape)}")
    a, b = _compact(bbox_gt, label_gt, mask_gt, dev), _compact(bbox_gen, label_gen, mask_gen, dev)
    return _docsim_launch(dev, a[0], a[1], a[2], b[0], b[1], b[2])


def compute_docsim(layouts_gt, layouts_generated, disable_parallel: bool = True, n_jobs=None):
    """helpers/metric.py:458-507: the mean over zip(layouts_gt, layouts_generated) of the per-pair DocSim (np.float64)."""
    pairs = list(zip(layouts_gt, layouts_generated))
    if not pairs:
        return np.array([]).mean()
    g, h = [p[0] for p in pairs], [p[1] for p in pairs]
    S = max([len(l) for _, l in g + h] + [1])
    _check_elements(S)
    dev = _device()
    b1, l1, n1 = (torch.from_numpy(x).to(dev) for x in _pack(g, S, _set_dtype(g)))
    b2, l2, n2 = (torch.from_numpy(x).to(dev) for x in _pack(h, S, _set_dtype(h)))
    return np.array(_docsim_launch(dev, b1, l1, n1, b2, l2, n2).cpu().numpy()).mean()


def _groups(layouts):
    g = {}
    for i, (_, l) in enumerate(layouts):
        g.setdefault(tuple(sorted(np.asarray(l).reshape(-1).tolist())), []).append(i)
    return g


def max_iou_pair_scores(layouts_1, layouts_2):
    """Max-IoU pair scores of every group of layouts that share a label multiset, in ONE launch (ldm_eval_max_iou_pairs).
    Returns [(key, n1, n2, scores (n1 * n2,) float64 in the reference's flat order: set-2 index outer)], groups ordered by
    first appearance in layouts_1."""
    g1, g2 = _groups(layouts_1), _groups(layouts_2)
    keys = [k for k in g1 if k in g2]
    if not keys:
        return []
    if any(len(k) == 0 for k in keys):
        raise ZeroDivisionError("float division by zero")   # the reference divides by the element count of empty layouts
    S = max(len(k) for k in keys)
    _check_elements(S)
    max_seg = max(max(np.unique(np.asarray(k), return_counts=True)[1]) for k in keys)
    rows1 = [i for k in keys for i in g1[k]]
    rows2 = [i for k in keys for i in g2[k]]
    table, f1, f2, off = [], 0, 0, 0
    for k in keys:
        n1, n2 = len(g1[k]), len(g2[k])
        table.append((f1, n1, f2, n2, len(k), off))
        f1, f2, off = f1 + n1, f2 + n2, off + n1 * n2
    dev = _device()
    s1, s2 = [layouts_1[i] for i in rows1], [layouts_2[i] for i in rows2]
    b1, l1, _ = _pack(s1, S, _set_dtype(s1), order=True)
    b2, _, _ = _pack(s2, S, _set_dtype(s2), order=True)
    b1, l1, b2 = (torch.from_numpy(x).to(dev) for x in (b1, l1, b2))
    gt = torch.tensor(table, dtype=torch.int64, device=dev)
    out = torch.empty(off, dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = load_library()
    with torch.cuda.device(dev):
        rc = lib.ldm_eval_max_iou_pairs(b1.data_ptr(), int(b1.dtype == torch.float64), l1.data_ptr(), len(rows1), b2.data_ptr(),
                                        int(b2.dtype == torch.float64), len(rows2), S, gt.data_ptr(), len(table), off,
                                        int(max_seg), out.data_ptr(), err.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_eval_max_iou_pairs failed ({rc})")
    e = int(err.item())
    if e & 1:
        raise ValueError("Max-IoU: an IoU matrix contains invalid numeric entries (NaN: two zero-area boxes)")
    if e:
        raise RuntimeError(f"ldm_eval_max_iou_pairs: device error flags {e}")
    out = out.cpu().numpy()
    return [(k, t[1], t[3], out[t[5]:t[5] + t[1] * t[3]]) for k, t in zip(keys, table)]


def compute_maximum_iou(layouts_1, layouts_2, disable_parallel: bool = True, n_jobs=None) -> float:
    """helpers/metric.py:317-371: pair scores on the device, each group's assignment by scipy on the host (as the reference)."""
    from scipy.optimize import linear_sum_assignment

    chosen = []
    for _, n1, n2, s in max_iou_pair_scores(layouts_1, layouts_2):
        scores = s.reshape(n1, n2)
        ii, jj = linear_sum_assignment(scores, maximize=True)
        chosen.append(scores[ii, jj])
    if not chosen:
        return 0.0
    scores = np.concatenate(chosen)
    return 0.0 if len(scores) == 0 else scores.mean().item()


# ------------------------------------------------------------------------------------------------------------------------
# Relation violation score (helpers/metric.py:62-95, called at test.py:230-254 after every cond=relation batch).  `data` is
# cond["batch_w_canvas"]: anything with y, edge_index, edge_attr, batch — a PyG batch, or a dict (relation.graph_to_csr).
# One wavefront per layout walks the layout's edges (kernels_violation.hip); float32 or float64 boxes.  No CPU fallback.

def _violation_graph(data, dev):
    """the device arrays ldm_relation_violation* take: (n_graph, n_edge, n_nodes, canvas, off, src, dst, attr, first, order)"""
    from .relation import graph_to_csr

    get = (lambda k: data[k]) if isinstance(data, dict) else (lambda k: getattr(data, k))
    batch = torch.as_tensor(get("batch"))
    if batch.numel() == 0:
        raise ValueError("compute_violation: empty batch")
    n_graph = int(batch.max()) + 1
    off, src, dst, attr, first, order = graph_to_csr(data, n_graph, with_nodes=True)
    y = torch.as_tensor(get("y")).reshape(-1)
    if y.numel() != batch.numel():
        raise ValueError("y / batch length mismatch")
    canvas = y.eq(0).to(device=dev, dtype=torch.uint8).contiguous()
    arrays = [t.to(dev).contiguous() for t in (off, src, dst, attr, first)]
    return (n_graph, int(src.numel()), int(y.numel()), canvas, *arrays, order)


def _out_device(data):
    get = data.get if isinstance(data, dict) else (lambda k: getattr(data, k, None))
    x = get("x")   # the reference: data.x.device; a graph without boxes answers where its labels live
    return x.device if isinstance(x, torch.Tensor) else torch.as_tensor(get("y")).device


def _violation_launch(dense, dev, b, mask, data, per_edge: bool):
    n_graph, E, n_nodes, canvas, off, src, dst, attr, first, order = _violation_graph(data, dev)
    out = torch.empty(n_graph, dtype=torch.float32, device=dev)
    edge = torch.empty((E, 3), dtype=torch.int32, device=dev) if per_edge else None
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    graph = (canvas.data_ptr(), n_nodes, off.data_ptr(), src.data_ptr(), dst.data_ptr(), attr.data_ptr(), first.data_ptr(),
             n_graph, E, out.data_ptr(), edge.data_ptr() if per_edge else None, err.data_ptr(), _stream_ptr(dev))
    lib = load_library()
    f64 = int(b.dtype == torch.float64)
    with torch.cuda.device(dev):
        if dense:
            B, S = mask.shape
            if n_graph > B:
                raise ValueError(f"the graph names {n_graph} layouts, bbox holds {B}")
            rows = torch.empty(B + 1, dtype=torch.int32, device=dev)
            name = "ldm_relation_violation_dense"
            rc = lib.ldm_relation_violation_dense(b.data_ptr(), f64, mask.data_ptr(), B, S, rows.data_ptr(), *graph)
        else:
            name = "ldm_relation_violation"
            rc = lib.ldm_relation_violation(b.data_ptr(), f64, b.shape[0], *graph)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc})")
    e = int(err.item())   # (synchronises: the temporaries above are done with)
    if e & 1:
        raise IndexError("compute_violation: an edge names a node beyond the flattened boxes (the generated masks hold "
                         "fewer elements than the relation graph expects)")
    if e:
        raise ValueError("compute_violation: malformed relation graph")
    return out, edge, order


def _flat_boxes(bbox_flatten: torch.Tensor, dev):
    if bbox_flatten.dim() != 2 or bbox_flatten.shape[-1] != 4:
        raise ValueError(f"bbox_flatten must be (rows,4); got {tuple(bbox_flatten.shape)}")
    dt = torch.float64 if bbox_flatten.dtype == torch.float64 else torch.float32
    return bbox_flatten.to(device=dev, dtype=dt).contiguous()


def compute_violation(bbox_flatten: torch.Tensor, data) -> torch.Tensor:
    """helpers/metric.py:62-95: float32 (batch.max() + 1,) failures / valid per layout (NaN where no relation is known), on
    data.x.device (the graph's device).  bbox_flatten (rows,4) = bbox_c[mask_c] of test.py:232-250, indexed by the graph's global node ids."""
    dev = bbox_flatten.device if bbox_flatten.is_cuda else _device()
    out, _, _ = _violation_launch(False, dev, _flat_boxes(bbox_flatten, dev), None, data, False)
    return out.to(_out_device(data))


def relation_violation(bbox: torch.Tensor, mask: torch.Tensor, data) -> torch.Tensor:
    """compute_violation on the dense output of Engine.decode / LayoutDM.sample — bbox (B,S,4), mask (B,S) — without
    building bbox_c[mask_c]: the canvas row in front of every layout and the flattening by mask (test.py:232-250) happen in
    the kernel.  Inputs and the float32 (batch.max() + 1,) result stay on the device."""
    dev = bbox.device if bbox.is_cuda else _device()
    if bbox.dim() != 3 or bbox.shape[-1] != 4 or tuple(mask.shape) != tuple(bbox.shape[:2]) or 0 in mask.shape:
        raise ValueError(f"bbox must be (B,S,4) and mask (B,S), B, S >= 1; got {tuple(bbox.shape)}, {tuple(mask.shape)}")
    dt = torch.float64 if bbox.dtype == torch.float64 else torch.float32
    out, _, _ = _violation_launch(True, dev, bbox.to(device=dev, dtype=dt).contiguous(),
                                  mask.to(device=dev, dtype=torch.uint8).contiguous(), data, False)
    return out


def relation_detect(bbox_flatten: torch.Tensor, data):
    """Per edge, in edge_index's order: (size_code, loc_code, failure) int32 tensors on the device — what
    detect_size_relation / detect_loc_relation (data/util.py:33-69, RelSize 1..3, RelLoc 5..9) say about the boxes, and how
    many of the relations edge_attr knows they break (0..2)."""
    dev = bbox_flatten.device if bbox_flatten.is_cuda else _device()
    _, edge, order = _violation_launch(False, dev, _flat_boxes(bbox_flatten, dev), None, data, True)
    back = torch.empty_like(edge)
    back[order.to(dev)] = edge
    return back[:, 0].contiguous(), back[:, 1].contiguous(), back[:, 2].contiguous()
