"""Coordinate bins from raw boxes on the GPU — what the reference's bin/clustering_coordinates.py writes with scikit-learn:
`<dataset>_max<N>_<alg>_train_clusters.pkl`, per-coordinate cluster centres for 2, 4, ... 256 bins, the file every
`bbox_quantization: kmeans` / `percentile` checkpoint needs (test_entry.GeometryTokenizer loads it).

Everything runs through libldm_hip.so (kernels_cluster.hip; rules and summation orders: csrc/ldm_cluster_core.h): a device radix
sort per coordinate, float64 prefix sums, greedy k-means++ seeding and Lloyd on the sorted array for every (coordinate, cluster
count, restart) in one batch, the reference's Percentile.fit on the distinct values.  There is no CPU fallback.

Differences from scikit-learn, all documented in the core header: own Philox draws (the distribution of sklearn's seeding, not
its stream); a point exactly on the midpoint of two centres goes to the lower one; a cluster that empties keeps its centre
(sklearn relocates it); fewer distinct values than clusters is refused (sklearn warns and returns duplicate centres).  The
models are small picklable objects with `cluster_centers_` and `predict`, not sklearn estimators.
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
import time
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch

from .binding import _stream_ptr, load_library

KEYS = ("x", "y", "w", "h")
N_CLUSTERS_LIST = tuple(2 ** i for i in range(1, 9))   # the tool's list
MAX_CLUSTERS = 256
QUANT_PERCENTILE, QUANT_KMEANS = 1, 2                    # LDM_QUANT_*
_STRIDE = 256                                            # centre rows of the C-ABI
_WORK_BUDGET = 1 << 30                                   # restarts are cut into calls whose workspace stays below this


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("layout_dm_amd.clustering needs a ROCm GPU (MI355X); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _check_k(k) -> int:
    k = int(k)
    if not 1 <= k <= MAX_CLUSTERS:
        raise ValueError(f"n_clusters must be in [1, {MAX_CLUSTERS}] (the tool's largest); got {k}")
    return k


def _tensor(X) -> torch.Tensor:
    if isinstance(X, np.ndarray) and not X.flags.writeable:
        X = X.copy()   # (torch warns about sharing memory it could write to; nothing here writes)
    return torch.as_tensor(X)


def _values(X, what: str) -> torch.Tensor:
    """(n, 1) / (n,) numpy or torch, float32 or float32-valued float64, host or device -> (n,) float32 on the GPU."""
    t = _tensor(X)
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1:
        raise ValueError(f"{what}: X must be (n, 1) or (n,); got {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"{what}: X is empty (n = 0)")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: X must be float32 or float64; got {t.dtype}")
    if t.dtype == torch.float64:   # checked where the values live, before a device is asked for: the refusals need no GPU
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{what}: X holds a NaN or an infinite value")
        f = t.float()
        if not bool((f.double() == t).all()):
            raise ValueError(f"{what}: float64 X is accepted only where every value is exactly a float32")
        t = f
    return t.to(t.device if t.is_cuda else _device()).contiguous()


class _Sorted:
    """ldm_cluster_sort of (A, n) float32 device values, with a workspace for P problems of n_init restarts."""

    def __init__(self, x: torch.Tensor, clip: bool, P: int, n_init: int, what: str):
        assert x.dim() == 2 and x.dtype == torch.float32 and x.is_cuda and x.is_contiguous()
        self.lib = load_library()
        self.dev = x.device
        self.A, self.n = int(x.shape[0]), int(x.shape[1])
        self.P, self.n_init = int(P), int(n_init)
        A, n = self.A, self.n
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.sorted = torch.empty((A, n), dtype=torch.float32, device=self.dev)
        self.ps, self.ps2, self.ps_unique = (torch.empty((A, n + 1), **f64) for _ in range(3))
        self.unique = torch.empty((A, n), dtype=torch.float32, device=self.dev)
        n_unique = torch.empty(A, dtype=torch.int64, device=self.dev)
        self.work = self._workspace(self.P, self.n_init)
        err = torch.empty(1, dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            rc = self.lib.ldm_cluster_sort(x.data_ptr(), A, n, int(bool(clip)), 3, self.sorted.data_ptr(), self.ps.data_ptr(),
                                           self.ps2.data_ptr(), self.unique.data_ptr(), self.ps_unique.data_ptr(),
                                           n_unique.data_ptr(), self.work.data_ptr(), self.work.numel(), err.data_ptr(),
                                           _stream_ptr(self.dev))
        if rc != 0:
            raise RuntimeError(f"ldm_cluster_sort failed ({rc})")
        if int(err.item()) & 1:   # (synchronises)
            raise ValueError(f"{what}: X holds a NaN or an infinite value")
        self.n_unique = [int(v) for v in n_unique.tolist()]

    def _workspace(self, P: int, n_init: int) -> torch.Tensor:
        return torch.empty(self.workspace_bytes(P, n_init), dtype=torch.uint8, device=self.dev)

    def workspace_bytes(self, P: int, n_init: int) -> int:
        need = C.c_size_t()
        if self.lib.ldm_cluster_workspace_bytes(self.A, self.n, P, n_init, C.byref(need)) != 0:
            raise ValueError(f"clustering: sizes out of range (A={self.A}, n={self.n}, problems={P}, n_init={n_init})")
        return int(need.value)

    def ensure(self, P: int, n_init: int):
        if self.workspace_bytes(P, n_init) > self.work.numel():
            self.work = self._workspace(P, n_init)


def _problem_table(problems, dev):
    """[(array, k)] -> (order that sorts them by k descending, host int32 (P,3) ctypes array, the same rows on the device).
    The problem id — a Philox counter word — is k itself: a model does not depend on what else is in its batch."""
    order = sorted(range(len(problems)), key=lambda i: -problems[i][1])
    rows = np.array([[problems[i][0], problems[i][1], problems[i][1]] for i in order], dtype=np.int32).reshape(-1, 3)
    return order, np.ascontiguousarray(rows), torch.from_numpy(rows).to(dev)


def _unsort(order, *tensors):
    inv = np.empty(len(order), dtype=np.int64)
    inv[np.asarray(order)] = np.arange(len(order))
    return [t[inv] for t in tensors]


def _kmeans_batch(s: _Sorted, problems, random_state: int, n_init: int, max_iter: int, tol: float):
    """-> centres (P, 256) float64, inertia (P) float64, n_iter (P), best restart (P): numpy, in the order of `problems`."""
    for a, k in problems:
        if s.n_unique[a] < k:
            raise ValueError(f"kmeans: {s.n_unique[a]} distinct values, fewer than n_clusters={k}")
    P = len(problems)
    order, h_prob, d_prob = _problem_table(problems, s.dev)
    per = max(1, s.workspace_bytes(P, 1) - s.workspace_bytes(0, 1))
    chunk = int(max(1, min(n_init, 64, 65535 // P, _WORK_BUDGET // per)))
    s.ensure(P, chunk)
    best = None
    with torch.cuda.device(s.dev):
        for r0 in range(0, n_init, chunk):
            cnt = min(chunk, n_init - r0)
            cen = torch.empty((P, _STRIDE), dtype=torch.float64, device=s.dev)
            ine = torch.empty(P, dtype=torch.float64, device=s.dev)
            nit, rst = (torch.empty(P, dtype=torch.int32, device=s.dev) for _ in range(2))
            rc = s.lib.ldm_kmeans1d_fit(s.sorted.data_ptr(), s.ps.data_ptr(), s.ps2.data_ptr(), s.A, s.n, h_prob.ctypes.data,
                                        d_prob.data_ptr(), P, cnt, r0, int(random_state) & (2 ** 64 - 1), int(max_iter),
                                        float(tol), cen.data_ptr(), ine.data_ptr(), nit.data_ptr(), rst.data_ptr(),
                                        s.work.data_ptr(), s.work.numel(), _stream_ptr(s.dev))
            if rc != 0:
                raise RuntimeError(f"ldm_kmeans1d_fit failed ({rc})")
            if best is None:
                best = [cen, ine, nit, rst]
            else:   # the lowest inertia, the earlier restart on a tie
                better = ine < best[1]
                best = [torch.where(better[:, None], cen, best[0])] + [torch.where(better, n_, o) for n_, o in
                                                                       zip((ine, nit, rst), best[1:])]
    return _unsort(order, *[t.cpu().numpy() for t in best])


def _lloyd_batch(s: _Sorted, problems, starts, max_iter: int, tol: float, trace: bool = False):
    """explicit start centres (one sorted float64 array of k per problem) -> centres, inertia, n_iter (+ trace (max_iter, k))"""
    P = len(problems)
    order, h_prob, d_prob = _problem_table(problems, s.dev)
    start = np.zeros((P, _STRIDE), dtype=np.float64)
    for row, i in enumerate(order):
        c = np.sort(np.asarray(starts[i], dtype=np.float64).reshape(-1))
        if c.shape != (problems[i][1],) or not np.isfinite(c).all():
            raise ValueError(f"init must hold n_clusters={problems[i][1]} finite centres; got shape {np.shape(starts[i])}")
        start[row, :c.size] = c
    s.ensure(P, 1)
    d_start = torch.from_numpy(start).to(s.dev)
    cen = torch.empty((P, _STRIDE), dtype=torch.float64, device=s.dev)
    ine = torch.empty(P, dtype=torch.float64, device=s.dev)
    nit = torch.empty(P, dtype=torch.int32, device=s.dev)
    tr = torch.full((int(max_iter), problems[0][1]), float("nan"), dtype=torch.float64, device=s.dev) if trace else None
    with torch.cuda.device(s.dev):
        rc = s.lib.ldm_kmeans1d_lloyd(s.sorted.data_ptr(), s.ps.data_ptr(), s.ps2.data_ptr(), s.A, s.n, h_prob.ctypes.data,
                                      d_prob.data_ptr(), P, d_start.data_ptr(), int(max_iter), float(tol), cen.data_ptr(),
                                      ine.data_ptr(), nit.data_ptr(), tr.data_ptr() if trace else None, s.work.data_ptr(),
                                      s.work.numel(), _stream_ptr(s.dev))
    if rc != 0:
        raise RuntimeError(f"ldm_kmeans1d_lloyd failed ({rc})")
    out = _unsort(order, cen.cpu().numpy(), ine.cpu().numpy(), nit.cpu().numpy())
    return out + [tr.cpu().numpy()] if trace else out


def _percentile_batch(s: _Sorted, problems):
    """-> centres (P, 256) float32 numpy, in the order of `problems`"""
    P = len(problems)
    order, h_prob, d_prob = _problem_table(problems, s.dev)
    s.ensure(P, 1)
    h_m = np.asarray(s.n_unique, dtype=np.int64)
    cen = torch.empty((P, _STRIDE), dtype=torch.float32, device=s.dev)
    with torch.cuda.device(s.dev):
        rc = s.lib.ldm_percentile_fit(s.ps_unique.data_ptr(), s.A, s.n, h_m.ctypes.data, h_prob.ctypes.data, d_prob.data_ptr(), P,
                                      cen.data_ptr(), s.work.data_ptr(), s.work.numel(), _stream_ptr(s.dev))
    if rc != 0:
        raise RuntimeError(f"ldm_percentile_fit failed ({rc})")
    return _unsort(order, cen.cpu().numpy())[0]


def nearest_centre(X, centres, quant: int):
    """ids of X under sorted centres through ldm_nearest_centre — the routine ldm_encode_cond quantises with.  X: (n, 1) / (n,)
    numpy or torch (cast to float32, as both tokenizer rules do); -> (n,) int64 of the same kind (numpy, or torch on X's device)."""
    t = _tensor(X)
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1:
        raise ValueError(f"predict: X must be (n, 1) or (n,); got {tuple(t.shape)}")
    src = t.device
    dev = src if t.is_cuda else _device()
    x = t.to(device=dev, dtype=torch.float32).contiguous()
    c = torch.as_tensor(np.asarray(centres, dtype=np.float64).reshape(-1)).to(dev)
    ids = torch.empty(x.numel(), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = load_library().ldm_nearest_centre(x.data_ptr(), x.numel(), c.data_ptr(), c.numel(), int(quant), ids.data_ptr(),
                                               _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_nearest_centre failed ({rc})")
    ids = ids.long().to(src)   # (synchronises: the temporaries are done with)
    return ids if isinstance(X, torch.Tensor) else ids.numpy()


class ClusterModel:
    """What the tokenizers read from a fitted model: `n_clusters`, `cluster_centers_` (k, 1) and `predict` — which takes the
    (n, 1) float32 numpy array BboxTokenizer.encode hands a model.  Plain data: pickles without scikit-learn."""

    def __init__(self, algorithm: str, cluster_centers_: np.ndarray, inertia_: Optional[float] = None, n_iter_: Optional[int] = None):
        if algorithm not in ("kmeans", "percentile"):
            raise ValueError(f"algorithm must be kmeans or percentile; got {algorithm}")
        self.algorithm = algorithm
        self.cluster_centers_ = np.asarray(cluster_centers_).reshape(-1, 1)
        self.n_clusters = int(self.cluster_centers_.shape[0])
        self.inertia_, self.n_iter_ = inertia_, n_iter_

    def predict(self, X):
        c = np.asarray(self.cluster_centers_, dtype=np.float64).reshape(-1)
        return nearest_centre(X, c, QUANT_KMEANS if self.algorithm == "kmeans" else QUANT_PERCENTILE)

    def __eq__(self, other):
        return (isinstance(other, ClusterModel) and self.algorithm == other.algorithm
                and self.cluster_centers_.dtype == other.cluster_centers_.dtype
                and np.array_equal(self.cluster_centers_, other.cluster_centers_))

    __hash__ = None


def _like(X, a: np.ndarray):
    """centres in the kind and dtype of X"""
    if isinstance(X, torch.Tensor):
        return torch.from_numpy(a).to(device=X.device, dtype=X.dtype)
    return a.astype(np.asarray(X).dtype)


class KMeans1D:
    """sklearn.cluster.KMeans(n_clusters, random_state, n_init=10) for one coordinate.  cluster_centers_ is (k, 1), sorted
    ascending (the reference sorts 1-D centres on load anyway, bbox_tokenizer.py:62-68), in the dtype of X."""

    def __init__(self, n_clusters: int = 8, random_state: int = 0, n_init: int = 10, max_iter: int = 300, tol: float = 1e-4):
        self.n_clusters, self.random_state, self.n_init = n_clusters, int(random_state), int(n_init)
        self.max_iter, self.tol = int(max_iter), float(tol)

    def fit(self, X, init=None):
        k = _check_k(self.n_clusters)
        if self.n_init < 1 or self.max_iter < 1 or not self.tol >= 0:
            raise ValueError("KMeans1D: n_init >= 1, max_iter >= 1, tol >= 0")
        x = _values(X, "KMeans1D.fit")
        s = _Sorted(x[None], False, 1, 1, "KMeans1D.fit")
        if init is None:
            cen, ine, nit, _ = _kmeans_batch(s, [(0, k)], self.random_state, self.n_init, self.max_iter, self.tol)
        else:
            if s.n_unique[0] < k:
                raise ValueError(f"kmeans: {s.n_unique[0]} distinct values, fewer than n_clusters={k}")
            cen, ine, nit = _lloyd_batch(s, [(0, k)], [init], self.max_iter, self.tol)
        self._centres64 = cen[0, :k].copy()
        self.cluster_centers_ = _like(X, self._centres64.reshape(k, 1))
        self.inertia_, self.n_iter_ = float(ine[0]), int(nit[0])
        return self

    def predict(self, X):
        if not hasattr(self, "_centres64"):
            raise NotImplementedError
        return nearest_centre(X, self._centres64, QUANT_KMEANS)

    def model(self) -> ClusterModel:
        c = self.cluster_centers_
        return ClusterModel("kmeans", c.cpu().numpy() if isinstance(c, torch.Tensor) else c, self.inertia_, self.n_iter_)


class Percentile:
    """The reference's Percentile (helpers/clustering.py): float32 centres (k, 1), -1 for an empty bin; predict is the
    percentile rule of the tokenizer (clip to [0, 1], nearest centre in float32, first minimum)."""

    def __init__(self, n_clusters: int = 32):
        self.n_clusters = n_clusters

    def fit(self, X):
        k = _check_k(self.n_clusters)
        x = _values(X, "Percentile.fit")
        s = _Sorted(x[None], True, 1, 1, "Percentile.fit")
        self.cluster_centers_ = _percentile_batch(s, [(0, k)])[0, :k].reshape(k, 1).copy()
        return self

    def predict(self, X):
        if not hasattr(self, "cluster_centers_"):
            raise NotImplementedError
        return nearest_centre(X, self.cluster_centers_, QUANT_PERCENTILE)

    def model(self) -> ClusterModel:
        return ClusterModel("percentile", self.cluster_centers_)


def fit_coordinate_bins(bboxes, algorithm: str, n_clusters_list: Sequence[int] = N_CLUSTERS_LIST, random_state: int = 0,
                        max_bbox_num: Optional[int] = None, n_init: int = 10, max_iter: int = 300, tol: float = 1e-4,
                        progress: Optional[Callable[[int, float], None]] = None) -> Dict[str, ClusterModel]:
    """bin/clustering_coordinates.py on (N, 4) boxes (xc, yc, w, h): {"x-2": model, ..., "h-256": model}.  Every coordinate is
    sorted once; all (coordinate, cluster count, restart) fits go into one batch.  max_bbox_num=None fits all boxes; a number
    subsamples the kmeans input exactly as the tool does (torch.randperm under torch.Generator().manual_seed(random_state)).
    progress(n_clusters, seconds): called per cluster count, which then is a batch of its own (the models are the same)."""
    if algorithm not in ("kmeans", "percentile"):
        raise ValueError(f"algorithm must be kmeans or percentile; got {algorithm}")
    ks = [_check_k(k) for k in n_clusters_list]
    b = _tensor(bboxes)
    if b.dim() != 2 or b.shape[1] != 4:
        raise ValueError(f"bboxes must be (N, 4); got {tuple(b.shape)}")
    if b.shape[0] == 0:
        raise ValueError("bboxes is empty (n = 0)")
    if max_bbox_num is not None and algorithm == "kmeans" and b.shape[0] > int(max_bbox_num):
        idx = torch.randperm(b.shape[0], generator=torch.Generator().manual_seed(int(random_state)))
        b = b[idx[:int(max_bbox_num)].to(b.device)]
    x = torch.stack([_values(b[:, i], "fit_coordinate_bins") for i in range(4)]).contiguous()
    kmeans = algorithm == "kmeans"
    s = _Sorted(x, not kmeans, 4 * len(ks), 1, "fit_coordinate_bins")
    models: Dict[str, ClusterModel] = {}
    for group in ([[k] for k in ks] if progress else [ks]):
        t0 = time.time()
        problems = [(a, k) for k in group for a in range(4)]
        if kmeans:
            cen, ine, nit, _ = _kmeans_batch(s, problems, random_state, n_init, max_iter, tol)
        else:
            cen = _percentile_batch(s, problems)
        for i, (a, k) in enumerate(problems):
            if kmeans:
                models[f"{KEYS[a]}-{k}"] = ClusterModel("kmeans", cen[i, :k].astype(np.float32), float(ine[i]), int(nit[i]))
            else:
                models[f"{KEYS[a]}-{k}"] = ClusterModel("percentile", cen[i, :k].copy())
        if progress:
            progress(group[0], time.time() - t0)
    return models


def clusters_file_name(dataset_name: str, max_seq_length: int, algorithm: str) -> str:
    return f"{dataset_name}_max{int(max_seq_length)}_{algorithm}_train_clusters.pkl"


def save_clusters(models: Dict[str, ClusterModel], result_dir: str, dataset_name: str, max_seq_length: int, algorithm: str) -> str:
    """Writes the file GeometryTokenizer / _find_clustering_file look for; returns its path."""
    os.makedirs(result_dir, exist_ok=True)
    path = os.path.join(result_dir, clusters_file_name(dataset_name, max_seq_length, algorithm))
    with open(path, "wb") as f:
        pickle.dump(dict(models), f, protocol=pickle.HIGHEST_PROTOCOL)
    return path


def cluster_stages(X, n_clusters: int, random_state: int = 0, restart: int = 0, max_iter: int = 300, tol: float = 1e-4,
                   want_dist: bool = False) -> Dict[str, np.ndarray]:
    """Development hook (ldm_dev_cluster_stages): one run with every stage kept, as numpy — sorted, ps, ps2; per seeding step
    unif / cand / pots (k, L_max, the first n_cand[s] valid), pick (k); dist (k, n) with want_dist (row 0 is nan); lloyd
    (n_iter, k); centres (k), inertia, n_iter."""
    k = _check_k(n_clusters)
    x = _values(X, "cluster_stages")
    n, dev = x.numel(), x.device
    if k > n:
        raise ValueError(f"cluster_stages: n_clusters={k} > n={n}")
    lib = load_library()
    need = C.c_size_t()
    if lib.ldm_cluster_workspace_bytes(1, n, 1, 1, C.byref(need)) != 0:
        raise ValueError(f"cluster_stages: sizes out of range (n={n})")
    work = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    srt = torch.empty(n, dtype=torch.float32, device=dev)
    ps, ps2 = torch.empty(n + 1, **f64), torch.empty(n + 1, **f64)
    unif, pots = torch.full((k, 7), float("nan"), **f64), torch.full((k, 7), float("nan"), **f64)
    cand = torch.full((k, 7), -1, dtype=torch.int64, device=dev)
    pick = torch.full((k,), -1, dtype=torch.int64, device=dev)
    dist = torch.full((k, n), float("nan"), **f64) if want_dist else None
    lloyd = torch.full((int(max_iter), k), float("nan"), **f64)
    cen, ine = torch.empty(_STRIDE, **f64), torch.empty(1, **f64)
    nit, err = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.ldm_dev_cluster_stages(x.data_ptr(), n, k, int(random_state) & (2 ** 64 - 1), k, int(restart), int(max_iter),
                                        float(tol), srt.data_ptr(), ps.data_ptr(), ps2.data_ptr(), unif.data_ptr(), cand.data_ptr(),
                                        pots.data_ptr(), pick.data_ptr(), dist.data_ptr() if want_dist else None, lloyd.data_ptr(),
                                        cen.data_ptr(), ine.data_ptr(), nit.data_ptr(), work.data_ptr(), work.numel(),
                                        err.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_dev_cluster_stages failed ({rc})")
    if int(err.item()) & 1:
        raise ValueError("cluster_stages: X holds a NaN or an infinite value")
    n_iter = int(nit.item())
    out = {"sorted": srt, "ps": ps, "ps2": ps2, "unif": unif, "cand": cand, "pots": pots, "pick": pick, "lloyd": lloyd[:n_iter],
           "centres": cen[:k], "inertia": ine, "n_iter": nit}
    if want_dist:
        out["dist"] = dist
    return {name: t.cpu().numpy() for name, t in out.items()}
