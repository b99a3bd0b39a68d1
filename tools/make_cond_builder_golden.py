"""Writes tests/golden/cond_builder/reference.npz: the reference's own `LayoutSequenceTokenizer.encode` and `get_cond`
(trainer/helpers/layout_tokenizer.py:208-253, helpers/bbox_tokenizer.py:84-115, helpers/task.py:27-151) and its relation
transforms (data/util.py:111-177) on synthetic layouts, with their inputs and the randomness they drew, for
tests/test_cond_builder_fixture.py.

    python tools/make_cond_builder_golden.py     # needs the reference tree (oracle.ref_harness.install_stubs())

Per dataset (rico25: 25 categories, publaynet: 5) and box precision (f32, f64), 64 layouts of 1 - 25 elements (every size
occurs; the reference's collate cannot represent a 0-element layout), the first layouts' boxes replaced by linear-bin
boundaries — k/32 +- 1 ulp, products k + 0.5 (half to even), values < 0, > 1, exactly 0 / 1, w / h below d:
  * enc_*       tokenizer.encode
  * c_* cwh_*   get_cond
  * partial_*   get_cond after random.seed(s) / torch.manual_seed(s); the keep mask is the returned cond["mask"]
  * ref_*       get_cond(model_type="LayoutDM") after torch.manual_seed(s); the noise is torch.normal after the same seed again
                (get_cond's first draw)
  * rel_*       a second batch through AddCanvasElement + AddRelationConstraints (boxes left as drawn, so that the graph belongs
                to them), then get_cond; the selection is recoverable from edge_attr (a sampled relation is never UNKNOWN)
percentile / kmeans (rico25 geometry): Percentile and sklearn KMeans fitted on synthetic coordinates, handed to the reference's
BboxTokenizer through a temporary pickle and the KMEANS_WEIGHT_ROOT name of trainer.helpers.bbox_tokenizer (in memory; nothing
is written into the reference tree).  kmeans inputs: set A re-drawn until nothing lies within 1e-5 of a midpoint of adjacent
centres (asserted: sklearn's predict == the nearest centre by |float32(x) - c| in float64); set B at midpoints +- {0, 1, 2} ulp.
Also, for the record only: seconds the reference's get_cond takes for 512 layouts per cond type on the machine that ran this
tool, and its core count.  Only data: no program text."""
from __future__ import annotations

import os
import pickle
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "cond_builder", "reference.npz")
SEED = 20261017
N_CATEGORY = {"rico25": 25, "publaynet": 5}
PRECISIONS = ("f32", "f64")
DTYPE = {"f32": np.float32, "f64": np.float64}
B, E, N_BIN = 64, 25, 32


def boundary_values(T):
    T = np.dtype(T).type
    d = T(1.0 / N_BIN)
    vals = []
    for k in range(N_BIN + 1):
        v = T(k / N_BIN)
        vals += [v, np.nextafter(v, T(2)), np.nextafter(v, T(-1))]
        h = T((k + 0.5) / N_BIN)
        vals += [h, np.nextafter(h, T(2)), np.nextafter(h, T(-1)), T(h + d)]
    vals += [T(-0.5), T(-1e-9), T(0.0), T(1.0), T(1.5), T(1e9), T(d / 2), T(d / 3), np.nextafter(d, T(-1)), T(1 - d), T(1e-30)]
    v = np.asarray(vals, T)
    return np.stack([v, v[::-1], np.roll(v, 7), np.roll(v[::-1], 3)], axis=1)


def make_batch(n_category, seed, T, relation):
    """64 layouts as one collated batch in dtype T; sizes: a permutation in which every size 1..25 occurs"""
    import torch

    from oracle import ref_harness as rh

    rh.install_stubs()
    from trainer.data.util import AddCanvasElement, AddRelationConstraints

    g = torch.Generator().manual_seed(seed)
    sizes = list(range(1, E + 1)) + torch.randint(1, E + 1, (B - E,), generator=g).tolist()
    sizes = [sizes[i] for i in torch.randperm(B, generator=g).tolist()]
    tf = [AddCanvasElement(), AddRelationConstraints(seed=seed, edge_ratio=0.1)] if relation else []
    bnd = torch.from_numpy(boundary_values(T))
    at, datas = 0, []
    for n in sizes:
        box = torch.rand(n, 4, generator=g) * torch.tensor([0.8, 0.8, 0.5, 0.5]) + torch.tensor([0.1, 0.1, 0.05, 0.05])
        box = box.to(torch.from_numpy(np.zeros(1, T)).dtype)
        if not relation and at < len(bnd):
            k = min(n, len(bnd) - at)
            box[:k] = bnd[at:at + k]
            at += k
        lab = torch.randint(0, n_category, (n,), generator=g)
        d = rh.Data(box, lab, {"has_canvas_element": torch.tensor([False]), "filtered": False, "NoiseAdded": False})
        for t in tf:
            d = t(d)
        datas.append(d)
    assert relation or at == len(bnd)
    return rh.DataBatch(datas)


def tokenizer_for(dataset, quant="linear"):
    from oracle import ref_harness as rh

    rh.install_stubs()
    from trainer.helpers.layout_tokenizer import LayoutSequenceTokenizer

    data_cfg, dataset_cfg, _ = rh.make_cfgs(dataset)
    data_cfg["bbox_quantization"] = quant
    return LayoutSequenceTokenizer(data_cfg, dataset_cfg)


def reference_conds(dataset, prec, seed):
    import torch

    from oracle import ref_harness as rh

    rh.install_stubs()
    from trainer.data.util import sparse_to_dense
    from trainer.helpers.task import get_cond

    tok = tokenizer_for(dataset)
    T = DTYPE[prec]
    out = {}
    batch = make_batch(N_CATEGORY[dataset], seed, T, relation=False)
    out["x"], out["y"], out["batch"] = batch.x.numpy(), batch.y.numpy().astype(np.int16), batch.batch.numpy().astype(np.int16)
    assert out["x"].dtype == T
    bbox, label, _, mask = sparse_to_dense(batch)
    assert bbox.shape[1] == E
    enc = tok.encode({"label": label, "mask": mask, "bbox": bbox})
    out["enc_seq"], out["enc_mask"] = enc["seq"].numpy().astype(np.int16), enc["mask"].numpy()
    for ct in ("c", "cwh", "partial", "refinement"):
        random.seed(seed)
        torch.manual_seed(seed)
        cond = get_cond(batch, tok, ct, "LayoutDM")
        p = "ref" if ct == "refinement" else ct
        out[f"{p}_seq"], out[f"{p}_mask"] = cond["seq"].numpy().astype(np.int16), cond["mask"].numpy()
        out[f"{p}_keys"] = np.asarray(sorted(cond))
        if "num_element" in cond:
            out[f"{p}_num_element"] = cond["num_element"].numpy().astype(np.int16)
        if ct == "refinement":
            out["ref_seq_orig"] = cond["seq_orig"].numpy().astype(np.int16)
            torch.manual_seed(seed)
            out["ref_noise"] = torch.normal(0, std=0.1, size=bbox.size()).numpy()
            assert out["ref_noise"].dtype == np.float32
    rb = make_batch(N_CATEGORY[dataset], seed + 1, T, relation=True)
    cond = get_cond(rb, tok, "relation", "LayoutDM")
    out["rel_x"], out["rel_y"], out["rel_batch"] = rb.x.numpy(), rb.y.numpy().astype(np.int16), rb.batch.numpy().astype(np.int16)
    assert out["rel_x"].dtype == T
    out["rel_edge_index"], out["rel_edge_attr"] = rb.edge_index.numpy().astype(np.int32), rb.edge_attr.numpy().astype(np.int16)
    out["rel_seq"], out["rel_mask"] = cond["seq"].numpy().astype(np.int16), cond["mask"].numpy()
    out["rel_num_element"] = cond["num_element"].numpy().astype(np.int16)
    out["rel_keys"] = np.asarray(sorted(cond))
    return out


def clustering_cases(seed):
    """percentile and kmeans through the reference's BboxTokenizer with models fitted here"""
    import torch
    from sklearn.cluster import KMeans

    from oracle import ref_harness as rh

    rh.install_stubs()
    import trainer.helpers.bbox_tokenizer as bt
    from trainer.helpers.clustering import Percentile

    rng = np.random.default_rng(seed)
    fit = {"x": rng.beta(2, 2, 4000), "y": rng.beta(1.5, 3, 4000), "w": rng.beta(1.2, 4, 4000), "h": rng.beta(1.1, 6, 4000)}
    out = {}
    old = bt.KMEANS_WEIGHT_ROOT
    with tempfile.TemporaryDirectory() as tmp:
        bt.KMEANS_WEIGHT_ROOT = tmp
        try:
            for quant in ("percentile", "kmeans"):
                models = {}
                for k, v in fit.items():
                    X = v.reshape(-1, 1).astype(np.float32)
                    models[f"{k}-{N_BIN}"] = Percentile(n_clusters=N_BIN).fit(X) if quant == "percentile" else \
                        KMeans(n_clusters=N_BIN, random_state=0, n_init=1).fit(X)
                with open(os.path.join(tmp, f"rico25_max25_{quant}_train_clusters.pkl"), "wb") as f:
                    pickle.dump(models, f)
                tok = bt.BboxTokenizer(N_BIN, "c-x-y-w-h", "x-y-w-h", quant, "rico25_max25")
                cs = np.stack([np.asarray(tok.clustering_models[f"{k}-{N_BIN}"].cluster_centers_, np.float64).reshape(-1) for k in "xywh"])
                assert (np.diff(cs, axis=1) >= 0).all()
                out[f"{quant}_centres"] = cs
                mids = (cs[:, :-1] + cs[:, 1:]) / 2
                n = 20 * E
                while True:     # set A: away from every midpoint
                    a = rng.random((n, 4)).astype(np.float32) * 1.2 - 0.1
                    if quant == "percentile" or all(np.abs(a[:, k].astype(np.float64)[:, None] - mids[k][None]).min() > 1e-5 for k in range(4)):
                        break
                a = a.reshape(-1, E, 4)
                ia = tok.encode(torch.from_numpy(a)).numpy()
                out[f"{quant}_a_box"], out[f"{quant}_a_idx"] = a, ia.astype(np.int16)
                ia64 = tok.encode(torch.from_numpy(a.astype(np.float64))).numpy()
                assert np.array_equal(ia, ia64)
                if quant == "kmeans":
                    flat = a.reshape(-1, 4)
                    for k in range(4):
                        rule = np.argmin(np.abs(flat[:, k].astype(np.float64)[:, None] - cs[k][None]), axis=1) + k * N_BIN
                        assert np.array_equal(rule, ia.reshape(-1, 4)[:, k]), "sklearn's predict differs from the documented rule on set A"
                    b = np.zeros((5 * (N_BIN - 1), 4), np.float32)     # set B: midpoints +- {0, 1, 2} ulp
                    for k in range(4):
                        m = np.repeat(mids[k].astype(np.float32), 5)
                        for u in range(5):
                            v = m[u::5].copy()
                            for _ in range(abs(u - 2)):
                                v = np.nextafter(v, np.float32(2 if u > 2 else -1))
                            m[u::5] = v
                        b[:, k] = m
                    pad = (-len(b)) % E
                    b = np.concatenate([b, np.full((pad, 4), 0.5, np.float32)]).reshape(-1, E, 4)
                    out["kmeans_b_box"] = b
                    out["kmeans_b_idx"] = tok.encode(torch.from_numpy(b)).numpy().astype(np.int16)
        finally:
            bt.KMEANS_WEIGHT_ROOT = old
    return out


def timings(seed):
    import torch

    from oracle import ref_harness as rh

    rh.install_stubs()
    from trainer.helpers.task import get_cond

    tok = tokenizer_for("rico25")
    secs = []
    for ct in ("c", "cwh", "partial", "refinement", "relation"):
        t0 = time.perf_counter()   # relation: the transforms are where the reference spends its time
        batch = rh.synth_layout_batch(25, 512, seed=seed, relation=ct == "relation", n_lo=1, n_hi=25)
        t1 = time.perf_counter()
        get_cond(batch, tok, ct, "LayoutDM")
        t2 = time.perf_counter()
        secs.append((t2 - t1) + ((t1 - t0) if ct == "relation" else 0.0))
    return np.asarray(secs, np.float64)


def compute(with_timings=True):
    out = {"seed": np.int64(SEED)}
    for i, ds in enumerate(N_CATEGORY):
        for j, p in enumerate(PRECISIONS):
            for k, v in reference_conds(ds, p, SEED + 10 * i).items():
                out[f"{ds}_{p}_{k}"] = v
    out.update(clustering_cases(SEED))
    if with_timings:
        out["ref_get_cond_seconds_512"] = timings(SEED)
        out["ref_get_cond_cores"] = np.int64(os.cpu_count() or 0)
    return out


def main():
    out = compute()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    print("reference get_cond, 512 layouts (c, cwh, partial, refinement, relation incl. transforms):", out["ref_get_cond_seconds_512"])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
