"""Writes tests/golden/clustering/reference.npz: what the coordinate-bin fits (layout_dm_amd/clustering.py) are held to.

CPU only.  Needs the reference tree ($LAYOUTDM_REFERENCE, for its own Percentile: trainer.helpers.clustering is imported
untouched) and scikit-learn (written with 1.7.2).  Nothing of either is copied: the file holds inputs and recorded results.

  (a) pct_*   Percentile.fit: inputs and the reference's centres for n in {1, 5, 40, 257, 5000} x k in {2, 32, 256} on continuous
              and on 1/360-grid data (values outside [0, 1] included; most bins are empty at small n), and per case the largest
              float32-ulp distance between the reference's centre and float32(fsum(values) / count).
  (b) lloyd_* explicit-start Lloyd: float32-valued data handed to sklearn as float64, KMeans(init=c0, n_init=1,
              algorithm="lloyd", tol=0, max_iter=M), M in {1, 5, 300}, (n, k) in {(257, 4), (1000, 32), (5000, 128), (20000, 256)}:
              centres, inertia, n_iter.  A case is re-drawn until the numpy restatement below (sorted boundaries at float64
              midpoints, x <= midpoint to the lower cluster) meets no point within 1e-9 of a midpoint in any iteration and no
              empty cluster, and agrees with sklearn to 1e-12 — so the differences documented in ldm_cluster_core.h (exact ties,
              empty clusters) are not in play.
  (c) full_*  sklearn KMeans(n_clusters=k, n_init=10, random_state=s).inertia_ for s = 0..19 on three data sets (continuous, grid,
              layout-like mixture; n = 5000, float32-valued, fitted as float64) x k in {4, 32, 128}: min and max, and the global
              1-D optimum by dynamic programming over the sorted data.
"""
import argparse
import math
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "clustering", "reference.npz")
PCT_N, PCT_K = (1, 5, 40, 257, 5000), (2, 32, 256)
LLOYD_M, LLOYD_NK = (1, 5, 300), ((257, 4), (1000, 32), (5000, 128), (20000, 256))
FULL_K, FULL_SEEDS, FULL_N = (4, 32, 128), 20, 5000


def ulp_distance(a, b):
    """distance in float32 ulps between two float32 arrays of the same sign pattern"""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def percentile_cases(Percentile, rng):
    out = {}
    for kind in ("cont", "grid"):
        for n in PCT_N:
            x = rng.normal(0.5, 0.4, n).astype(np.float32)          # about a tenth falls outside [0, 1] on either side
            if kind == "grid":
                x = (np.round(x * 360) / 360).astype(np.float32)
            if n >= 40:
                x[:3] = (-0.25, 1.5, 1.0)
            out[f"pct_{kind}_{n}_x"] = x
            for k in PCT_K:
                ref = Percentile(n_clusters=k).fit(x.reshape(-1, 1)).cluster_centers_[:, 0]
                assert ref.dtype == np.float32
                # membership as the reference computes it, the mean exactly
                X = np.sort(np.unique(x.clip(0.0, 1.0)))
                thr = [X[int(t * len(X))] for t in np.linspace(0.0, 1.0, k + 1)[:-1]]
                ids = (thr <= X.reshape(-1, 1)).sum(axis=1) - 1
                worst = 0
                for i in range(k):
                    v = X[ids == i]
                    assert (len(v) == 0) == (ref[i] == -1.0)
                    if len(v):
                        exact = np.float32(math.fsum(float(t) for t in v) / len(v))
                        worst = max(worst, int(ulp_distance(ref[i], exact)))
                out[f"pct_{kind}_{n}_{k}_centres"] = ref
                out[f"pct_{kind}_{n}_{k}_ulp"] = np.int64(worst)
    return out


def lloyd_numpy(x, c0, max_iter):
    """the restatement: -> (centres, n_iter, inertia, closest |x - midpoint| met, an empty cluster met)"""
    x = np.sort(x.astype(np.float64))
    ps = np.concatenate([[0.0], np.cumsum(x)])
    c = np.sort(c0.astype(np.float64))
    prev, closest, empty, n_iter = None, np.inf, False, 0
    for it in range(max_iter):
        mid = (c[:-1] + c[1:]) / 2
        b = np.concatenate([[0], np.searchsorted(x, mid, side="right"), [len(x)]])
        near = np.searchsorted(x, mid)
        for off in (-1, 0):
            j = np.clip(near + off, 0, len(x) - 1)
            closest = min(closest, float(np.abs(x[j] - mid).min()))
        cnt = np.diff(b)
        empty |= bool((cnt == 0).any())
        new = np.where(cnt > 0, (ps[b[1:]] - ps[b[:-1]]) / np.maximum(cnt, 1), c)
        shift = float(((new - c) ** 2).sum())
        c, n_iter = new, it + 1
        if prev is not None and np.array_equal(b, prev):
            break
        if shift <= 0.0:
            break
        prev = b
    mid = (c[:-1] + c[1:]) / 2
    lab = np.searchsorted(mid, x, side="left")
    return c, n_iter, float(((x - c[lab]) ** 2).sum()), closest, empty


def lloyd_cases(rng):
    from sklearn.cluster import KMeans

    out = {}
    for n, k in LLOYD_NK:
        for attempt in range(200):
            x = rng.random(n).astype(np.float32)
            c0 = rng.choice(np.unique(x), k, replace=False).astype(np.float64)
            res, ok = {}, True
            for M in LLOYD_M:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    km = KMeans(n_clusters=k, init=c0.reshape(k, 1), n_init=1, algorithm="lloyd", tol=0, max_iter=M)
                    km.fit(x.astype(np.float64).reshape(-1, 1))
                sk = np.sort(km.cluster_centers_[:, 0])
                c, n_iter, inertia, closest, empty = lloyd_numpy(x, c0, M)
                ok = (closest > 1e-9 and not empty and n_iter == km.n_iter_ and np.abs(c - sk).max() <= 1e-12
                      and abs(inertia - km.inertia_) <= 1e-9 * km.inertia_)
                if not ok:
                    break
                res[M] = (sk, km.inertia_, km.n_iter_)
            if ok:
                break
        assert ok, (n, k)
        print(f"lloyd n={n} k={k}: attempt {attempt}, n_iter {[res[M][2] for M in LLOYD_M]}")
        out[f"lloyd_{n}_{k}_x"], out[f"lloyd_{n}_{k}_c0"] = x, c0
        for M in LLOYD_M:
            out[f"lloyd_{n}_{k}_{M}_centres"] = res[M][0]
            out[f"lloyd_{n}_{k}_{M}_inertia"] = np.float64(res[M][1])
            out[f"lloyd_{n}_{k}_{M}_n_iter"] = np.int64(res[M][2])
    return out


def optimum_1d(x, k):
    """global optimum of 1-D k-means by dynamic programming over the distinct sorted values (weights = multiplicities), with the
    divide-and-conquer speed-up (the optimal split point is monotone); the cost of the optimal partition is then summed directly"""
    v, w = np.unique(x.astype(np.float64), return_counts=True)
    m = len(v)
    W = np.concatenate([[0.0], np.cumsum(w)])
    S = np.concatenate([[0.0], np.cumsum(w * v)])
    S2 = np.concatenate([[0.0], np.cumsum(w * v * v)])

    def cost(j, i):   # values j .. i-1 in one cluster (j may be an array)
        cnt, s = W[i] - W[j], S[i] - S[j]
        return np.maximum((S2[i] - S2[j]) - s * s / np.maximum(cnt, 1), 0.0)

    prev = cost(0, np.arange(m + 1))
    prev[0] = 0.0
    args = []
    for layer in range(1, k):
        cur = np.full(m + 1, np.inf)
        arg = np.zeros(m + 1, dtype=np.int64)
        stack = [(layer + 1, m, layer, m - 1)]   # i in [lo, hi], split j in [jlo, jhi]: clusters 0..layer-1 cover [0, j)
        while stack:
            lo, hi, jlo, jhi = stack.pop()
            if lo > hi:
                continue
            i = (lo + hi) // 2
            js = np.arange(jlo, min(jhi, i - 1) + 1)
            tot = prev[js] + cost(js, i)
            b = int(np.argmin(tot))
            cur[i], arg[i] = tot[b], js[b]
            stack.append((lo, i - 1, jlo, js[b]))
            stack.append((i + 1, hi, js[b], jhi))
        args.append(arg)
        prev = cur
    cuts, i = [m], m
    for arg in reversed(args):
        i = int(arg[i])
        cuts.append(i)
    cuts.append(0)
    cuts = cuts[::-1]
    total = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        seg_v, seg_w = v[a:b], w[a:b]
        mean = float((seg_v * seg_w).sum() / seg_w.sum())
        total += float((seg_w * (seg_v - mean) ** 2).sum())
    return total


def full_cases(rng):
    from sklearn.cluster import KMeans

    n = FULL_N
    comp = rng.integers(0, 4, n)
    mix = np.where(comp == 0, rng.normal(0.5, 0.02, n), np.where(comp == 1, rng.normal(0.25, 0.08, n),
                   np.where(comp == 2, rng.beta(2, 5, n), 0.5)))
    data = {"cont": rng.random(n), "grid": np.round(rng.beta(2, 3, n) * 360) / 360,
            "mix": np.round(np.clip(mix, 0, 1) * 1440) / 1440}
    out = {}
    for name, x in data.items():
        x = x.astype(np.float32)
        out[f"full_{name}_x"] = x
        for k in FULL_K:
            js = []
            for s in range(FULL_SEEDS):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    js.append(KMeans(n_clusters=k, n_init=10, random_state=s).fit(x.astype(np.float64).reshape(-1, 1)).inertia_)
            opt = optimum_1d(x, k)
            assert opt <= min(js) * (1 + 1e-9), (name, k, opt, min(js))
            print(f"full {name} k={k}: sklearn {min(js):.6g} .. {max(js):.6g} (spread {(max(js) - min(js)) / min(js):.3%}), optimum {opt:.6g}")
            out[f"full_{name}_{k}_min"], out[f"full_{name}_{k}_max"] = np.float64(min(js)), np.float64(max(js))
            out[f"full_{name}_{k}_opt"] = np.float64(opt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from oracle.build_ref import REFERENCE_ROOT   # $LAYOUTDM_REFERENCE

    sys.dont_write_bytecode = True   # the reference tree stays pristine
    sys.path.insert(0, os.path.join(REFERENCE_ROOT, "src", "trainer"))
    from trainer.helpers.clustering import Percentile

    rng = np.random.default_rng(20261018)
    out = {}
    out.update(percentile_cases(Percentile, rng))
    out.update(lloyd_cases(rng))
    out.update(full_cases(rng))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
