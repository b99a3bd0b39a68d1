"""Writes tests/golden/eval_iou/reference.npz: the reference's own Max-IoU, DocSim and average-IoU results
(trainer/helpers/metric.py:206-507) on seeded synthetic layouts, for tests/test_eval_iou.py and tests/test_eval_iou_gpu.py.

    python tools/make_eval_iou_golden.py            # needs the reference tree (oracle.ref_harness.install_stubs())

Inputs (`inputs()`, reproducible from SEED) are float64 master values; the float32 runs cast them, the mixed run hands
set 1 as float32 and set 2 as float64 (a dataset layout against a kmeans-decoded one).  They cover random layouts over a
small skewed label vocabulary (shared groups of tens of layouts), segments of 1, 2, 3 and 25 equal labels, identical boxes
(tied matrices), touching and disjoint boxes, DocSim at |N - M| = 0, 2, 3 and across categories, layouts of 0 and 1
elements, boxes on kmeans-like centres where x * 32 falls on .5, and two sets without a shared label multiset.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "eval_iou", "reference.npz")
SEED = 20261016
SETS = ("mx_a", "mx_b", "ds_gt", "ds_gen", "avg", "nk_a", "nk_b")
PRECISIONS = ("f32", "f64", "mix")


def _boxes(rng, n, grid):
    if grid:  # kmeans-like centres: multiples of 1/64, so x * 32 lands on .5 for odd multiples
        xy = rng.integers(4, 60, (n, 2)) / 64.0
        wh = rng.integers(2, 30, (n, 2)) / 64.0
    else:
        xy = rng.uniform(0.1, 0.9, (n, 2))
        wh = rng.uniform(0.02, 0.5, (n, 2))
    return np.concatenate([xy, wh], 1)


def _layout(rng, labels, grid=None):
    labels = np.asarray(labels, np.int64)
    return _boxes(rng, len(labels), bool(rng.integers(2)) if grid is None else grid), labels


def inputs():
    """{set name: list of (bbox float64 (n,4), label int64 (n,))}"""
    rng = np.random.default_rng(SEED)
    p = np.array([0.6, 0.3, 0.1])

    def rand_set(k, n_max=4):
        return [_layout(rng, rng.choice(3, rng.integers(1, n_max + 1), p=p)) for _ in range(k)]

    mx_a, mx_b = rand_set(150), rand_set(150)
    # segments of 25 (the largest solver problem) and of 1 / 2 / 3 within one layout
    for s in (mx_a, mx_b):
        s += [_layout(rng, [0] * 25) for _ in range(3)]
        s += [_layout(rng, [0, 1, 1, 2, 2, 2]) for _ in range(4)]
    # identical boxes (tied matrices), touching and disjoint boxes
    same = np.tile([[0.5, 0.5, 0.25, 0.25]], (4, 1))
    mx_a.append((same.copy(), np.zeros(4, np.int64)))
    mx_b.append((same.copy(), np.zeros(4, np.int64)))
    touch = np.array([[0.25, 0.5, 0.25, 0.5], [0.5, 0.5, 0.25, 0.5], [0.75, 0.5, 0.25, 0.5], [0.9, 0.9, 0.1, 0.1]])
    mx_a.append((touch.copy(), np.zeros(4, np.int64)))
    mx_b.append((touch[::-1].copy(), np.zeros(4, np.int64)))

    ds_gt, ds_gen = [], []
    for d in (0, 0, 0, 2, -2, 3, -3, 1, -1, 4):
        for _ in range(8):
            n = int(rng.integers(3, 12))
            ds_gt.append(_layout(rng, rng.integers(0, 4, n)))
            ds_gen.append(_layout(rng, rng.integers(0, 4, n + d)))
    ds_gt += [_layout(rng, []), _layout(rng, [1]), _layout(rng, [1]), _layout(rng, [0, 0]), _layout(rng, [2] * 25)]
    ds_gen += [_layout(rng, [1]), _layout(rng, []), _layout(rng, [2]), _layout(rng, [1, 1]), _layout(rng, [2] * 24)]
    ds_gt.append((same.copy(), np.zeros(4, np.int64)))
    ds_gen.append((same.copy(), np.zeros(4, np.int64)))

    avg = [_layout(rng, rng.integers(0, 5, rng.integers(2, 14))) for _ in range(60)]
    avg += [_layout(rng, []), _layout(rng, [3]), _layout(rng, [0] * 25, grid=True), _layout(rng, [1] * 32, grid=False)]
    avg += [(same.copy(), np.zeros(4, np.int64)), (touch.copy(), np.zeros(4, np.int64))]
    avg.append((np.array([[0.5, 0.5, 0.0, 0.0], [0.2, 0.2, 0.1, 0.1]]), np.zeros(2, np.int64)))   # zero-area box
    avg.append((np.array([[0.5, 0.5, 0.01, 0.01], [0.5, 0.5, 0.01, 0.01]]), np.zeros(2, np.int64)))  # paints nothing

    nk_a = [_layout(rng, [5] * int(rng.integers(1, 4))) for _ in range(5)]
    nk_b = [_layout(rng, [6] * int(rng.integers(1, 4))) for _ in range(5)]
    return dict(mx_a=mx_a, mx_b=mx_b, ds_gt=ds_gt, ds_gen=ds_gen, avg=avg, nk_a=nk_a, nk_b=nk_b)


def flatten(layouts):
    n = np.array([len(l) for _, l in layouts], np.int32)
    box = np.concatenate([b for b, _ in layouts]).astype(np.float64) if len(layouts) else np.zeros((0, 4))
    lab = np.concatenate([l for _, l in layouts]).astype(np.int64) if len(layouts) else np.zeros(0, np.int64)
    return box.reshape(-1, 4), lab, n


def unflatten(box, lab, n, dtype=np.float64):
    out, o = [], 0
    for k in n:
        out.append((np.ascontiguousarray(box[o:o + k], dtype), lab[o:o + k].copy()))
        o += k
    return out


def cast(layouts, prec, which):
    """the layouts as handed to the metric in precision `prec` ('f32', 'f64', 'mix'); which = 1 (set 1) or 2 (set 2)"""
    f64 = prec == "f64" or (prec == "mix" and which == 2)
    return [(b.astype(np.float64 if f64 else np.float32), l) for b, l in layouts]


def group_keys(layouts_1, layouts_2):
    """shared label multisets in order of first appearance in layouts_1, and each set's member indices"""
    def groups(ls):
        g = {}
        for i, (_, l) in enumerate(ls):
            g.setdefault(tuple(sorted(l.tolist())), []).append(i)
        return g

    g1, g2 = groups(layouts_1), groups(layouts_2)
    keys = [k for k in g1 if k in g2]
    return keys, g1, g2


def compute(inp):
    from oracle import ref_harness as rh

    rh.install_stubs()
    metric = importlib.import_module("trainer.helpers.metric")
    pair_mx = getattr(metric, "__compute_maximum_iou_for_layout")
    group_mx = getattr(metric, "__compute_maximum_iou")
    pair_ds = getattr(metric, "__compute_docsim_between_two_layouts")
    layout_avg = getattr(metric, "__compute_average_iou")
    out = {}
    for name in SETS:
        out[f"{name}_box"], out[f"{name}_label"], out[f"{name}_n"] = flatten(inp[name])
    for p in PRECISIONS:
        a, b = cast(inp["mx_a"], p, 1), cast(inp["mx_b"], p, 2)
        keys, g1, g2 = group_keys(a, b)
        pairs, means, sizes = [], [], []
        for k in keys:
            l1, l2 = [a[i] for i in g1[k]], [b[i] for i in g2[k]]
            # the reference's flat order: meshgrid(range(N), range(M)) flattened -> set-2 index outer, set-1 inner
            pairs += [pair_mx(l1[i], l2[j]) for j in range(len(l2)) for i in range(len(l1))]
            means.append(group_mx((l1, l2)).mean())
            sizes.append((len(l1), len(l2)))
        out[f"maxiou_pairs_{p}"] = np.asarray(pairs, np.float64)
        out[f"maxiou_group_mean_{p}"] = np.asarray(means, np.float64)
        out[f"maxiou_group_size_{p}"] = np.asarray(sizes, np.int64)
        out[f"maxiou_{p}"] = np.float64(metric.compute_maximum_iou(a, b))
        out[f"maxiou_nokey_{p}"] = np.float64(metric.compute_maximum_iou(cast(inp["nk_a"], p, 1), cast(inp["nk_b"], p, 2)))

        g, h = cast(inp["ds_gt"], p, 1), cast(inp["ds_gen"], p, 2)
        out[f"docsim_pairs_{p}"] = np.asarray([pair_ds((x, y)) for x, y in zip(g, h)], np.float64)
        out[f"docsim_{p}"] = np.float64(metric.compute_docsim(g, h))
        # IoU entries of every DocSim pair (rows of set 1 x columns of set 2, row-major, concatenated): bit-exact targets
        ent = []
        for (b1, _), (b2, _) in zip(g, h):
            ii, jj = np.meshgrid(range(len(b1)), range(len(b2)), indexing="ij")
            if ii.size:
                ent.append(np.asarray(metric.compute_iou(b1[ii.ravel()], b2[jj.ravel()]), np.float64))
        out[f"iou_entries_{p}"] = np.concatenate(ent)

        if p != "mix":
            v = cast(inp["avg"], p, 1)
            out[f"avgiou_blt_{p}"] = np.asarray([layout_avg(l, perceptual=True) for l in v], np.float64)
            out[f"avgiou_vtn_{p}"] = np.asarray([layout_avg(l, perceptual=False) for l in v], np.float64)
            r = metric.compute_average_iou(v)
            out[f"avgiou_{p}"] = np.array([r["average_iou-BLT"], r["average_iou-VTN"]], np.float64)
            # perceptual entries of every layout's ordered off-diagonal pairs (the reference's flat order): bit-exact targets
            ent = []
            for bb, _ in v:
                N = len(bb)
                if N < 2:
                    continue
                ii, jj = np.meshgrid(range(N), range(N))
                ii, jj = ii.ravel(), jj.ravel()
                keep = ii != jj
                ent.append(np.asarray(metric.compute_perceptual_iou(bb[ii[keep]], bb[jj[keep]]), np.float64).ravel())
            out[f"blt_entries_{p}"] = np.concatenate(ent)
    out["seed"] = np.int64(SEED)
    return out


def main():
    out = compute(inputs())
    # (a directory of its own: every *.npz directly under tests/golden/ is oracle/make_golden.py's, and a test holds it to that)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
