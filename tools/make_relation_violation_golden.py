"""Writes tests/golden/relation_violation/reference.npz: the reference's own relation violation results —
compute_violation (trainer/helpers/metric.py:62-95), detect_size_relation and detect_loc_relation (trainer/data/util.py:33-69)
— with their inputs, for tests/test_relation_violation.py and tests/test_relation_violation_gpu.py.

    python tools/make_relation_violation_golden.py     # needs the reference tree (oracle.ref_harness.install_stubs())

Three sets of (boxes, y, edge_index, edge_attr, batch), each scored in float32 and in float64:
  * big    512 layouts of 1 - 25 elements through the reference's own AddCanvasElement + AddRelationConstraints
           (oracle.ref_harness.synth_layout_batch), the boxes then perturbed by 0.1 * randn, clamped to [0, 1], canvas rows
           restored, so that relations break: NaN, zero and many distinct non-zero scores.  float32 values; the float64
           run widens them.
  * edge   hand-made boundaries, built per precision (`handmade`): a2 exactly T(0.9) * a1 and T(1.1) * a1 and one ulp
           either side; boxes that touch (b2 == t1, r2 == l1, ...) and miss by one ulp, corners where two rules hold; a
           canvas source with yc at and next to 1/3 and 2/3 (in float32 and double roundings); gt with only the size part
           known, only the loc part, both, neither, several bits in a part, none; a duplicated edge; a graph without
           edges and one whose edges know nothing (NaN); a node with y == 0 that is not node 0 of its graph.
  * empty  three graphs and an empty edge list (the reference returns all NaN).
Node 0 of every graph is the canvas box (0.5, 0.5, 1, 1), so every set can also be laid out densely.

Per set and precision the file holds the reference's per-layout scores, the per-edge `failure` and `valid` it hands to
to_dense_adj, and both detectors' codes for every edge.  Only data: no program text.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "relation_violation", "reference.npz")
SEED = 20261016
SETS = ("big", "edge", "empty")
PRECISIONS = ("f32", "f64")
DTYPE = {"f32": np.float32, "f64": np.float64}
BIG = dict(n_category=25, B=512, seed=1, relation=True, n_lo=1, n_hi=25)

CANVAS = (0.5, 0.5, 1.0, 1.0)
S_UNK, L_UNK = 1 << 0, 1 << 4   # RelSize.UNKNOWN, RelLoc.UNKNOWN
# edge_attr variants: size part only (SMALLER / EQUAL / LARGER), loc part only (LEFT .. CENTER), both, neither, several bits
# in a part, no bit at all
GTS = [L_UNK | 1 << 1, L_UNK | 1 << 2, L_UNK | 1 << 3,
       S_UNK | 1 << 5, S_UNK | 1 << 6, S_UNK | 1 << 7, S_UNK | 1 << 8, S_UNK | 1 << 9,
       1 << 2 | 1 << 6, 1 << 3 | 1 << 9, 1 << 1 | 1 << 8, S_UNK | L_UNK,
       1 << 1 | 1 << 2 | 1 << 5 | 1 << 6, 1 << 2 | 1 << 3 | 1 << 7 | 1 << 9, 0, S_UNK | L_UNK | 1 << 2 | 1 << 6]


def handmade(T):
    """(box (N,4) T, y (N,), edge_index (2,E), edge_attr (E,), batch (N,)) of the boundary graphs, arithmetic in T"""
    T = np.dtype(T).type
    graphs = []   # (boxes, y, [(src, dst, gt)]), local node ids; node 0 = canvas
    up, dn = (lambda v: np.nextafter(T(v), T(2))), (lambda v: np.nextafter(T(v), T(-1)))

    # size: a1 = w1 * h1 rounded in T; a2 = target * 1 is exact
    w1, h1 = T(0.5), T(0.4)
    a1 = T(w1 * h1)
    lo, hi = T(T(1 - 0.1) * a1), T(T(1 + 0.1) * a1)
    boxes, y, edges = [CANVAS, (0.5, 0.5, w1, h1)], [0, 1], []
    for target in (lo, dn(lo), up(lo), hi, dn(hi), up(hi), a1, dn(a1), up(a1)):
        boxes.append((0.5, 0.5, target, 1.0))
        y.append(2)
        k = len(boxes) - 1
        edges += [(1, k, gt) for gt in GTS]
        edges += [(k, 1, GTS[(k + d) % len(GTS)]) for d in range(3)]
    graphs.append((boxes, y, edges))

    # loc: b1 = [0.375, 0.625]^2 (exact in both precisions); b2 of the same size on a grid of touching / one-ulp positions
    pos = [T(0.25), up(0.25), dn(0.25), T(0.5), T(0.75), dn(0.75), up(0.75)]
    boxes, y, edges = [CANVAS, (0.5, 0.5, 0.25, 0.25)], [0, 3], []
    for xc in pos:
        for yc in pos:
            boxes.append((xc, yc, 0.25, 0.25))
            y.append(4)
            k = len(boxes) - 1
            edges += [(1, k, GTS[(3 * k + d) % len(GTS)]) for d in range(3)]
            edges.append((k, 1, GTS[(5 * k) % len(GTS)]))
    graphs.append((boxes, y, edges))

    # canvas source: thirds of b2's yc, at and around both roundings of 1/3 and 2/3
    ycs = []
    for third in (1.0 / 3, 2.0 / 3):
        for v in (T(third), T(np.float32(third))):
            ycs += [v, dn(v), up(v)]
    ycs += [T(0.0), T(0.2), T(0.5), T(0.9), T(1.0)]
    boxes, y, edges = [CANVAS], [0], []
    for yc in ycs:
        boxes.append((0.5, yc, 0.2, 0.2))
        y.append(7)
        k = len(boxes) - 1
        edges += [(0, k, gt) for gt in (S_UNK | 1 << 6, S_UNK | 1 << 9, S_UNK | 1 << 8, 1 << 1 | 1 << 6, GTS[k % len(GTS)])]
        edges.append((k, 0, GTS[(k + 7) % len(GTS)]))      # a canvas TARGET is an ordinary box
    graphs.append((boxes, y, edges))

    # no edge at all: 0 / 0
    graphs.append(([CANVAS, (0.3, 0.3, 0.2, 0.2), (0.7, 0.7, 0.2, 0.2)], [0, 1, 2], []))

    # y == 0 on a node that is not node 0: the thirds rule follows the label, not the position; a duplicated edge
    boxes = [CANVAS, (0.3, 0.2, 0.2, 0.2), (0.6, 0.5, 0.3, 0.3), (0.5, 0.9, 0.2, 0.1)]
    edges = [(2, 3, S_UNK | 1 << 8), (2, 3, S_UNK | 1 << 8), (2, 1, S_UNK | 1 << 6), (1, 2, S_UNK | 1 << 6),
             (0, 2, 1 << 1 | 1 << 9), (2, 0, 1 << 3 | 1 << 9), (2, 3, 1 << 2 | 1 << 7), (3, 2, S_UNK | 1 << 5)]
    graphs.append((boxes, [0, 3, 0, 5], edges))

    # edges that know nothing: valid = 0 although there are edges
    graphs.append(([CANVAS, (0.3, 0.3, 0.2, 0.2), (0.7, 0.7, 0.2, 0.2)], [0, 1, 2], [(1, 2, S_UNK | L_UNK), (0, 1, S_UNK | L_UNK)]))

    # every known relation broken: 2 failures per edge
    graphs.append(([CANVAS, (0.3, 0.3, 0.2, 0.2), (0.7, 0.7, 0.2, 0.2)], [0, 1, 2], [(1, 2, 0), (2, 1, 0), (0, 2, 0)]))

    box, yy, ei, ea, batch, first = [], [], [], [], [], 0
    for g, (b, y, edges) in enumerate(graphs):
        box += [[T(v) for v in r] for r in b]
        yy += y
        batch += [g] * len(b)
        ei += [(first + s, first + d) for s, d, _ in edges]
        ea += [gt for _, _, gt in edges]
        first += len(b)
    return (np.asarray(box, T), np.asarray(yy, np.int64), np.asarray(ei, np.int64).T.reshape(2, -1), np.asarray(ea, np.int64),
            np.asarray(batch, np.int64))


def big_batch():
    """the 512-layout relation batch with perturbed float32 boxes (needs the reference: its transforms build the graph)"""
    import torch

    from oracle import ref_harness as rh

    b = rh.synth_layout_batch(BIG["n_category"], BIG["B"], seed=BIG["seed"], relation=BIG["relation"], n_lo=BIG["n_lo"],
                              n_hi=BIG["n_hi"])
    g = torch.Generator().manual_seed(SEED)
    box = (b.x + 0.1 * torch.randn(b.x.shape, generator=g)).clamp(0.0, 1.0)
    box[b.y == 0] = torch.tensor(CANVAS)
    return (box.numpy().astype(np.float32), b.y.numpy().astype(np.int64), b.edge_index.numpy().astype(np.int64),
            b.edge_attr.numpy().astype(np.int64), b.batch.numpy().astype(np.int64))


def inputs():
    """{set: {"f32": (box, y, edge_index, edge_attr, batch), "f64": ...}}"""
    big = big_batch()
    empty = (np.asarray([CANVAS, (0.3, 0.3, 0.2, 0.2), CANVAS, CANVAS, (0.6, 0.6, 0.1, 0.1)]), np.asarray([0, 4, 0, 0, 2], np.int64),
             np.zeros((2, 0), np.int64), np.zeros(0, np.int64), np.asarray([0, 0, 1, 2, 2], np.int64))
    return {"big": {p: (big[0].astype(DTYPE[p]),) + big[1:] for p in PRECISIONS},
            "edge": {p: handmade(DTYPE[p]) for p in PRECISIONS},
            "empty": {p: (empty[0].astype(DTYPE[p]),) + empty[1:] for p in PRECISIONS}}


def load_inputs(fx):
    """the same structure from the committed file"""
    out = {}
    for s in SETS:
        graph = tuple(np.asarray(fx[f"{s}_{k}"], np.int64) for k in ("y", "edge_index", "edge_attr", "batch"))
        out[s] = {p: (fx[f"{s}_box_{p}"] if f"{s}_box_{p}" in fx else fx[f"{s}_box"].astype(DTYPE[p]),) + graph
                  for p in PRECISIONS}
    return out


def reference_outputs(box, y, edge_index, edge_attr, batch):
    """the reference's own functions on one set: score float32 (n_graph,), per-edge failure / valid / size / loc int32"""
    import torch

    from oracle import ref_harness as rh

    rh.install_stubs()
    from trainer.data.util import detect_loc_relation, detect_size_relation
    from trainer.helpers import metric

    bx, yt = torch.from_numpy(np.ascontiguousarray(box)), torch.from_numpy(y)
    ei, ea, bt = torch.from_numpy(edge_index), torch.from_numpy(edge_attr), torch.from_numpy(batch)
    data = rh.GraphBatch(yt, ei, ea, bt)
    data.x = bx
    seen, dense = [], metric.to_dense_adj

    def spy(edge_index, batch, attr):   # compute_violation's per-edge failures, then valid, on their way into the sum
        seen.append(attr.clone())
        return dense(edge_index, batch, attr)

    metric.to_dense_adj = spy
    try:
        score = metric.compute_violation(bx, data)
    finally:
        metric.to_dense_adj = dense
    failure, valid = seen
    size = [int(detect_size_relation(bx[i], bx[j])) for i, j in ei.t()]
    loc = [int(detect_loc_relation(bx[i], bx[j], yt[i].eq(0))) for i, j in ei.t()]
    assert score.dtype == torch.float32
    return {"score": score.numpy(), "failure": failure.numpy().astype(np.int32), "valid": valid.numpy().astype(np.int32),
            "size": np.asarray(size, np.int32), "loc": np.asarray(loc, np.int32)}


def compute(inp):
    out = {"seed": np.int64(SEED)}
    for s in SETS:
        box32, y, ei, ea, batch = inp[s]["f32"]
        out[f"{s}_y"], out[f"{s}_batch"] = y.astype(np.int16), batch.astype(np.int32)
        out[f"{s}_edge_index"], out[f"{s}_edge_attr"] = ei.astype(np.int32), ea.astype(np.int16)
        if np.array_equal(box32.astype(np.float64), inp[s]["f64"][0]):
            out[f"{s}_box"] = box32                     # one copy: the float64 run widens it
        else:
            for p in PRECISIONS:
                out[f"{s}_box_{p}"] = inp[s][p][0]
        for p in PRECISIONS:
            for k, v in reference_outputs(*inp[s][p]).items():
                out[f"{s}_{k}_{p}"] = v
    return out


def main():
    out = compute(inputs())
    # (a directory of its own: every *.npz directly under tests/golden/ is oracle/make_golden.py's, and a test holds it to that)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    for s in SETS:
        for p in PRECISIONS:
            v = out[f"{s}_score_{p}"]
            f = v[~np.isnan(v)]
            print(s, p, "graphs", len(v), "NaN", int(np.isnan(v).sum()), "zero", int((f == 0).sum()), "non-zero", int((f != 0).sum()),
                  "distinct", len(np.unique(f)), "edges", out[f"{s}_edge_attr"].size)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
