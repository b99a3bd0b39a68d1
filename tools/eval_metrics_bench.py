"""Device time of Max-IoU, DocSim and average IoU (layout_dm_amd/metrics.py, kernels_eval_iou.hip) on a seeded synthetic
workload; prints ONE JSON line.

    python tools/eval_metrics_bench.py [--layouts 3000] [--iters 5]          # on the MI355X
    python tools/eval_metrics_bench.py --reference-cpu 300                    # the reference's CPU cost per pair (needs it)
    python tools/eval_metrics_bench.py --violation [--iters 20]               # the relation violation score instead

Workload: two sets of `--layouts` layouts whose label multisets come from a handful of keys (a 6-element key, a 12-element
one and a 25-element one with segments of 1 - 10 equal labels), so that Max-IoU groups hold hundreds of layouts and the pair
count runs into the millions; set 1 float32 (the dataset side), set 2 float64 (LayoutDM's kmeans decode).  DocSim pairs
set 1 with set 2 element by element; average IoU runs over set 2.

device_ms: HIP events around the C-ABI launch on inputs already in HBM (warmed up, median of --iters);
end_to_end_ms: the drop-in from the Python lists (packing, copies, the launch, and for Max-IoU scipy's per-group
assignment on the host).  --reference-cpu N times the reference's own per-pair / per-layout functions on N problems of the
same workload on the CPU (single process, as eval.py runs them: DISABLED = True).

--violation: compute_violation (kernels_violation.hip) on the 512-layout relation batch of
tests/golden/relation_violation/reference.npz (7 267 nodes, 11 643 edges) and on 8 copies of it (4 096 layouts): device_ms
of the flattened and the dense entry point, end_to_end_ms of metrics.compute_violation as test.py:251 calls it (boxes on
the GPU, the graph on the host; includes the host-side CSR build, whose share is reported as csr_ms), and — where the
reference is importable — the reference's own function called the same way and on CPU tensors.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = (
    [0, 0, 0, 1, 1, 2],
    [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 4, 4],
    [0] * 10 + [1] * 6 + [2] * 4 + [3] * 2 + [4, 5, 6],
)


def workload(n: int, seed: int = 0):
    rng = np.random.default_rng(seed)

    def one(dt):
        key = np.asarray(KEYS[rng.integers(len(KEYS))], np.int64)
        k = len(key)
        b = np.concatenate([rng.integers(4, 60, (k, 2)) / 64.0, rng.integers(2, 30, (k, 2)) / 64.0], 1)
        return b.astype(dt), rng.permutation(key)

    return [one(np.float32) for _ in range(n)], [one(np.float64) for _ in range(n)]


def _median_ms(fn, iters):
    import torch

    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def gpu(args):
    import torch

    from layout_dm_amd import metrics as M
    from layout_dm_amd.binding import _stream_ptr, load_library

    a, b = workload(args.layouts, args.seed)
    lib, dev = load_library(), torch.device("cuda", 0)
    st = _stream_ptr(dev)
    res = {"workload": {"layouts_per_set": args.layouts, "keys": [len(k) for k in KEYS], "seed": args.seed}}

    # ---- Max-IoU: stage exactly what max_iou_pair_scores stages, then time the launch alone
    g1, g2 = M._groups(a), M._groups(b)
    keys = [k for k in g1 if k in g2]
    rows1, rows2 = [i for k in keys for i in g1[k]], [i for k in keys for i in g2[k]]
    table, f1, f2, off = [], 0, 0, 0
    for k in keys:
        n1, n2 = len(g1[k]), len(g2[k])
        table.append((f1, n1, f2, n2, len(k), off))
        f1, f2, off = f1 + n1, f2 + n2, off + n1 * n2
    S = max(len(k) for k in keys)
    max_seg = max(max(np.unique(np.asarray(k), return_counts=True)[1]) for k in keys)
    b1, l1, _ = M._pack([a[i] for i in rows1], S, np.float32, order=True)
    b2, _, _ = M._pack([b[i] for i in rows2], S, np.float64, order=True)
    b1, l1, b2 = (torch.from_numpy(x).to(dev) for x in (b1, l1, b2))
    gt = torch.tensor(table, dtype=torch.int64, device=dev)
    out = torch.empty(off, dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def mx():
        rc = lib.ldm_eval_max_iou_pairs(b1.data_ptr(), 0, l1.data_ptr(), len(rows1), b2.data_ptr(), 1, len(rows2), S,
                                        gt.data_ptr(), len(table), off, int(max_seg), out.data_ptr(), err.data_ptr(), st)
        assert rc == 0

    for _ in range(args.warmup):
        mx()
    ms = _median_ms(mx, args.iters)
    t0 = time.perf_counter()
    r = M.compute_maximum_iou(a, b)
    e2e = (time.perf_counter() - t0) * 1e3
    res["max_iou"] = {"pairs": off, "groups": [(t[1], t[3]) for t in table], "device_ms": ms, "pairs_per_s": off / ms * 1e3,
                      "end_to_end_ms": e2e, "value": r}

    # ---- DocSim: (a[i], b[i])
    Sd = max(len(l) for _, l in a + b)
    p1 = [torch.from_numpy(x).to(dev) for x in M._pack(a, Sd, np.float32)]
    p2 = [torch.from_numpy(x).to(dev) for x in M._pack(b, Sd, np.float64)]
    dout = torch.empty(len(a), dtype=torch.float64, device=dev)

    def ds():
        rc = lib.ldm_eval_docsim(p1[0].data_ptr(), 0, p1[1].data_ptr(), p1[2].data_ptr(), p2[0].data_ptr(), 1, p2[1].data_ptr(),
                                 p2[2].data_ptr(), len(a), Sd, dout.data_ptr(), err.data_ptr(), st)
        assert rc == 0

    for _ in range(args.warmup):
        ds()
    ms = _median_ms(ds, args.iters)
    t0 = time.perf_counter()
    r = M.compute_docsim(a, b)
    e2e = (time.perf_counter() - t0) * 1e3
    res["docsim"] = {"pairs": len(a), "device_ms": ms, "pairs_per_s": len(a) / ms * 1e3, "end_to_end_ms": e2e, "value": float(r)}

    # ---- average IoU over set 2
    box = p2[0]
    mask = (torch.arange(Sd, device=dev)[None, :] < p2[2][:, None].long()).to(torch.uint8).contiguous()
    aout = torch.empty((len(b), 2), dtype=torch.float64, device=dev)

    def av():
        rc = lib.ldm_eval_average_iou(box.data_ptr(), 1, mask.data_ptr(), len(b), Sd, aout.data_ptr(), st)
        assert rc == 0

    for _ in range(args.warmup):
        av()
    ms = _median_ms(av, args.iters)
    t0 = time.perf_counter()
    r = M.compute_average_iou(b)
    e2e = (time.perf_counter() - t0) * 1e3
    res["average_iou"] = {"layouts": len(b), "device_ms": ms, "layouts_per_s": len(b) / ms * 1e3, "end_to_end_ms": e2e,
                          "value": r}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


def violation_workload(copies: int):
    fx = np.load(os.path.join(ROOT, "tests", "golden", "relation_violation", "reference.npz"))
    box, y, ei, ea, batch = (fx["big_box"], fx["big_y"].astype(np.int64), fx["big_edge_index"].astype(np.int64),
                             fx["big_edge_attr"].astype(np.int64), fx["big_batch"].astype(np.int64))
    n, B = len(y), int(batch.max()) + 1
    return (np.tile(box, (copies, 1)), np.tile(y, copies), np.concatenate([ei + c * n for c in range(copies)], 1),
            np.tile(ea, copies), np.concatenate([batch + c * B for c in range(copies)]))


def violation(args):
    import torch

    from layout_dm_amd import metrics as M
    from layout_dm_amd.binding import _stream_ptr, load_library
    from layout_dm_amd.relation import graph_to_csr
    from oracle import ref_harness as rh

    lib, dev = load_library(), torch.device("cuda", 0)
    st = _stream_ptr(dev)
    ref = None
    if rh.reference_importable():
        rh.install_stubs()
        from trainer.helpers import metric as ref
    res = {"device": torch.cuda.get_device_name(0), "reference_importable": ref is not None, "iters": args.iters}

    def wall_ms(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    for copies in (1, 8):
        box, y, ei, ea, batch = violation_workload(copies)
        data = rh.GraphBatch(*(torch.from_numpy(v) for v in (y, ei, ea, batch)))
        data.x = torch.from_numpy(box)
        bx = data.x.to(dev)
        n_graph, E, n_nodes, canvas, off, src, dst, attr, first, _ = M._violation_graph(data, dev)
        out = torch.empty(n_graph, dtype=torch.float32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        g = (canvas.data_ptr(), n_nodes, off.data_ptr(), src.data_ptr(), dst.data_ptr(), attr.data_ptr(), first.data_ptr(), n_graph,
             E, out.data_ptr(), None, err.data_ptr(), st)
        # the dense layout of the same rows: elements first in their rows, the canvas row left to the kernel
        n = np.bincount(batch)
        S = int(n.max()) - 1
        mask = np.arange(S)[None, :] < (n - 1)[:, None]
        dense = np.zeros((n_graph, S, 4), np.float32)
        assert int((y == 0).sum()) == n_graph      # one canvas node per layout, its first
        dense[mask] = box[y != 0]
        tb, tm = torch.from_numpy(dense).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
        rows = torch.empty(n_graph + 1, dtype=torch.int32, device=dev)

        def flat():
            assert lib.ldm_relation_violation(bx.data_ptr(), 0, len(bx), *g) == 0

        def dens():
            assert lib.ldm_relation_violation_dense(tb.data_ptr(), 0, tm.data_ptr(), n_graph, S, rows.data_ptr(), *g) == 0

        leg = {"layouts": n_graph, "nodes": n_nodes, "edges": E}
        for name, fn in (("flat", flat), ("dense", dens)):
            for _ in range(args.warmup):
                fn()
            leg[f"{name}_device_ms"] = _median_ms(fn, args.iters)
            leg[f"{name}_err"] = int(err.item())
            leg[f"{name}_nan"] = int(out.isnan().sum())
        for _ in range(args.warmup):
            M.compute_violation(bx, data)
        leg["end_to_end_ms"] = wall_ms(lambda: M.compute_violation(bx, data), args.iters)
        leg["csr_ms"] = wall_ms(lambda: graph_to_csr(data, n_graph, with_nodes=True), args.iters)
        leg["dense_end_to_end_ms"] = wall_ms(lambda: M.relation_violation(tb, tm, data), args.iters)
        mine = M.compute_violation(bx, data)
        if ref is not None:
            leg["reference_gpu_tensors_ms"] = wall_ms(lambda: ref.compute_violation(bx, data), 1)
            leg["reference_cpu_tensors_ms"] = wall_ms(lambda: ref.compute_violation(data.x, data), 1)
            want = ref.compute_violation(data.x, data)
            leg["equal_to_reference"] = bool(torch.equal(mine.isnan(), want.isnan())
                                             and torch.equal(mine[~mine.isnan()], want[~want.isnan()]))
        res[f"x{copies}"] = leg
    print(json.dumps(res))


def reference_cpu(args):
    """the reference's own functions on N problems of the same workload (on the CPU, one process)"""
    import importlib

    from oracle import ref_harness as rh

    rh.install_stubs()
    metric = importlib.import_module("trainer.helpers.metric")
    pair_mx = getattr(metric, "__compute_maximum_iou_for_layout")
    pair_ds = getattr(metric, "__compute_docsim_between_two_layouts")
    layout_avg = getattr(metric, "__compute_average_iou")
    a, b = workload(args.layouts, args.seed)
    g1, g2 = {}, {}
    for i, (_, l) in enumerate(a):
        g1.setdefault(tuple(sorted(l.tolist())), []).append(i)
    for i, (_, l) in enumerate(b):
        g2.setdefault(tuple(sorted(l.tolist())), []).append(i)
    n = args.reference_cpu
    rng = np.random.default_rng(1)
    res = {"workload": {"layouts_per_set": args.layouts, "keys": [len(k) for k in KEYS], "seed": args.seed}, "problems": n}
    per_key = {}
    for k in g1:
        if k not in g2:
            continue
        pairs = [(g1[k][rng.integers(len(g1[k]))], g2[k][rng.integers(len(g2[k]))]) for _ in range(n)]
        t0 = time.perf_counter()
        for i, j in pairs:
            pair_mx(a[i], b[j])
        per_key[len(k)] = (time.perf_counter() - t0) / n * 1e6
    npairs = {len(k): len(g1[k]) * len(g2[k]) for k in g1 if k in g2}
    res["max_iou_us_per_pair_by_key_len"] = per_key
    res["max_iou_pairs_by_key_len"] = npairs
    res["max_iou_projected_s"] = sum(per_key[m] * npairs[m] for m in per_key) / 1e6
    t0 = time.perf_counter()
    for i in range(n):
        pair_ds((a[i], b[i]))
    res["docsim_us_per_pair"] = (time.perf_counter() - t0) / n * 1e6
    t0 = time.perf_counter()
    for i in range(n):
        layout_avg(b[i], perceptual=True)
        layout_avg(b[i], perceptual=False)
    res["average_iou_us_per_layout"] = (time.perf_counter() - t0) / n * 1e6
    res["cpu"] = "single process"
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reference-cpu", type=int, default=0, help="time the reference's CPU functions on N problems instead")
    ap.add_argument("--violation", action="store_true", help="time the relation violation score instead")
    args = ap.parse_args()
    if args.violation:
        violation(args)
    elif args.reference_cpu:
        reference_cpu(args)
    else:
        gpu(args)


if __name__ == "__main__":
    main()
