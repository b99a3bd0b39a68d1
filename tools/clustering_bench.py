"""Times the coordinate-bin fits (layout_dm_amd/clustering.py) and writes profiles/clustering_bench.json.

    python tools/clustering_bench.py [--out profiles/clustering_bench.json] [--sizes 100000 3000000] [--yardstick FILE]
    python tools/clustering_bench.py --yardstick-only --out profiles/clustering_bench_yardstick.json   (CPU; no GPU needed)

Boxes: layout_dm_amd.synthetic.synth_boxes at N = 1e5 (the reference tool's cap) and N = 3e6 (PubLayNet's order).
  tool      fit_coordinate_bins end to end from host boxes (upload, sort, 32 models), kmeans and percentile legs alternated,
            median of 3.
  phases    HIP events around the C-ABI calls, medians of 3: sort and derive (prefix sums, distinct values) are the two stages of
            ldm_cluster_sort; fit = ldm_kmeans1d_fit(max_iter = 300) of all 320 runs; fit_1 = the same with max_iter = 1;
            lloyd_1 = ldm_kmeans1d_lloyd, one iteration of the 320 runs from quantile starts (Lloyd iteration + inertia pass +
            finish).  seeding = fit_1 - lloyd_1, lloyd = fit - seeding.
  seeding bandwidth: every seeding step of a run reads its coordinate's n float32 once in the potential pass (the candidate walk
            reads one tile more): bytes = 4 n * sum of k over runs; next to it a plain device copy of the four coordinate arrays
            measured in the same run (read bytes / time; it writes as many).
  yardstick sklearn KMeans(n_init=10) on float32 input at N = 1e5 for k = 32 and 256 (one coordinate, so x 4 for a cluster count
            of the tool) and, where the reference tree is at hand ($LAYOUTDM_REFERENCE), its Percentile at k = 256; the host and
            the thread count are recorded.  The reference tree is read with --yardstick-only alone, never in the GPU run; the GPU
            run times sklearn on its own host if it imports there and embeds a yardstick file written elsewhere under its label.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_of(fn, reps=3):
    return statistics.median(fn() for _ in range(reps))


def yardstick(label, with_reference):
    """with_reference: also time the reference's own Percentile (only where the reference tree may be read: --yardstick-only)"""
    from layout_dm_amd.synthetic import synth_boxes

    threads = os.environ.get("OMP_NUM_THREADS")   # (os.cpu_count() names the whole machine, not what a job may use)
    out = {"host": label, "threads": int(threads) if threads else "unset (library default)", "N": 100000}
    x = synth_boxes(100000, seed=1)[:, 0:1]
    try:
        import sklearn
        from sklearn.cluster import KMeans

        out["sklearn"] = sklearn.__version__
        for k in (32, 256):
            def run():
                t0 = time.time()
                KMeans(n_clusters=k, n_init=10, random_state=0).fit(x)
                return time.time() - t0
            out[f"kmeans_k{k}_one_coordinate_s"] = median_of(run, 3 if k == 32 else 1)
    except ImportError:
        out["sklearn"] = None
    if not with_reference:
        return out
    try:
        from oracle.build_ref import REFERENCE_ROOT

        sys.dont_write_bytecode = True
        sys.path.insert(0, os.path.join(REFERENCE_ROOT, "src", "trainer"))
        from trainer.helpers.clustering import Percentile

        def run():
            t0 = time.time()
            Percentile(n_clusters=256).fit(x)
            return time.time() - t0
        out["reference_percentile_k256_one_coordinate_s"] = median_of(run)
    except Exception as e:   # no reference tree on this host
        out["reference_percentile_k256_one_coordinate_s"] = None
        out["reference_percentile_note"] = f"not measured here ({type(e).__name__})"
    return out


def gpu_part(sizes):
    import torch

    from layout_dm_amd import clustering as cl
    from layout_dm_amd.binding import _stream_ptr
    from layout_dm_amd.synthetic import synth_boxes

    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "sizes": {}}

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for N in sizes:
        boxes = synth_boxes(N, seed=1)
        cl.fit_coordinate_bins(boxes[:5000], "kmeans")   # warm-up: library load, allocator
        legs = {"kmeans": [], "percentile": []}
        for _ in range(3):
            for alg in legs:   # alternated
                torch.cuda.synchronize()
                t0 = time.time()
                cl.fit_coordinate_bins(boxes, alg)
                torch.cuda.synchronize()
                legs[alg].append(time.time() - t0)
        r = {"tool_s": {alg: statistics.median(v) for alg, v in legs.items()}, "tool_runs_s": legs}
        # phases
        x = torch.from_numpy(boxes).to(dev).t().contiguous()
        problems = [(a, k) for k in cl.N_CLUSTERS_LIST for a in range(4)]
        s = cl._Sorted(x, False, len(problems), 10, "bench")
        order, h_prob, d_prob = cl._problem_table(problems, dev)
        P = len(problems)
        n_unique = torch.empty(4, dtype=torch.int64, device=dev)
        err = torch.empty(1, dtype=torch.int32, device=dev)

        def sort_stage(stages):
            rc = s.lib.ldm_cluster_sort(x.data_ptr(), 4, N, 0, stages, s.sorted.data_ptr(), s.ps.data_ptr(), s.ps2.data_ptr(),
                                        s.unique.data_ptr(), s.ps_unique.data_ptr(), n_unique.data_ptr(), s.work.data_ptr(),
                                        s.work.numel(), err.data_ptr(), _stream_ptr(dev))
            assert rc == 0

        cen = torch.empty((P * 10, 256), dtype=torch.float64, device=dev)
        ine = torch.empty(P * 10, dtype=torch.float64, device=dev)
        nit, rst = (torch.empty(P * 10, dtype=torch.int32, device=dev) for _ in range(2))

        def fit(max_iter):
            rc = s.lib.ldm_kmeans1d_fit(s.sorted.data_ptr(), s.ps.data_ptr(), s.ps2.data_ptr(), 4, N, h_prob.ctypes.data,
                                        d_prob.data_ptr(), P, 10, 0, 0, max_iter, 1e-4, cen.data_ptr(), ine.data_ptr(), nit.data_ptr(),
                                        rst.data_ptr(), s.work.data_ptr(), s.work.numel(), _stream_ptr(dev))
            assert rc == 0

        # one Lloyd iteration of as many runs as the fit has, from quantile starts
        runs = sorted([(a, k) for a, k in problems for _ in range(10)], key=lambda t: -t[1])
        q_prob = np.array([[a, k, k] for a, k in runs], np.int32)
        qd_prob = torch.from_numpy(q_prob).to(dev)
        distinct = [np.unique(row) for row in s.sorted.cpu().numpy()]
        start = np.zeros((len(runs), 256))
        for i, (a, k) in enumerate(runs):
            start[i, :k] = distinct[a][np.linspace(0, len(distinct[a]) - 1, k).astype(int)]
        d_start = torch.from_numpy(start).to(dev)
        s.ensure(len(runs), 1)

        def lloyd_1():
            rc = s.lib.ldm_kmeans1d_lloyd(s.sorted.data_ptr(), s.ps.data_ptr(), s.ps2.data_ptr(), 4, N, q_prob.ctypes.data,
                                          qd_prob.data_ptr(), len(runs), d_start.data_ptr(), 1, 1e-4, cen.data_ptr(), ine.data_ptr(),
                                          nit.data_ptr(), None, s.work.data_ptr(), s.work.numel(), _stream_ptr(dev))
            assert rc == 0

        dst = torch.empty_like(x)
        ph = {"sort_ms": median_of(lambda: events(lambda: sort_stage(1))),
              "derive_ms": median_of(lambda: events(lambda: sort_stage(2))),
              "fit_ms": median_of(lambda: events(lambda: fit(300))),
              "fit_1_ms": median_of(lambda: events(lambda: fit(1))),
              "lloyd_1_ms": median_of(lambda: events(lloyd_1)),
              "copy_ms": median_of(lambda: events(lambda: dst.copy_(x)), 5)}
        ph["seeding_ms"] = ph["fit_1_ms"] - ph["lloyd_1_ms"]
        ph["lloyd_ms"] = ph["fit_ms"] - ph["seeding_ms"]
        ph["note"] = ("sort, derive, fit, fit_1, lloyd_1 and copy are HIP-event times of whole calls; seeding_ms = fit_1_ms - lloyd_1_ms and "
                      "lloyd_ms = fit_ms - seeding_ms are differences of those, not events around the phases")
        seed_bytes = 4.0 * N * sum(k for _, k in problems) * 10
        ph["seeding_read_GBps"] = seed_bytes / (ph["seeding_ms"] * 1e-3) / 1e9
        ph["copy_read_GBps"] = 4.0 * N * 4 / (ph["copy_ms"] * 1e-3) / 1e9
        r["phases"] = ph
        res["sizes"][str(N)] = r
        print(N, json.dumps(r["tool_s"]), json.dumps(ph), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clustering_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 3000000])
    ap.add_argument("--yardstick", help="a yardstick JSON written by --yardstick-only on another host, embedded as it is")
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--host-label", default="build machine (no GPU)")
    args = ap.parse_args()
    if args.yardstick_only:
        out = {"yardstick": yardstick(args.host_label, True)}
    else:
        out = gpu_part(args.sizes)
        out["yardstick_gpu_host"] = yardstick("GPU host", False)
        if args.yardstick:
            with open(args.yardstick) as f:
                out["yardstick_other_host"] = json.load(f)["yardstick"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
