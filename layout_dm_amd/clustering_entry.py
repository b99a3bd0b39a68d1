"""bin/clustering_coordinates.py without the reference, its datasets or scikit-learn:

    python -m layout_dm_amd.clustering_entry LAYOUTS.pkl {kmeans,percentile} --dataset rico25 --max_seq_length 25 \\
        --result_dir DIR [--random_state 0] [--max_bbox_num N]

LAYOUTS.pkl is a result pickle — a list of (bbox (n,4), label (n,)) under `results` or `inputs`, the form LDM_COND_LAYOUTS
reads (cond_entry.load_cond_layouts) — standing in for the training split.  Writes
DIR/<dataset>_max<N>_<algorithm>_train_clusters.pkl, the file GeometryTokenizer looks for, with one model per coordinate and
cluster count 2 .. 256, and prints one line per cluster count with its time, as the tool does.  --max_bbox_num: the tool's
subsampling of the kmeans input (its default there is 1e5 "to avoid too much time consumption"); left out, every box is fitted.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np
import torch


def main(argv=None) -> str:
    ap = argparse.ArgumentParser(prog="python -m layout_dm_amd.clustering_entry", description=__doc__.split("\n\n")[0])
    ap.add_argument("layouts", help="result pickle with the training layouts")
    ap.add_argument("algorithm", choices=["kmeans", "percentile"])
    ap.add_argument("--dataset", required=True, help="dataset name in the file name (rico25, publaynet, ...)")
    ap.add_argument("--max_seq_length", type=int, required=True)
    ap.add_argument("--result_dir", default="tmp/clustering_weights")
    ap.add_argument("--random_state", type=int, default=0)
    ap.add_argument("--max_bbox_num", type=int, default=None)
    args = ap.parse_args(argv)

    from . import clustering
    from .cond_entry import load_cond_layouts

    layouts = load_cond_layouts(args.layouts)
    bboxes = torch.from_numpy(np.concatenate([np.asarray(b, dtype=np.float32).reshape(-1, 4) for b, _ in layouts], axis=0))
    if args.max_bbox_num is not None and args.algorithm == "kmeans" and bboxes.shape[0] > args.max_bbox_num:
        print(f"Subsampling bboxes for kmeans: ({bboxes.shape[0]} -> {args.max_bbox_num})", file=sys.stderr)

    def report(n_clusters: int, seconds: float):
        print(f"{args.dataset} ({args.algorithm} {n_clusters} clusters): {seconds}s", flush=True)

    models = clustering.fit_coordinate_bins(bboxes, args.algorithm, random_state=args.random_state,
                                            max_bbox_num=args.max_bbox_num, progress=report)
    path = clustering.save_clusters(models, args.result_dir, args.dataset, args.max_seq_length, args.algorithm)
    print(path, flush=True)
    return path


if __name__ == "__main__":
    main()
