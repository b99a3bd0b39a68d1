"""Timing of the layout renderer (layout_dm_amd/visualization.py, kernels_render.hip) and of the reference's own loop.

    python tools/render_bench.py [--out profiles/render_gpu_bench.json]     # on the GPU
    python tools/render_bench.py --reference [--out ...]                    # CPU: the reference's convert_layout_to_image loop

GPU: 512 seeded layouts of 1 - 25 elements (32 linear bins, float32) as one render_grid mosaic on the (60, 40) and the
(120, 80) canvas, and a 100-step x 512-layout render_trajectory (decode + render per step) of a synthetic engine's
intermediates.  Per case: device time of the launches between two events (median over repeats, after a warm-up), and the
wall-clock time of the Python call ending in a synchronise.  With --reference the same 512 layouts go through the
reference's per-layout PIL loop on the CPU (what save_image does before make_grid), timed with a host clock; the thread
count is recorded.  The two run on different machines: the file reports both and draws no ratio.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_LAYOUTS, N_CATEGORY, SEED = 512, 25, 3


def layouts():
    rng = np.random.default_rng(SEED)
    ids = rng.integers(0, 32, (N_LAYOUTS, 25, 4))
    d = np.float32(1 / 32)
    bbox = np.concatenate([ids[..., :2].astype(np.float32) * d, (ids[..., 2:] + 1).astype(np.float32) * d], -1)
    n = rng.integers(1, 26, N_LAYOUTS)
    return bbox, rng.integers(0, N_CATEGORY, (N_LAYOUTS, 25)).astype(np.int64), np.arange(25)[None, :] < n[:, None]


def reference_cpu(repeats: int):
    import torch

    from oracle import ref_harness as rh

    rh.install_stubs()
    from trainer.helpers.visualization import convert_layout_to_image

    from layout_dm_amd.visualization import default_colors

    bbox, label, mask = (torch.from_numpy(a) for a in layouts())
    colors = default_colors(N_CATEGORY)
    out = {"what": "the reference's convert_layout_to_image loop of save_image over 512 layouts, CPU, one process",
           "layouts": N_LAYOUTS, "elements": int(mask.sum()), "torch_threads": torch.get_num_threads(), "cases": {}}
    for canvas in ((60, 40), (120, 80)):
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for i in range(N_LAYOUTS):
                np.asarray(convert_layout_to_image(bbox[i][mask[i]], label[i][mask[i]], colors, canvas))
            times.append(time.perf_counter() - t0)
        out["cases"][f"{canvas[0]}x{canvas[1]}"] = {"seconds_median": statistics.median(times), "seconds_all": times}
    return out


def gpu(repeats: int):
    import torch

    from layout_dm_amd import visualization as V
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion
    from oracle import spec as SP
    from oracle import synth

    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs a GPU (use --reference for the CPU side)")
    dev = torch.device("cuda", 0)
    bbox, label, mask = (torch.from_numpy(a).to(dev) for a in layouts())
    colors = V.default_colors(N_CATEGORY)
    out = {"device": torch.cuda.get_device_name(0), "layouts": N_LAYOUTS, "elements": int(mask.sum()), "repeats": repeats,
           "cases": {}}

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        dev_ms, wall_ms = [], []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            r = fn()
            b.record()
            torch.cuda.synchronize()
            wall_ms.append(1e3 * (time.perf_counter() - t0))
            dev_ms.append(a.elapsed_time(b))
        return r, {"device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms),
                   "end_to_end_ms_median": statistics.median(wall_ms), "end_to_end_ms_min": min(wall_ms)}

    for canvas in ((60, 40), (120, 80)):
        grid, t = timed(lambda: V.render_grid(bbox, label, mask, colors, canvas))
        t["mosaic"] = list(grid.shape)
        out["cases"][f"render_grid_512_{canvas[0]}x{canvas[1]}"] = t
    spec = SP.RICO25
    m = HipMaskAndReplaceDiffusion(n_category=spec.n_category, precision="fast", max_batch=512, device=0)
    m.load_state_dict(synth.synth_state_dict(spec, seed=1, perturb=True))
    tokens = torch.full((N_LAYOUTS, m.engine.S), m.engine.mask_id, dtype=torch.int32, device=dev)
    from layout_dm_amd.diffusion import timestep_schedule

    t_model, t_post = timestep_schedule(100, 100, 0.0)
    _, inter = m.engine.sample_loop(tokens, t_model, t_post, {"name": "random", "temperature": 1.0}, seed=1, intermediates=True)
    frames, t = timed(lambda: V.render_trajectory(m.engine, inter, colors))
    t["frames"] = list(frames.shape)
    t["note"] = "device time spans 100 decode + 100 render launches and the host work between them"
    out["cases"]["render_trajectory_100x512_60x40"] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = reference_cpu(a.repeats or 3) if a.reference else gpu(a.repeats or 20)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
