"""What scoring costs next to sampling (kernels_vb.hip, HipMaskAndReplaceDiffusion.elbo).

    python tools/vb_bench.py [--out profiles/vb_scoring_bench.json]     # on the GPU

B = 512 Rico25-shaped layouts, T = 100, on the `split` and `fast` engines.  Two legs, alternated, medians of `--runs` (3):

  elbo     HipMaskAndReplaceDiffusion.elbo: per t one forward-noising launch, the denoiser pass of the engine (chunk by chunk),
           one launch of the bound's terms per chunk, the error word read back (one stream synchronisation per t)
  sampling the eager (use_graph = 0) sample_loop of the same engine and batch: the same 100 denoiser passes with the
           sampling tail.  In the fast mode the reference's backbone runs that loop as ONE launch whatever use_graph says, so
           there the leg measures the one-launch loop, and the per-pass denoiser of ldm_denoise_logits is what elbo runs.

Each leg is timed with a host clock around work that ends in a device synchronise (wall) and with device events around the
same work (device).  ratio = elbo / sampling of the medians.  Where it exceeds 1.15 the per-launch profile of the elbo leg
(ldm_set_profiling) is recorded so that the launch that accounts for it can be named.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, SEED = 512, 100, 3


def layouts(spec, n, seed):
    """(n, S) int64 valid sequences: 1 .. max_elem elements, [PAD] behind them"""
    import numpy as np
    import torch

    rng = np.random.default_rng(seed)
    x = np.full((n, spec.seq_len), spec.pad_id, np.int64)
    for b in range(n):
        k = int(rng.integers(1, spec.max_elem + 1))
        x[b, 0:5 * k:5] = rng.integers(0, spec.n_category, k)
        for a in range(1, 5):
            x[b, a:5 * k:5] = spec.n_category + (a - 1) * spec.n_bin + rng.integers(0, spec.n_bin, k)
    return torch.from_numpy(x)


def one_engine(precision: str, runs: int):
    import torch

    from layout_dm_amd import synthetic as SY
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion, timestep_schedule

    spec = SY.RICO25
    d = HipMaskAndReplaceDiffusion(n_category=spec.n_category, num_timesteps=T, precision=precision, max_batch=B, use_graph=False)
    d.load_state_dict(SY.synth_state_dict(spec, seed=1, perturb=True))
    eng = d.engine
    x0 = layouts(spec, B, SEED).to(eng.device)
    tm, tp = timestep_schedule(T, T)
    cfg = {"name": "random", "temperature": 1.0, "num_timesteps": T}

    def elbo_leg():
        return d.elbo(x0, seed=7)

    def sampling_leg():
        tokens = torch.full((B, eng.S), eng.mask_id, dtype=torch.int32, device=eng.device)
        return eng.sample_loop(tokens, tm, tp, cfg, seed=7, use_graph=False)[0]

    legs = {"elbo": elbo_leg, "sampling": sampling_leg}
    first = {k: fn() for k, fn in legs.items()}             # warm-up: code objects, workspaces
    wall = {k: [] for k in legs}
    dev = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():                          # alternated
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall[k].append(1e3 * (time.perf_counter() - t0))
            dev[k].append(a.elapsed_time(b))
    res = {"describe": eng.describe(), "elbo_mean_nats_per_token": float(first["elbo"].mean()),
           "elbo_repeats_bitwise": bool(torch.equal(first["elbo"], elbo_leg()))}
    for k in legs:
        res[f"{k}_wall_ms"], res[f"{k}_device_ms"] = wall[k], dev[k]
        res[f"{k}_wall_ms_median"], res[f"{k}_device_ms_median"] = statistics.median(wall[k]), statistics.median(dev[k])
    res["ratio_wall"] = res["elbo_wall_ms_median"] / res["sampling_wall_ms_median"]
    res["ratio_device"] = res["elbo_device_ms_median"] / res["sampling_device_ms_median"]
    res["elbo_layouts_per_s"] = B / (res["elbo_wall_ms_median"] / 1e3)
    # the scoring launches alone, device events, and the denoiser passes alone: what the two legs do not share
    def timed(fn, n=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    t = T // 3
    xt = eng.q_sample(x0, t, 7, 0)
    logits = eng.denoise_logits(xt, t)
    res["q_sample_ms"] = timed(lambda: eng.q_sample(x0, t, 7, 0))
    res["vb_terms_ms"] = timed(lambda: eng.vb_terms(logits, x0, xt, t))
    res["denoise_logits_ms"] = timed(lambda: eng.denoise_logits(xt, t), 10)
    res["vb_step_ms"] = timed(lambda: eng.vb_step(x0, t, xt=xt), 10)
    if res["ratio_wall"] > 1.15 or res["ratio_device"] > 1.15:
        eng.set_profiling(True)
        elbo_leg()
        torch.cuda.synchronize()
        res["elbo_profile"] = sorted(eng.profile(reset=True), key=lambda r: -r["ms"])[:12]
        sampling_leg()
        torch.cuda.synchronize()
        res["sampling_profile"] = sorted(eng.profile(reset=True), key=lambda r: -r["ms"])[:12]
        eng.set_profiling(False)
    d.close()
    return res


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--engines", default="split,fast")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vb_bench needs a GPU")
    out = {"workload": {"B": B, "T": T, "dataset_shape": "rico25", "runs": a.runs, "legs": "alternated, medians"},
           "device": torch.cuda.get_device_name(0)}
    for p in a.engines.split(","):
        out[p] = one_engine(p, a.runs)
        print(p, json.dumps({k: v for k, v in out[p].items() if "median" in k or k.startswith("ratio") or k.endswith("_ms")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
