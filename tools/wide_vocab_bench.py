"""Throughput of the reference-precision `split` engine at wide vocabularies, and the check that the existing paths did not move.

    python tools/wide_vocab_bench.py [--parent-lib PATH] [--out profiles/wide_vocab_bench.json]        # on the GPU

  wide       precision split on the reference backbone, B = 512 Rico25-shaped unconditional layouts, T = 100, sampler random, at
             32, 64 and 128 bins per coordinate (155, 283 and 539 classes): layouts/s (median of --runs timed calls behind one
             warm-up, host clock around a call that ends in a device synchronise), and from one more call under
             ldm_set_profiling the device time per launch of the step tail (posterior_sample) and of the vocabulary head.
             No target is set: nothing had been measured at these sizes.
  ab         --parent-lib: the library built from the PARENT commit.  `python bench.py --gpus 1 --steps 5 --warmup 1 --full
             --modes <mode> --no-extras ...` on the default mode (fast) and on --precision split, one process per run, the two
             builds alternated (parent, this) --rounds times in this one session through LDM_HIP_LIB.  Per mode: the gain of
             this build per pair, and the spread of each build's own values over the rounds.  What must hold: |mean gain| stays
             inside the larger of the two builds' own spreads, and tokens_sha256 is identical in every run.

A child that fails ends the tool at once (nothing more is started on the GPU behind a failed run)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, SEED = 512, 100, 7
HEAD_LAUNCHES = ("gemm_ffn2_head_ln", "gemm_head_ln", "gemm_head", "layernorm_head")


def wide_point(n_bin: int, runs: int, chunk: int = 0):
    import dataclasses

    import torch

    from layout_dm_amd import synthetic as SY
    from layout_dm_amd.binding import Engine
    from layout_dm_amd.diffusion import timestep_schedule

    spec = dataclasses.replace(SY.RICO25, name=f"rico25_{n_bin}", n_bin=n_bin)
    eng = Engine(n_category=spec.n_category, n_bin=n_bin, precision="split", max_batch=B, chunk=chunk)
    eng.load_state_dict(SY.synth_state_dict(spec, seed=1, perturb=True))
    tm, tp = timestep_schedule(T, T)
    cfg = {"name": "random", "temperature": 1.0}

    def call(use_graph=True):
        tokens = torch.full((B, eng.S), eng.mask_id, dtype=torch.int32, device=eng.device)
        out = eng.sample_loop(tokens, tm, tp, cfg, seed=SEED, use_graph=use_graph)[0]
        torch.cuda.synchronize()
        return out

    first = call()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t0))
    assert torch.equal(call(), first)
    res = {"n_bin": n_bin, "n_class": spec.n_class, "describe": eng.describe(), "chunk": eng.chunk, "lanes": eng.lanes,
           "ms_per_call": ms, "ms_per_call_median": statistics.median(ms),
           "layouts_per_s": round(B / (statistics.median(ms) * 1e-3), 1)}
    eng.set_profiling(True)          # (per-launch events: eager launches, one more call)
    call(use_graph=False)
    prof = {r["name"]: r for r in eng.profile(reset=True)}
    eng.set_profiling(False)
    total = sum(r["ms"] for r in prof.values())
    res["profiled_call_device_ms"] = round(total, 3)
    res["launches"] = {k: {"device_ms_per_launch": round(r["ms"] / max(r["launches"], 1), 4), "launches": r["launches"],
                           "share_of_call": round(r["ms"] / total, 4)}
                       for k, r in prof.items() if k == "posterior_sample" or k in HEAD_LAUNCHES}
    assert bool((first != eng.mask_id).all())
    eng.close()
    return res


def bench_run(lib, mode):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--full", "--modes", mode,
           "--no-extras", "--no-cpu-baseline", "--no-traffic", "--no-roofline"]
    if mode != "fast":
        cmd += ["--precision", mode]
    env = dict(os.environ)
    env.pop("LDM_HIP_LIB", None)
    if lib:
        env["LDM_HIP_LIB"] = lib
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=420, cwd=ROOT)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} (LDM_HIP_LIB={lib}) ended with {p.returncode}:\n{p.stderr[-3000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    r = json.loads(line)
    return {"value": r["value"], "ms_per_step": r["ms_per_step"], "tokens_sha256": r["tokens_sha256"]["sha256"],
            "src_digest": r["config"]["library"].get("src_digest")}


def spread_pct(vals):
    return round(100.0 * (max(vals) - min(vals)) / statistics.mean(vals), 3)


def ab(parent_lib, rounds):
    out = {"what": "bench.py --gpus 1 --steps 5 --warmup 1 --full --modes <mode> --no-extras --no-cpu-baseline --no-traffic --no-roofline, "
                   "one process per run, builds alternated in one session on one GPU through LDM_HIP_LIB: P = the parent commit's "
                   "library, N = this build", "rounds": rounds}
    for mode in ("fast", "split"):
        pairs = []
        for rnd in range(rounds):
            p = bench_run(parent_lib, mode)
            n = bench_run(None, mode)
            pairs.append({"round": rnd, "P": p, "N": n, "gain_value_pct": round(100.0 * (n["value"] / p["value"] - 1.0), 3)})
            print(mode, json.dumps(pairs[-1]), flush=True)
        gains = [x["gain_value_pct"] for x in pairs]
        sp = {k: spread_pct([x[k]["value"] for x in pairs]) for k in ("P", "N")}
        shas = {x[k]["tokens_sha256"] for x in pairs for k in ("P", "N")}
        digests = {k: sorted({x[k]["src_digest"] for x in pairs}) for k in ("P", "N")}
        out[mode] = {"pairs": pairs, "n": len(pairs), "mean_gain_value_pct": round(statistics.mean(gains), 3),
                     "min_gain_value_pct": min(gains), "max_gain_value_pct": max(gains),
                     "spread_of_each_builds_own_values_pct": sp, "src_digest": digests,
                     "inside_the_alternations_spread": abs(statistics.mean(gains)) <= max(sp.values()),
                     "tokens_sha256_identical": len(shas) == 1, "tokens_sha256": sorted(shas)}
        assert digests["P"] != digests["N"], "both legs loaded the same library"
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--bins", default="32,64,128")
    ap.add_argument("--chunk", type=int, default=0, help="layouts per pass (0 = the library's choice for the vocabulary)")
    ap.add_argument("--parent-lib", default=None, help="libldm_hip.so built from the parent commit (the A/B is skipped without it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_vocab_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_vocab_bench needs a GPU")
    out = {"workload": {"B": B, "T": T, "precision": "split", "dataset_shape": "rico25, unconditional, sampler random", "runs": a.runs},
           "device": torch.cuda.get_device_name(0), "wide": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for nb in [int(x) for x in a.bins.split(",") if x]:
        out["wide"][str(nb)] = r = wide_point(nb, a.runs, a.chunk)
        print(nb, json.dumps({k: r[k] for k in ("n_class", "layouts_per_s", "ms_per_call_median", "launches")}), flush=True)
        save()
    if a.parent_lib:
        out["existing_paths_ab"] = ab(os.path.abspath(a.parent_lib), a.rounds)
        save()
    else:
        out["existing_paths_ab"] = "not collected (no --parent-lib)"
        save()


if __name__ == "__main__":
    main()
