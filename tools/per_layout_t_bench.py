"""What per-layout timesteps change for scoring: loss() and elbo() of this tree against the parent commit, alternated.

    python tools/per_layout_t_bench.py --parent PATH_TO_A_BUILT_CHECKOUT_OF_THE_PARENT [--out profiles/per_layout_t_bench.json]

Rico25-shaped layouts, T = 100, max_batch = 512, synthetic weights (the launch sequence does not depend on them), on the `split`
engine and on `hybrid` — the engine precision="auto" selects for the fitted checkpoint.  Cases:

  loss_b64    HipMaskAndReplaceDiffusion.loss of one batch of 64 at sample_time()'s t (uniform over [0, T) without a history:
              43 distinct values under the seed used here), x_t drawn — one evaluate_loss batch
  elbo_b4     elbo() of 4 layouts   (ranking num_run candidates)        parent: 100 passes of 4;    here: 1 pass of 400 rows
  elbo_b64    elbo() of 64 layouts                                      parent: 100 passes of 64;   here: 13 passes of <= 512
  elbo_b512   elbo() of 512 layouts                                     both: 100 single-t passes of 512 — nothing changed

One worker process per tree (this file run with --worker: it imports layout_dm_amd from the tree it is given and uses only
what both trees have), both alive for the whole session; the driver alternates them case by case, `--rounds` times, after one
warm-up of every case on both.  The side that goes first changes from round to round (this tree, parent | parent, this tree |
...), so that neither side always starts on a GPU the other has just kept busy; medians are also given per position.  A value
is the host-clock time of one call that ends synchronised (loss() returns host scalars; elbo() is followed by a device
synchronise), the mean over the case's inner repeats.  Each side also reports the engine calls one call of the case makes and
a digest of its result under the fixed seeds: the two trees must compute the same bits.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, MAX_BATCH = 100, 512
CASES = {"loss_b64": ("loss", 64, 3), "elbo_b4": ("elbo", 4, 3), "elbo_b64": ("elbo", 64, 2), "elbo_b512": ("elbo", 512, 1)}   # kind, B, inner repeats
ENGINES = ("split", "hybrid")


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


# ------------------------------------------------------------------------------------------------ one tree
def worker(root: str):
    """Commands on stdin, one JSON line each: {"engine", "case", "count": bool} -> {"ms", "digest", "calls"}; "quit" ends."""
    sys.path.insert(0, root)
    import torch

    from layout_dm_amd import synthetic as SY
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion

    spec = SY.RICO25
    sd = SY.synth_state_dict(spec, seed=1, perturb=True)
    models = {}
    for p in ENGINES:
        d = HipMaskAndReplaceDiffusion(n_category=spec.n_category, num_timesteps=T, precision=p, max_batch=MAX_BATCH, use_graph=False)
        d.load_state_dict(sd)
        models[p] = d
    x0 = {B: layouts(spec, B, 3 + B).to(models[ENGINES[0]].engine.device) for _, B, _ in CASES.values()}
    torch.manual_seed(9)
    t64, pt64 = models[ENGINES[0]].sample_time(64)

    def run(d, kind, B):
        if kind == "loss":
            out = d.loss(x0[B], t=t64, pt=pt64, seed=5)
            return b"".join(float(out[k]).hex().encode() for k in sorted(out))
        out = d.elbo(x0[B], seed=7)
        torch.cuda.synchronize()
        return out.cpu().numpy().tobytes()

    print(json.dumps({"ready": True, "root": root, "describe": {p: models[p].engine.describe() for p in ENGINES},
                      "distinct_t_of_loss_b64": len(set(t64.tolist()))}), flush=True)
    for line in sys.stdin:
        line = line.strip()
        if line == "quit":
            break
        cmd = json.loads(line)
        d = models[cmd["engine"]]
        kind, B, reps = CASES[cmd["case"]]
        calls = None
        if cmd.get("count"):
            eng, calls = d.engine, {}
            for name in ("vb_step", "vb_step_t", "q_sample"):
                if hasattr(eng, name):
                    def spy(*a, _inner=getattr(eng, name), _name=name, **k):
                        calls[_name] = calls.get(_name, 0) + 1
                        return _inner(*a, **k)
                    setattr(eng, name, spy)
            run(d, kind, B)
            for name in ("vb_step", "vb_step_t", "q_sample"):
                if name in eng.__dict__:
                    delattr(eng, name)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            raw = run(d, kind, B)
        ms = 1e3 * (time.perf_counter() - t0) / reps
        print(json.dumps({"ms": ms, "digest": hashlib.sha256(raw).hexdigest()[:16], "calls": calls}), flush=True)
    for d in models.values():
        d.close()


# ------------------------------------------------------------------------------------------------ the session
class Side:
    def __init__(self, root):
        self.root = root
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True, cwd=root)
        self.hello = self.read()

    def read(self):
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise SystemExit(f"the worker of {self.root} ended (exit {self.p.wait()})")
            if line.startswith("{"):
                return json.loads(line)

    def ask(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        return self.read()

    def quit(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.flush()
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--this", default=ROOT, help="the tree under test (default: this one).  Control: --this PARENT --parent PARENT times two "
                                                 "processes of the SAME code, which is how far two processes differ by themselves")
    ap.add_argument("--rounds", type=int, default=6, help="alternations (even: each side goes first equally often)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("per_layout_t_bench needs a GPU")
    if not a.parent or not os.path.exists(os.path.join(a.parent, "layout_dm_amd", "libldm_hip.so")):
        raise SystemExit("--parent: a checkout of the parent commit with layout_dm_amd/libldm_hip.so built")
    sides = {"this_tree": Side(os.path.abspath(a.this)), "parent": Side(os.path.abspath(a.parent))}     # (one after the other: two start-ups, not overlapped)
    out = {"workload": {"T": T, "max_batch": MAX_BATCH, "dataset_shape": "rico25", "rounds": a.rounds, "cases": {k: {"kind": v[0], "B": v[1], "inner_repeats": v[2]} for k, v in CASES.items()},
                        "method": "two worker processes alive for the session, alternated case by case, the side that goes first swapped every round; "
                                  "ms = host clock around one synchronised call"},
           "device": torch.cuda.get_device_name(0), "trees": {k: s.root for k, s in sides.items()},
           "distinct_t_of_loss_b64": sides["this_tree"].hello["distinct_t_of_loss_b64"],
           "per_layout_t": {k: {p: s.hello["describe"][p].get("per_layout_t", "absent") for p in ENGINES} for k, s in sides.items()}}
    try:
        for eng in ENGINES:
            res = out[eng] = {}
            for case in CASES:     # warm-up of both sides, with the engine calls counted
                res[case] = {k: {"engine_calls": s.ask(engine=eng, case=case, count=True)["calls"], "ms": [], "went_first": []} for k, s in sides.items()}
            for rnd in range(a.rounds):
                order = list(sides) if rnd % 2 == 0 else list(sides)[::-1]
                for case in CASES:
                    for pos, k in enumerate(order):     # alternated
                        r = sides[k].ask(engine=eng, case=case)
                        res[case][k]["ms"].append(round(r["ms"], 3))
                        res[case][k]["went_first"].append(pos == 0)
                        res[case][k]["digest"] = r["digest"]
            for case in CASES:
                c = res[case]
                for k in sides:
                    c[k]["ms_median"] = statistics.median(c[k]["ms"])
                    c[k]["ms_spread"] = max(c[k]["ms"]) - min(c[k]["ms"])
                    for first in (True, False):
                        v = [m for m, f in zip(c[k]["ms"], c[k]["went_first"]) if f == first]
                        if v:
                            c[k]["ms_median_going_" + ("first" if first else "second")] = statistics.median(v)
                c["same_bits"] = c["this_tree"]["digest"] == c["parent"]["digest"]
                c["parent_over_this_tree"] = round(c["parent"]["ms_median"] / c["this_tree"]["ms_median"], 3)
                print(eng, case, json.dumps({"this_tree_ms": c["this_tree"]["ms_median"], "parent_ms": c["parent"]["ms_median"], "ratio": c["parent_over_this_tree"],
                                             "same_bits": c["same_bits"], "calls": c["this_tree"]["engine_calls"], "parent_calls": c["parent"]["engine_calls"]}), flush=True)
            # the one timing condition: nothing changed at B = 512, so this tree is not slower there than the alternations themselves spread
            c = res["elbo_b512"]
            c["not_slower_than_the_spread"] = c["this_tree"]["ms_median"] - c["parent"]["ms_median"] <= max(c["this_tree"]["ms_spread"], c["parent"]["ms_spread"])
    finally:
        for s in sides.values():
            s.quit()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
