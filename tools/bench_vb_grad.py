"""What the loss backward costs on the MI355X: ldm_vb_grad (kernels_vb.hip vb_grad_k) on rico25 (S = 125, C = 155) at B = 64 and 512.

    python tools/bench_vb_grad.py [--out profiles/vb_grad_bench.json]

Per batch size, every figure the median over --reps timed repeats after --warmup untimed ones, device events around the work:
  vb_grad_call_us      one Engine.vb_grad call, values + gradient: the timestep upload, the error-word reset, vb_grad_k and the
                       error-word read-back the call ends with — a CALL's device time, not the kernel's alone
  vb_grad_values_us    the values-only call (the forward of DiffusionLoss)
  copy_us              a device copy of the same bytes (B S C float32 read and written): the distance to the bandwidth floor
  eager_fwd_bwd_us     float32 torch-eager forward + backward of oracle/restatement.py's loss (predict_start_from_logits, q_posterior
                       twice, kl / nll / aux, mean) on the same device, ONE t for the batch (the restatement takes a Python int): the
                       stand-in for what PyTorch does today.  "unavailable: ..." where the restatement does not run on the device.
Logits: seeded normal x 2; x_0: random valid layouts; x_t: Engine.q_sample at T // 3; the same t for every layout.  No ratio is
asserted anywhere: the file is a record.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def layouts(spec, n, seed):
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


def timed(fn, warmup, reps):
    """median device-event time of fn() in microseconds"""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out), max(out)


def eager_loss(R, W, spec, logits, x0, xt, t, T, aux_weight):
    import torch

    recon = R.predict_start_from_logits(logits)
    model = R.q_posterior(W, spec, recon, xt, t)
    lx0 = R.index_to_log_onehot(x0, spec.n_class)
    true = R.q_posterior(W, spec, lx0, xt, t)
    kl = (true.exp() * (true - model)).sum(1).mean(1)
    nll = -(lx0.exp() * model).sum(1).mean(1)
    aux = (lx0[:, :-1].exp() * (lx0[:, :-1] - recon[:, :-1])).sum(1).mean(1)
    pt = 1.0 / T
    first = 1.0 if t == 0 else 0.0
    w = (1 - t / T) + 1.0
    return ((first * nll + (1 - first) * kl) / pt).mean() + (w * aux_weight * (first * nll + (1 - first) * aux) / pt).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vb_grad_bench.json"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    import numpy as np
    import torch

    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion
    from layout_dm_amd.training import loss_coefficients
    from oracle import restatement as R
    from oracle import spec as SP
    from oracle import synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_vb_grad needs the GPU: nothing here falls back")
    dev = torch.device("cuda", 0)
    spec = SP.RICO25
    T, S, C = spec.n_step, spec.seq_len, spec.n_class
    d = HipMaskAndReplaceDiffusion(n_category=spec.n_category, precision="exact", max_batch=512)
    d.load_state_dict(synth.synth_state_dict(spec, seed=1, perturb=True))
    e = d.engine
    res = {"device": torch.cuda.get_device_name(0), "dataset": "rico25", "S": S, "C": C, "warmup": args.warmup, "reps": args.reps,
           "timing": "device events around the work, median (min, max) in microseconds", "batches": {}}
    for B in (64, 512):
        g = torch.Generator().manual_seed(B)
        logits = (torch.randn((B, S, C), generator=g) * 2.0).to(dev)
        x0 = layouts(spec, B, seed=B).to(dev)
        t = T // 3
        xt = e.q_sample(x0, t, seed=5)
        tv = np.full(B, t, np.int32)
        coef = torch.from_numpy(loss_coefficients(tv, np.full(B, 1.0 / T), T, 0.1, True, 1.0, 1.0, B, S)).to(dev)
        r = {"bytes_read_and_written": 2 * B * S * C * 4}
        r["vb_grad_call_us"] = timed(lambda: e.vb_grad(logits, x0, xt, tv, coef), args.warmup, args.reps)
        r["vb_grad_values_us"] = timed(lambda: e.vb_grad(logits, x0, xt, tv, None, want_grad=False), args.warmup, args.reps)
        dst = torch.empty_like(logits)
        r["copy_us"] = timed(lambda: dst.copy_(logits), args.warmup, args.reps)
        try:
            with torch.device(dev):
                W = {k: torch.from_numpy(v).to(dev) for k, v in SP.schedule_buffers(spec).items()}
                x0l, xtl = x0.long(), xt.long()

                def step():
                    leaf = logits.clone().requires_grad_(True)
                    eager_loss(R, W, spec, leaf, x0l, xtl, t, T, 0.1).backward()
                    return leaf.grad

                ge = step()
                r["eager_fwd_bwd_us"] = timed(step, max(2, args.warmup // 5), max(5, args.reps // 5))
                gk = e.vb_grad(logits, x0, xt, tv, coef)[0]
                r["eager_vs_kernel_max_abs"] = float((ge - gk).abs().max())
        except Exception as ex:  # the restatement was written for the CPU: say why it did not run
            r["eager_fwd_bwd_us"] = f"unavailable: {type(ex).__name__}: {ex}"[:300]
        res["batches"][str(B)] = r
        print(B, json.dumps(r))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
