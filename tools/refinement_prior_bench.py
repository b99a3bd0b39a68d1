"""What building the cond=refinement prior on the device buys (kernels_refine.hip, binding.refinement_prior).

    python tools/refinement_prior_bench.py [--out profiles/refinement_prior_bench.json]     # on the GPU

(a) End to end: LayoutDM.sample(batch_size=512, cond=refinement, T=100) on Rico25-shaped sequences from CPU cond tensors, as
    test.py hands them over, on the fast and the hybrid engine (synthetic weights: the time does not depend on them).  Two legs:
      host    the prior built by layoutdm.refinement_weak_logits on the host inside the timed call and passed as
              cond["weak_logits"] — what LayoutDM._sample_tokens did before this kernel existed;
      device  the cond as given: _sample_tokens builds the prior with the kernel.
    The legs alternate, three timed runs each after one warm-up run each; wall clock around a call that ends in a
    synchronise (LayoutDM.sample returns CPU tensors).  Both legs' layouts are compared: they must be identical.
(b) The kernel alone, B = 512, C = 155, S = 125 (39.7 MB out): device events around each ldm_refinement_prior call (the call's
    4-byte clear of the error word included), next to hipMemsetAsync of the same bytes between the same events.
The host leg's prior time alone (the gather on this machine's CPU) is recorded with the thread count.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B, T, SEED = 512, 100, 3
BACKBONE_CFG = {"encoder_layer": {"d_model": 512, "nhead": 8, "dim_feedforward": 2048, "timestep_type": "adalayernorm",
                                  "diffusion_step": T}, "num_layers": 4}


def refinement_cond(spec, tok, dev):
    """a cond=refinement dict of B layouts with CPU tensors (task.get_cond on seeded layouts, moved to the host)"""
    import torch

    from layout_dm_amd import task

    g = torch.Generator().manual_seed(SEED)
    E = spec.max_elem
    n = torch.randint(1, E + 1, (B,), generator=g)
    mask = torch.arange(E)[None] < n[:, None]
    wh = 0.05 + 0.4 * torch.rand((B, E, 2), generator=g)
    xy = wh / 2 + (1 - wh) * torch.rand((B, E, 2), generator=g)
    lay = {"bbox": (torch.cat([xy, wh], dim=-1) * mask[..., None]).to(dev),
           "label": (torch.randint(0, spec.n_category, (B, E), generator=g) * mask).to(dev), "mask": mask.to(dev)}
    cond = task.get_cond(lay, tok, "refinement", seed=SEED)
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in cond.items()}


def end_to_end(precision: str, runs: int):
    import torch

    from _stub_tokenizer import StubTokenizer
    from layout_dm_amd import layoutdm
    from oracle import spec as SP
    from oracle import synth

    spec = SP.RICO25
    tok = StubTokenizer(spec)
    dev = torch.device("cuda", 0)
    m = layoutdm.LayoutDM(backbone_cfg=BACKBONE_CFG, tokenizer=tok, num_timesteps=T, q_type="constrained", max_batch=B,
                          precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, seed=1, perturb=True).items()})
    cond = refinement_cond(spec, tok, dev)
    cfg = {"name": "random", "temperature": 1.0, "num_timesteps": T, "refine_mode": "uniform", "refine_offset_ratio": 0.1,
           "refine_lambda": 3.0}
    host_cache = {}

    def host_leg():
        c = dict(cond, weak_logits=layoutdm.refinement_weak_logits(tok, cond["seq_orig"], cfg, host_cache))
        return m.sample(batch_size=B, cond=c, sampling_cfg=cfg, seed=7)

    def device_leg():
        return m.sample(batch_size=B, cond=cond, sampling_cfg=cfg, seed=7)

    legs = {"host": host_leg, "device": device_leg}
    outs = {k: fn() for k, fn in legs.items()}          # warm-up: code objects, graphs, the cached tables
    same = all(torch.equal(outs["host"][k], outs["device"][k]) for k in ("bbox", "label", "mask"))
    times = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():                      # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0))
    gather = []
    for _ in range(runs):
        t0 = time.perf_counter()
        layoutdm.refinement_weak_logits(tok, cond["seq_orig"], cfg, host_cache)
        gather.append(1e3 * (time.perf_counter() - t0))
    m.model.module.close()
    res = {"engine": m.model.module.selected_precision, "identical_layouts": bool(same),
           "host_prior_alone_ms": gather, "host_torch_threads": torch.get_num_threads()}
    for k in legs:
        res[f"{k}_leg_ms"] = times[k]
        res[f"{k}_leg_ms_median"] = statistics.median(times[k])
    res["device_over_host"] = res["device_leg_ms_median"] / res["host_leg_ms_median"]
    return res


def kernel_alone(repeats: int):
    import torch

    from layout_dm_amd import binding
    from oracle import spec as SP

    spec = SP.RICO25
    dev = torch.device("cuda", 0)
    Cn, S = spec.n_class, spec.seq_len
    g = torch.Generator().manual_seed(SEED)
    seq = torch.randint(0, Cn, (B, S), generator=g).to(dev)
    table = torch.randn((Cn, Cn), generator=g).to(dev)
    out = torch.empty((B, Cn, S), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = binding.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemsetAsync.restype = C.c_int
    nbytes = out.numel() * 4
    stream = int(torch.cuda.current_stream(dev).cuda_stream)

    def prior(s):
        rc = lib.ldm_refinement_prior(s.data_ptr(), int(s.dtype == torch.int64), s.shape[0], B, S, Cn, table.data_ptr(), 3.0,
                                      out.data_ptr(), err.data_ptr(), stream)
        assert rc == 0, rc

    def fill(_s):
        assert hip.hipMemsetAsync(out.data_ptr(), 0, nbytes, stream) == 0

    def timed(fn, arg):
        for _ in range(5):
            fn(arg)
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(arg)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return {"device_ms_median": statistics.median(ms), "device_ms_min": min(ms), "gb_per_s_at_median": nbytes / statistics.median(ms) / 1e6}

    res = {"B": B, "C": Cn, "S": S, "bytes_out": nbytes, "repeats": repeats}
    # alternated in blocks: fill, kernel (int64 ids), fill, kernel (int32 ids, the builder's dtype), broadcast form
    res["memset_first"] = timed(fill, None)
    res["kernel_int64"] = timed(prior, seq)
    res["memset_second"] = timed(fill, None)
    res["kernel_int32"] = timed(prior, seq.int())
    res["kernel_broadcast_1_to_512"] = timed(prior, seq[:1].contiguous())
    assert int(err.item()) == 0
    fill_ms = min(res["memset_first"]["device_ms_median"], res["memset_second"]["device_ms_median"])
    res["kernel_over_memset"] = res["kernel_int64"]["device_ms_median"] / fill_ms
    return res


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refinement_prior_bench needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "T": T,
           "end_to_end": {p: end_to_end(p, a.runs) for p in ("fast", "hybrid")}, "kernel": kernel_alone(a.repeats)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
