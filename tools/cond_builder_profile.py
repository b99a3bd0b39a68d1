"""A 512-layout `task.get_cond` per cond type, for a kernel trace and for wall-clock times:

    rocprofv3 --kernel-trace --stats -d OUT -o cond --output-format csv -- python tools/cond_builder_profile.py
    python tools/cond_builder_profile.py            # wall-clock only

Layouts are synthetic (1 - 25 elements, Rico25 geometry, linear bins), resident on the device; every draw is the builder's own.
Per cond type: 3 warm-up calls, then 20 timed calls (each ends with the call's one device-to-host read).  Prints one JSON line."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, E, N_CATEGORY, CALLS = 512, 25, 25, 20


def main():
    from _stub_tokenizer import StubTokenizer
    from oracle import spec as SP

    from layout_dm_amd import task

    tok = StubTokenizer(SP.RICO25)
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    n = torch.randint(1, E + 1, (B,), generator=g)
    mask = torch.arange(E)[None] < n[:, None]
    wh = 0.05 + 0.4 * torch.rand((B, E, 2), generator=g)
    xy = wh / 2 + (1 - wh) * torch.rand((B, E, 2), generator=g)
    lay = {"bbox": (torch.cat([xy, wh], dim=-1) * mask[..., None]).to(dev),
           "label": (torch.randint(0, N_CATEGORY, (B, E), generator=g) * mask).to(dev), "mask": mask.to(dev)}
    out = {"layouts": B, "calls": CALLS, "ms_per_get_cond": {}}
    for ct in ("c", "cwh", "partial", "refinement", "relation"):
        for i in range(3):
            task.get_cond(lay, tok, ct, seed=i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(CALLS):
            cond = task.get_cond(lay, tok, ct, seed=i)
        torch.cuda.synchronize()
        out["ms_per_get_cond"][ct] = round(1e3 * (time.perf_counter() - t0) / CALLS, 4)
        if ct == "relation":
            out["relation_edges"] = int(cond["batch_w_canvas"].edge_attr.numel())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
