"""`python -m layout_dm_amd.score_entry job_dir=JOB layouts=RESULT_OR_DATA.pkl [seed=0] [out=score.json] [key=value ...]`

How well a checkpoint explains layouts it did not generate: the reference's held-out loss (trainer/main.py:271-294 `evaluate`,
the number that picks best_model.pt and is written to result.json as `test_loss`) and the per-layout variational bound, on
the GPU.  `layouts` is a pickle in the format the entry points (and the reference's test.py) write — its `results` list, or
its `inputs` where it has none, of (bbox (n,4), label (n,)) pairs — read the way cond_entry reads LDM_COND_LAYOUTS.

Prints `test_loss: <value>` per checkpoint of the job (job_dir itself, or job_dir/0, job_dir/1, ...) and writes `out`:

    {"job_dir", "layouts", "n_layouts", "seed", "n_draws", "checkpoints": [{"ckpt_dir", "test_loss", "elbo": [per layout]}]}

test_loss = mean over batches of kl_loss + aux_loss (LayoutDM.evaluate_loss: it includes the auxiliary term, because the
reference's LayoutDM.forward runs the diffusion with is_train=True even under evaluate()).  elbo = nats per token, sum over
the T timesteps of the reference's kl_loss term at one drawn x_t each, without the prior term L_T (the reference's bound has
none); lower = better explained.  Both are stochastic estimates, reproducible under `seed`: the noised states come from a
Philox stream keyed by (seed, layout index, t, position), not from the reference's torch generator.  Evaluation only.

Keys: job_dir, layouts (mandatory); seed (0), out (score.json), batch_size (64, the reference's default), n_draws (1),
max_batch_size (512), precision (auto), dataset_dir (for kmeans / percentile bin centres, as in test_entry), elbo (true).
"""
from __future__ import annotations

import json
import os
import random
import sys
from typing import Any, Dict, List, Optional

from .test_entry import AttrDict, _coerce, _find_ckpt_dirs

SCORE_DEFAULTS: Dict[str, Any] = {"job_dir": None, "layouts": None, "seed": 0, "out": "score.json", "batch_size": 64, "n_draws": 1,
                                  "max_batch_size": 512, "precision": "auto", "dataset_dir": None, "elbo": True}


def parse_cli(argv: List[str]) -> AttrDict:
    """`key=value` arguments; unknown keys and missing mandatory ones are errors."""
    cfg = AttrDict(SCORE_DEFAULTS)
    for arg in argv:
        if "=" not in arg:
            raise SystemExit(f"expected key=value, got '{arg}'")
        k, v = arg.split("=", 1)
        if k not in SCORE_DEFAULTS:
            raise SystemExit(f"unknown key '{k}' (keys: {', '.join(SCORE_DEFAULTS)})")
        try:
            cfg[k] = _coerce(v, SCORE_DEFAULTS[k]) if SCORE_DEFAULTS[k] is not None else (None if v in ("null", "None") else v)
        except ValueError as e:
            raise SystemExit(f"{k}={v}: {e}")
    for k in ("job_dir", "layouts"):
        if not cfg[k]:
            raise SystemExit(f"missing mandatory value: {k}=...")
    if cfg.batch_size < 1 or cfg.n_draws < 1 or cfg.max_batch_size < 1:
        raise SystemExit("batch_size, n_draws and max_batch_size must be >= 1")
    return cfg


def load_layouts(path: str):
    """(bbox (n,4), label (n,)) pairs of a result / data pickle (cond_entry.load_cond_layouts)."""
    from .cond_entry import COND_LAYOUTS_ENV, load_cond_layouts

    try:
        return load_cond_layouts(path)
    except SystemExit as e:
        raise SystemExit(str(e).replace(COND_LAYOUTS_ENV + "=", "layouts="))


def build_model(cfg: AttrDict, train_cfg):
    """The job's LayoutDM on the GPU with a tokenizer that can encode raw layouts (cond_entry.LayoutGeometryTokenizer)."""
    from .cond_entry import LayoutGeometryTokenizer
    from .layoutdm import LayoutDM

    model_cfg = dict(train_cfg.model)
    target = str(model_cfg.pop("_target_"))
    model_cfg.pop("_partial_", None)
    if target.rsplit(".", 1)[-1] != "LayoutDM":
        raise NotImplementedError(f"model {target}: only LayoutDM is accelerated")
    data_cfg = train_cfg.data
    data_cfg["pad_until_max"] = True
    clustering_dir = os.path.join(cfg.dataset_dir, "..", "clustering_weights") if cfg.dataset_dir else None
    tokenizer = LayoutGeometryTokenizer(data_cfg, train_cfg.dataset, clustering_dir)
    model_cfg.setdefault("precision", cfg.precision)
    return LayoutDM(backbone_cfg=train_cfg.backbone, tokenizer=tokenizer, max_batch=max(1, min(int(cfg.max_batch_size), 2048)),
                    **model_cfg)


def run(cfg: AttrDict) -> Dict[str, Any]:
    import numpy as np
    import torch

    from . import task

    if not os.path.isdir(cfg.job_dir):
        raise FileNotFoundError(cfg.job_dir)
    layouts = load_layouts(cfg.layouts)
    train_cfg, ckpt_dirs = _find_ckpt_dirs(cfg.job_dir)
    model = build_model(cfg, train_cfg)
    dense = task.layouts_from_list(layouts, int(train_cfg.dataset["max_seq_length"]))
    seq = model.encode(dense)["seq"]
    out = {"job_dir": cfg.job_dir, "layouts": cfg.layouts, "n_layouts": len(layouts), "seed": int(cfg.seed),
           "n_draws": int(cfg.n_draws), "checkpoints": []}
    for ckpt_dir in ckpt_dirs:
        random.seed(cfg.seed)         # set_seed, helpers/util.py:10-13: the timesteps come from torch's generator
        np.random.seed(cfg.seed)
        torch.manual_seed(cfg.seed)
        model.load_state_dict(torch.load(os.path.join(ckpt_dir, "best_model.pt"), map_location="cpu"))
        model.eval()
        test_loss = float(model.evaluate_loss(seq, batch_size=int(cfg.batch_size), seed=int(cfg.seed)))
        rec = {"ckpt_dir": ckpt_dir, "test_loss": test_loss}
        if cfg.elbo:
            rec["elbo"] = [float(v) for v in model.score(seq, n_draws=int(cfg.n_draws), seed=int(cfg.seed)).tolist()]
        print(f"test_loss: {test_loss}")
        out["checkpoints"].append(rec)
    if cfg.out:
        d = os.path.dirname(cfg.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(cfg.out, "w") as f:
            json.dump(out, f, indent=1)
        print(f"Scores saved to {cfg.out}", file=sys.stderr)
    return out


def main(argv: Optional[List[str]] = None):
    return run(parse_cli(sys.argv[1:] if argv is None else argv))


if __name__ == "__main__":
    main()
