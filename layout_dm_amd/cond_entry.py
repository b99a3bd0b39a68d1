"""`python -m layout_dm_amd.cond_entry cond=... job_dir=... result_dir=... [key=value ...]`

The hydra-less entry point (layout_dm_amd/test_entry.py) with the conditional tasks: same CLI keys, same job_dir layout, same
result pickles.  With the environment variable LDM_COND_LAYOUTS naming a result pickle in the format the entry points (and the
reference's test.py) write — its `results` list, or its `inputs` where it has none, of (bbox (n,4), label (n,)) pairs —
`cond=c|cwh|partial|refinement|relation` runs on those layouts: the cond dicts are built on the GPU (layout_dm_amd/task.py), so
neither the reference, its datasets nor torch_geometric is needed, and the output of a previous run can be refined or completed:

    LDM_COND_LAYOUTS=res/unconditional_.../seed_0.pkl python -m layout_dm_amd.cond_entry cond=refinement job_dir=JOB result_dir=res

With LDM_SAVE_VIS=1 the built-in runners also write the picture the reference saves of the first batch (test.py:205-214,
layout_dm_amd/visualization.py) as <result_dir>/<cond>_<key>/test_generated.png; any other non-empty value is the path itself.

Everything else — `cond=unconditional` without LDM_SAVE_VIS, both variables unset, the reference package importable — is
`test_entry.main` unchanged (without LDM_COND_LAYOUTS a conditional task stops with its SystemExit).
"""
from __future__ import annotations

import os
import pickle
import random
import sys
import time
from typing import Any, Dict, List, Optional

from .test_entry import (SAMPLING_DEFAULTS, AttrDict, GeometryTokenizer, _filter_invalid, _find_ckpt_dirs, _plain, parse_cli)
from .test_entry import main as _test_entry_main
from .test_entry import run_builtin as _run_builtin

COND_LAYOUTS_ENV = "LDM_COND_LAYOUTS"
BUILTIN_COND_TYPES = ("c", "cwh", "partial", "refinement", "relation")


class LayoutGeometryTokenizer(GeometryTokenizer):
    """GeometryTokenizer with the encode half: `encode` (LayoutSequenceTokenizer.encode, layout_tokenizer.py:208-253) and
    `bbox_tokenizer.encode` (BboxTokenizer.encode, bbox_tokenizer.py:84-115) run on the GPU through layout_dm_amd/task.py, and
    linear bins carry their cluster centres (bbox_tokenizer.py:72-82) like the other quantisations, which the refinement prior
    and the relation plan read."""

    def __init__(self, data_cfg, dataset_cfg, clustering_dir: Optional[str] = None):
        super().__init__(data_cfg, dataset_cfg, clustering_dir)
        self.pad_until_max, self.sort_by = True, None
        self.bbox_tokenizer["encode"] = self._encode_bbox
        if self.bbox_tokenizer.bbox_quantization == "linear":
            import numpy as np

            N, d = self.N_bbox_per_var, 1 / self.N_bbox_per_var
            xy, wh = np.linspace(0.0, 1.0 - d, N).reshape(N, 1), np.linspace(d, 1.0, N).reshape(N, 1)
            self.bbox_tokenizer["clustering_models"] = {f"{k}-{N}": AttrDict(cluster_centers_=xy if k in "xy" else wh)
                                                        for k in "xywh"}

    def encode(self, inputs):
        """{"bbox", "label", "mask"} -> {"seq" int64, "mask" bool}."""
        from . import task

        return task.encode(self, inputs["bbox"], inputs["label"], inputs["mask"])

    def _encode_bbox(self, bbox):
        """(B,S,4) boxes -> (B,S,4) int64 ids of the stacked bbox vocabulary."""
        import torch

        from . import task

        bbox = torch.as_tensor(bbox)
        B, S = bbox.shape[:2]
        seq = task.encode(self, bbox, torch.zeros((B, S), dtype=torch.long), torch.ones((B, S), dtype=torch.bool))["seq"]
        return seq.view(B, self.max_seq_length, 5)[:, :S, 1:] - self.N_category


def load_cond_layouts(path: str):
    """The layouts of a result pickle: its `results` list — or, where it has none, its `inputs` — of (bbox (n,4), label (n,))."""
    with open(path, "rb") as f:
        data = pickle.load(f)
    if not isinstance(data, dict) or not any(k in data for k in ("results", "inputs")):
        raise SystemExit(f"{COND_LAYOUTS_ENV}={path}: not a result pickle (a dict with 'results' or 'inputs')")
    items = data["results"] if "results" in data else data["inputs"]
    out = []
    for it in items:
        if not isinstance(it, (tuple, list)) or len(it) != 2 or len(it[0]) != len(it[1]):
            raise SystemExit(f"{COND_LAYOUTS_ENV}={path}: every layout must be a (bbox (n,4), label (n,)) pair")
        out.append((it[0], it[1]))
    if not out:
        raise SystemExit(f"{COND_LAYOUTS_ENV}={path}: no layouts")
    return out


def run_builtin_conditional(test_cfg: AttrDict, layouts) -> Dict[str, Any]:
    """trainer/test.py:57-283 for cond = c / cwh / partial / refinement / relation without the reference: `layouts` — a list
    of (bbox (n,4), label (n,)) — stands in for the dataset, layout_dm_amd.task.get_cond for the reference's get_cond and
    relation transforms (AddRelationConstraints(edge_ratio=0.1), keyed by the seed number like test.py:152-158).  The pickle has
    the reference's layout: `results`, `train_cfg`, `test_cfg`, `inputs` for partial / refinement (test.py:216-227), and for
    relation `violation_score`, the per-layout mean test.py:230-255,273-274 prints, through metrics.compute_violation."""
    import numpy as np
    import torch

    from . import metrics, task
    from .layoutdm import LayoutDM

    if test_cfg.cond not in BUILTIN_COND_TYPES:
        raise SystemExit(f"cond={test_cfg.cond}: the built-in conditional runner covers {', '.join(BUILTIN_COND_TYPES)}")
    layouts = list(layouts or [])
    if not layouts:
        raise SystemExit("the built-in conditional runner needs at least one layout")
    if not os.path.isdir(test_cfg.job_dir):
        raise FileNotFoundError(test_cfg.job_dir)
    # ---- the set-up of test_entry.run_builtin (test.py:64-128)
    train_cfg, ckpt_dirs = _find_ckpt_dirs(test_cfg.job_dir)
    if test_cfg.debug:
        ckpt_dirs = ckpt_dirs[:1]
    if test_cfg.sampling not in SAMPLING_DEFAULTS:
        raise SystemExit(f"sampling={test_cfg.sampling}: one of {sorted(SAMPLING_DEFAULTS)}")
    sampling_cfg = AttrDict(SAMPLING_DEFAULTS[test_cfg.sampling])
    if "temperature" in test_cfg and "temperature" in sampling_cfg:
        sampling_cfg.temperature = test_cfg.temperature
    if sampling_cfg.name == "top_p":
        sampling_cfg.top_p = test_cfg.top_p
    if sampling_cfg.name == "top_k_top_p":
        raise NotImplementedError("sampling=top_k resolves to top_k_top_p in the reference (sampling.py:52-54), which its "
                                  "own sample() does not implement either (sampling.py:117-118)")
    model_cfg = dict(train_cfg.model)
    target = str(model_cfg.pop("_target_"))
    model_cfg.pop("_partial_", None)
    if target.rsplit(".", 1)[-1] != "LayoutDM":
        raise NotImplementedError(f"model {target}: only LayoutDM is accelerated")
    data_cfg = train_cfg.data
    data_cfg["pad_until_max"] = True
    clustering_dir = os.path.join(test_cfg.dataset_dir, "..", "clustering_weights") if test_cfg.dataset_dir else None
    tokenizer = LayoutGeometryTokenizer(data_cfg, train_cfg.dataset, clustering_dir)
    model = LayoutDM(backbone_cfg=train_cfg.backbone, tokenizer=tokenizer,
                     max_batch=max(1, min(int(test_cfg.max_batch_size), 2048)), **model_cfg)
    sampling_cfg = model.aggregate_sampling_settings(sampling_cfg, test_cfg)
    key = "_".join(f"{k}_{v}" for k, v in sampling_cfg.items())
    if test_cfg.is_validation:
        key += "_validation"
    if test_cfg.debug:
        key += "_debug"
    if test_cfg.debug_num_samples > 0:
        key += f"_only_{test_cfg.debug_num_samples}_samples"
        layouts = layouts[:int(test_cfg.debug_num_samples)]
    result_dir = os.path.join(test_cfg.result_dir, f"{test_cfg.cond}_{key}")
    os.makedirs(result_dir, exist_ok=True)
    print(f"Results saved to {result_dir}", file=sys.stderr)

    engine = model.model.module.engine
    summary = {"result_dir": result_dir, "pickles": [], "ms_per_sample": []}
    for seed_no, ckpt_dir in enumerate(ckpt_dirs):
        random.seed(seed_no)          # set_seed, helpers/util.py:10-13
        np.random.seed(seed_no)
        torch.manual_seed(seed_no)
        model.load_state_dict(torch.load(os.path.join(ckpt_dir, "best_model.pt"), map_location="cpu"))
        model.eval()
        n, bs = len(layouts), int(test_cfg.max_batch_size)
        batches = (n // bs) * [bs] + ([n % bs] if n % bs else [])
        t_total, n_total, results, inputs, violation = 0.0, 0, [], [], 0.0
        for batch_size in batches:
            dense = task.layouts_from_list(layouts[n_total:n_total + batch_size], tokenizer.max_seq_length)
            dense = {k: v.to(engine.device) for k, v in dense.items()}
            cond = task.get_cond(dense, tokenizer, test_cfg.cond, first_layout=n_total,
                                 seed=seed_no if test_cfg.cond == "relation" else None)
            t0 = time.time()
            out = model.sample(batch_size=batch_size, cond=cond, sampling_cfg=sampling_cfg, cond_type=test_cfg.cond)
            t_total += time.time() - t0
            if n_total == 0:     # test.py:205-214, behind LDM_SAVE_VIS (off by default)
                from . import visualization

                vis = visualization.save_first_batch(out, result_dir, tokenizer.N_category)
                if vis:
                    summary.setdefault("images", []).append(vis)
            n_total += batch_size
            if cond["type"] in ("partial", "refinement"):   # test.py:216-227
                ids = cond["seq_orig" if cond["type"] == "refinement" else "seq"]
                shown = engine.decode(ids, model._device_decode_centres()[1])
                inputs.extend(_filter_invalid({k: v.cpu() for k, v in shown.items()}))
            results.extend(_filter_invalid(out))
            if cond["type"] == "relation":                   # test.py:230-255
                graph = cond["batch_w_canvas"]
                canvas = torch.tensor([0.5, 0.5, 1.0, 1.0], dtype=out["bbox"].dtype).expand(batch_size, 1, 4)
                bbox_c = torch.cat([canvas, out["bbox"]], dim=1)
                mask_c = torch.cat([torch.ones((batch_size, 1), dtype=torch.bool), out["mask"]], dim=1)
                if graph.edge_index.numel() > 0:
                    v = metrics.compute_violation(bbox_c[mask_c], graph)
                    violation += v[~v.isnan()].sum().item()
        dummy_cfg = AttrDict(train_cfg)
        dummy_cfg["sampling"] = sampling_cfg
        data = {"results": results, "train_cfg": _plain(dummy_cfg), "test_cfg": _plain(test_cfg)}
        if inputs:
            data["inputs"] = inputs
        if test_cfg.cond == "relation":
            data["violation_score"] = violation / max(len(results), 1)
            summary.setdefault("violation_score", []).append(data["violation_score"])
        pkl = os.path.join(result_dir, f"seed_{seed_no}.pkl")
        with open(pkl, "wb") as f:
            pickle.dump(data, f)
        print(n_total)
        print(f"ms per sample: {1e3 * t_total / max(n_total, 1)}")
        summary["pickles"].append(pkl)
        summary["ms_per_sample"].append(1e3 * t_total / max(n_total, 1))
    return summary


def run_builtin_unconditional(test_cfg: AttrDict) -> Dict[str, Any]:
    """test_entry.run_builtin, and with LDM_SAVE_VIS set the picture of batch 0 of every seed (test.py:205-214; each seed
    overwrites the file, as the reference overwrites tmp/test_generated.png).  That runner keeps nothing but its pickle, so
    batch 0 is read back from it: the first max_batch_size entries of `results`, one per layout with the invalid elements
    already dropped in order — the elements, the order and so the pixels that drawing the batch under its mask gives."""
    from . import task, visualization

    summary = _run_builtin(test_cfg)
    path = visualization.vis_path(summary["result_dir"])
    if path is None:
        return summary
    for pkl in summary["pickles"]:
        with open(pkl, "rb") as f:
            first = pickle.load(f)["results"][:max(1, int(test_cfg.max_batch_size))]
        if not first:
            continue
        import numpy as np
        import torch

        f64 = any(np.asarray(b).dtype == np.float64 for b, _ in first)
        dense = task.layouts_from_list(first, max(1, max(len(l) for _, l in first)), torch.float64 if f64 else torch.float32)
        n_colors = max(1, max((int(np.max(l)) + 1 for _, l in first if len(l)), default=1))   # (default_colors is prefix-stable)
        summary.setdefault("images", []).append(visualization.save_first_batch(dense, summary["result_dir"], n_colors))
    return summary


def _reference_importable() -> bool:
    try:
        import hydra  # noqa: F401
        import trainer.test  # noqa: F401
    except Exception:
        return False
    return True


def main(argv: Optional[List[str]] = None):
    argv = sys.argv[1:] if argv is None else argv
    path = os.environ.get(COND_LAYOUTS_ENV)
    if path and not _reference_importable():
        cfg = parse_cli(argv)
        if cfg.cond != "unconditional":
            return run_builtin_conditional(cfg, load_cond_layouts(path))
    if os.environ.get("LDM_SAVE_VIS") and not _reference_importable():
        cfg = parse_cli(argv)
        if cfg.cond == "unconditional":
            return run_builtin_unconditional(cfg)
    return _test_entry_main(argv)


if __name__ == "__main__":
    main()
