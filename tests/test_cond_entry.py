"""The built-in conditional runner of the hydra-less entry point (layout_dm_amd/cond_entry.py run_builtin_conditional): with
LDM_COND_LAYOUTS naming a result pickle, `cond=c|cwh|partial|refinement|relation` runs from that pickle's layouts, the cond
dicts built on the GPU (layout_dm_amd/task.py).  CPU: argument handling, and the unchanged SystemExit without the variable.
GPU: the pickles it writes."""
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from layout_dm_amd import cond_entry as CE
from layout_dm_amd import test_entry as TE
from test_entry_point import TRAIN_CFG

UNSET_TEXT = ("cond=c needs the reference's datasets and get_cond (trainer/helpers/task.py, torch_geometric): install the layout-dm "
              "package (poetry install) — this entry point then drives its own main(); the built-in runner covers cond=unconditional")


def _job(tmp_path, weights=False):
    job = tmp_path / "job"
    job.mkdir()
    (job / "config.yaml").write_text(yaml.safe_dump(TRAIN_CFG))
    if weights:
        from layout_dm_amd import synthetic as SY

        sd = {k: torch.from_numpy(v) for k, v in SY.synth_state_dict(SY.RICO25, seed=1, perturb=True).items()}
        torch.save(sd, job / "best_model.pt")
    return job


def _layouts(n_layouts=10, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_layouts):
        n = 1 + (3 * i) % 12
        wh = 0.05 + 0.3 * rng.random((n, 2))
        xy = wh / 2 + (1 - wh) * rng.random((n, 2))
        out.append((np.concatenate([xy, wh], axis=1).astype(np.float32), rng.integers(0, 25, n)))
    return out


def _no_reference(monkeypatch):
    """main() drives the reference's own entry point whenever hydra + trainer are importable: make sure they are not"""
    import sys

    for name in ("hydra", "trainer", "trainer.test", "trainer.models.layoutdm"):
        monkeypatch.setitem(sys.modules, name, None)


def test_geometry_tokenizer_has_encode_and_linear_centres():
    tok = CE.LayoutGeometryTokenizer(TE.to_attr(TRAIN_CFG["data"]), TE.to_attr(TRAIN_CFG["dataset"]))
    assert isinstance(tok, TE.GeometryTokenizer) and callable(tok.encode) and callable(tok.bbox_tokenizer.encode)
    from layout_dm_amd import task
    from layout_dm_amd.layoutdm import refinement_prior_table

    assert task.tokenizer_geometry(tok) == (25, 32, 25, "linear", None)
    cs = tok.bbox_tokenizer.clustering_models
    assert np.array_equal(cs["x-32"].cluster_centers_.reshape(-1), np.linspace(0.0, 1.0 - 1 / 32, 32))
    assert np.array_equal(cs["h-32"].cluster_centers_.reshape(-1), np.linspace(1 / 32, 1.0, 32))
    assert refinement_prior_table(tok, "uniform", 0.1).shape == (155, 155)


def test_without_the_variable_the_system_exit_is_unchanged(tmp_path, monkeypatch):
    job = _job(tmp_path)
    _no_reference(monkeypatch)
    monkeypatch.delenv(CE.COND_LAYOUTS_ENV, raising=False)
    with pytest.raises(SystemExit) as e:
        CE.main([f"job_dir={job}", f"result_dir={tmp_path / 'res'}", "cond=c"])
    assert str(e.value) == UNSET_TEXT
    with pytest.raises(SystemExit) as e:
        TE.run_builtin(TE.parse_cli([f"job_dir={job}", f"result_dir={tmp_path / 'res'}", "cond=c"]))
    assert str(e.value) == UNSET_TEXT


def test_argument_handling(tmp_path, monkeypatch):
    job = _job(tmp_path)
    _no_reference(monkeypatch)
    args = [f"job_dir={job}", f"result_dir={tmp_path / 'res'}"]
    # the layouts pickle: `results` first, `inputs` where there are none; anything else is refused
    lay = _layouts(3)
    p = tmp_path / "lay.pkl"
    pickle.dump({"results": lay, "inputs": lay[:1]}, open(p, "wb"))
    assert len(CE.load_cond_layouts(str(p))) == 3
    pickle.dump({"inputs": lay[:2]}, open(p, "wb"))
    assert len(CE.load_cond_layouts(str(p))) == 2
    for bad in ([1, 2, 3], {"other": 1}, {"results": []}, {"results": [(np.zeros((2, 4)), np.zeros(3))]}, {"results": [np.zeros(4)]}):
        pickle.dump(bad, open(p, "wb"))
        with pytest.raises(SystemExit, match=CE.COND_LAYOUTS_ENV):
            CE.load_cond_layouts(str(p))
    # cond types the runner does not cover, no layouts, a missing job_dir
    for cond in ("unconditional", "gt", "random"):
        with pytest.raises(SystemExit, match="covers c, cwh, partial, refinement, relation"):
            CE.run_builtin_conditional(TE.parse_cli(args + [f"cond={cond}"]), lay)
    with pytest.raises(SystemExit, match="at least one layout"):
        CE.run_builtin_conditional(TE.parse_cli(args + ["cond=c"]), [])
    with pytest.raises(FileNotFoundError):
        CE.run_builtin_conditional(TE.parse_cli([f"job_dir={tmp_path / 'nope'}", args[1], "cond=c"]), lay)
    # with the variable set, main() goes to the conditional runner (and stops at the pickle it cannot read)
    monkeypatch.setenv(CE.COND_LAYOUTS_ENV, str(tmp_path / "missing.pkl"))
    with pytest.raises(FileNotFoundError, match="missing.pkl"):
        CE.main(args + ["cond=refinement"])
    # a layout with more elements than the tokenizer holds is refused before anything runs
    from layout_dm_amd import task

    with pytest.raises(ValueError, match="26 elements"):
        task.layouts_from_list([(np.zeros((26, 4), np.float32), np.zeros(26, np.int64))], 25)
    dense = task.layouts_from_list(lay, 25)
    assert dense["bbox"].shape == (3, 25, 4) and dense["mask"].sum(1).tolist() == [len(l) for _, l in lay]


@pytest.mark.gpu
def test_conditional_runner_end_to_end(tmp_path, monkeypatch):
    """every cond type from a layouts pickle; the pickle has the reference's layout (`inputs` for partial / refinement), refining the
    output of a previous run works, and cond types that fix the categories return them."""
    job = _job(tmp_path, weights=True)
    _no_reference(monkeypatch)
    lay = _layouts(10)
    src = tmp_path / "lay.pkl"
    pickle.dump({"results": lay}, open(src, "wb"))
    monkeypatch.setenv(CE.COND_LAYOUTS_ENV, str(src))
    base = [f"job_dir={job}", "max_batch_size=4", "num_timesteps=10", "sampling=random"]
    outs = {}
    for cond in CE.BUILTIN_COND_TYPES:
        out = CE.main(base + [f"result_dir={tmp_path / 'res'}", f"cond={cond}"])
        assert os.path.basename(out["result_dir"]).startswith(cond + "_")
        data = pickle.load(open(out["pickles"][0], "rb"))
        outs[cond] = out
        want = {"results", "train_cfg", "test_cfg"} | ({"inputs"} if cond in ("partial", "refinement") else set()) | \
            ({"violation_score"} if cond == "relation" else set())
        assert set(data) == want and len(data["results"]) == 10 and data["test_cfg"]["cond"] == cond
        for (bbox, label), (b0, l0) in zip(data["results"], lay):
            assert bbox.ndim == 2 and bbox.shape[1] == 4 and bbox.dtype == np.float32 and label.shape == (bbox.shape[0],)
            if cond != "partial":
                assert np.array_equal(label, l0)           # the categories (and the element count) are the condition
            if cond == "cwh":
                assert np.abs(bbox[:, 2:] - b0[:, 2:]).max() <= 1 / 32 + 1e-6     # sizes come back within a bin
        if cond == "refinement":
            assert len(data["inputs"]) == 10
            for (bbox, label), (b0, l0) in zip(data["inputs"], lay):
                assert np.array_equal(label, l0) and bbox.shape == b0.shape      # the noisy layouts the model was shown
        if cond == "partial":
            assert len(data["inputs"]) == 10 and all(1 <= len(l) <= max(1, int((len(l0) - 1) * 0.3)) for (_, l), (_, l0) in zip(data["inputs"], lay))
        if cond == "relation":
            assert 0.0 <= data["violation_score"] <= 1.0 and outs[cond]["violation_score"] == [data["violation_score"]]
    # refine the output of a previous run
    monkeypatch.setenv(CE.COND_LAYOUTS_ENV, outs["c"]["pickles"][0])
    again = CE.main(base + [f"result_dir={tmp_path / 'res2'}", "cond=refinement"])
    data = pickle.load(open(again["pickles"][0], "rb"))
    prev = pickle.load(open(outs["c"]["pickles"][0], "rb"))["results"]
    assert len(data["results"]) == 10 and all(np.array_equal(l, l0) for (_, l), (_, l0) in zip(data["results"], prev))
