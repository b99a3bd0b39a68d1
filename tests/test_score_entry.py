"""`python -m layout_dm_amd.score_entry` — CPU side: the key=value arguments, the layouts pickle, and the path from the pickle to
test_loss / per-layout bounds with a stand-in model in place of the GPU one (the numbers themselves: tests/test_vb_gpu.py).
Also what HipMaskAndReplaceDiffusion does on the host around the kernels: time_weights / sample_time (base.py:179-198) against
the fixture of tools/make_vb_golden.py, and the checkpoint's Lt_history / Lt_count staying on the host."""
import json
import pickle

import numpy as np
import pytest
import torch
import yaml

import _vb_cases as VC
from layout_dm_amd import score_entry as SE
from test_cond_entry import _layouts
from test_entry_point import TRAIN_CFG


def test_cli_parsing():
    cfg = SE.parse_cli(["job_dir=J", "layouts=L.pkl"])
    assert (cfg.job_dir, cfg.layouts, cfg.seed, cfg.out, cfg.batch_size, cfg.n_draws, cfg.elbo) == ("J", "L.pkl", 0, "score.json", 64, 1, True)
    cfg = SE.parse_cli(["job_dir=J", "layouts=L.pkl", "seed=7", "out=x/y.json", "batch_size=8", "n_draws=3", "elbo=false", "precision=split"])
    assert (cfg.seed, cfg.out, cfg.batch_size, cfg.n_draws, cfg.elbo, cfg.precision) == (7, "x/y.json", 8, 3, False, "split")
    for bad, msg in ((["job_dir=J"], "missing mandatory value: layouts"), (["layouts=L"], "missing mandatory value: job_dir"),
                     (["job_dir=J", "layouts=L", "cond=c"], "unknown key 'cond'"), (["job_dir=J", "layouts=L", "seed"], "expected key=value"),
                     (["job_dir=J", "layouts=L", "seed=x"], "seed=x"), (["job_dir=J", "layouts=L", "batch_size=0"], ">= 1")):
        with pytest.raises(SystemExit, match=msg):
            SE.parse_cli(bad)


def test_layouts_pickle(tmp_path):
    lay = _layouts(3)
    p = tmp_path / "lay.pkl"
    pickle.dump({"results": lay, "inputs": lay[:1]}, open(p, "wb"))
    assert len(SE.load_layouts(str(p))) == 3
    pickle.dump({"inputs": lay[:2]}, open(p, "wb"))
    assert len(SE.load_layouts(str(p))) == 2
    pickle.dump({"other": 1}, open(p, "wb"))
    with pytest.raises(SystemExit, match=r"^layouts=.*not a result pickle"):
        SE.load_layouts(str(p))
    with pytest.raises(FileNotFoundError):
        SE.load_layouts(str(tmp_path / "missing.pkl"))


class _FakeModel:
    """stands in for LayoutDM: records what the entry point hands it"""

    def __init__(self):
        self.calls = []

    def encode(self, dense):
        self.calls.append(("encode", tuple(dense["bbox"].shape), dense["mask"].sum(1).tolist()))
        return {"seq": torch.arange(dense["bbox"].shape[0] * 125).reshape(-1, 125)}

    def load_state_dict(self, sd):
        self.calls.append(("load", sorted(sd)))

    def eval(self):
        return self

    def evaluate_loss(self, seq, batch_size, seed):
        self.calls.append(("evaluate_loss", tuple(seq.shape), batch_size, seed))
        return 12.5

    def score(self, seq, n_draws, seed):
        self.calls.append(("score", n_draws, seed))
        return torch.arange(seq.shape[0], dtype=torch.float64) + 0.25


def test_pickle_to_scores_with_a_stand_in_model(tmp_path, monkeypatch, capsys):
    job = tmp_path / "job"
    for sub in ("0", "1"):                                   # the multi-seed job layout: one record per checkpoint
        (job / sub).mkdir(parents=True)
        (job / sub / "config.yaml").write_text(yaml.safe_dump(TRAIN_CFG))
        torch.save({"w": torch.zeros(1)}, job / sub / "best_model.pt")
    lay = _layouts(5)
    p = tmp_path / "lay.pkl"
    pickle.dump({"results": lay}, open(p, "wb"))
    fake = _FakeModel()
    monkeypatch.setattr(SE, "build_model", lambda cfg, train_cfg: fake)
    out_path = tmp_path / "sub" / "score.json"
    out = SE.main([f"job_dir={job}", f"layouts={p}", "seed=3", f"out={out_path}", "batch_size=2", "n_draws=2"])
    assert fake.calls[0] == ("encode", (5, 25, 4), [len(l) for _, l in lay])
    assert fake.calls[1:4] == [("load", ["w"]), ("evaluate_loss", (5, 125), 2, 3), ("score", 2, 3)] and len(fake.calls) == 7
    assert capsys.readouterr().out.splitlines() == ["test_loss: 12.5", "test_loss: 12.5"]
    data = json.load(open(out_path))
    assert data == out and data["n_layouts"] == 5 and data["seed"] == 3 and data["n_draws"] == 2
    assert [c["ckpt_dir"] for c in data["checkpoints"]] == [str(job / "0"), str(job / "1")]
    assert data["checkpoints"][0]["elbo"] == [0.25, 1.25, 2.25, 3.25, 4.25] and data["checkpoints"][1]["test_loss"] == 12.5
    # elbo=false leaves the bounds out; a missing job_dir is refused before anything is built
    out = SE.main([f"job_dir={job}", f"layouts={p}", f"out={out_path}", "elbo=false"])
    assert "elbo" not in out["checkpoints"][0]
    with pytest.raises(FileNotFoundError):
        SE.main([f"job_dir={tmp_path / 'nope'}", f"layouts={p}"])


class _NoEngine:
    """HipMaskAndReplaceDiffusion's host half without a GPU: the methods below touch no engine"""
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion as _D

    time_weights, sample_time, _has_history, _load = _D.time_weights, _D.sample_time, _D._has_history, _D.load_state_dict

    def __init__(self, T):
        self.num_timesteps, self.Lt_history, self.Lt_count = T, None, None
        self.verified = None
        self.engine = type("E", (), {"load_state_dict": lambda self, sd: None})()

    def _report_selection(self):
        pass


@pytest.mark.parametrize("ds,q_type", VC.MODELS)
def test_time_weights_from_the_checkpoints_history(ds, q_type):
    fx = VC.fixture()
    p = f"{VC.name(ds, q_type)}/mixed/"
    d = _NoEngine(100)
    assert torch.equal(d.time_weights(), torch.ones(100) / 100)                       # no history: uniform
    d._load({"model.module.Lt_history": fx[p + "Lt_history"], "model.module.Lt_count": fx[p + "Lt_count"], "model.module.x": np.zeros(2)})
    assert d.Lt_history.device.type == "cpu" and d.Lt_history.dtype == torch.float32 and d.Lt_count.shape == (100,)
    assert np.allclose(d.time_weights().numpy(), fx[p + "pt_all"], rtol=1e-6, atol=0)
    assert np.array_equal(d.time_weights()[torch.from_numpy(fx["t_mixed"].astype(np.int64))].numpy(), d.time_weights().numpy()[fx["t_mixed"]])
    assert np.array_equal(d.Lt_history.numpy(), fx[p + "Lt_history"])                 # read, never written
    torch.manual_seed(0)
    t, pt = d.sample_time(256)
    assert t.dtype == torch.int64 and torch.equal(pt, d.time_weights()[t]) and 0 <= int(t.min()) and int(t.max()) < 100
    d._load({"Lt_history": fx[p + "Lt_history"], "Lt_count": np.full(100, 10.0, np.float32)})   # some t visited <= 10 times: uniform
    assert torch.equal(d.time_weights(), torch.ones(100) / 100)
    t, pt = d.sample_time(32)
    assert torch.equal(pt, torch.full((32,), 1.0 / 100))
