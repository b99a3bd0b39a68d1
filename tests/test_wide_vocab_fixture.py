"""CPU: tests/golden/wide_vocab/wide_vocab_rico25_64.npz — the real reference at 64 bins per coordinate (283 classes), written by
tools/make_wide_vocab_golden.py — against the oracle restatement, within the tolerances tests/test_oracle_golden.py holds the
32-bin fixtures to (logits 1e-5 x max |logit|, posterior 1e-5 and the same argmax, greedy trajectory and decode exactly); and,
where the reference can be imported, the tool writes the committed file again bit for bit."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import ref_harness
from oracle import restatement as R
from oracle import spec as SP
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = os.path.join("wide_vocab", "wide_vocab_rico25_64.npz")
SPEC = dataclasses.replace(SP.RICO25, name="rico25_64", n_bin=64)


@pytest.fixture(scope="module")
def fx(golden_dir):
    with np.load(os.path.join(golden_dir, NAME)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def W(fx):
    return R.as_torch_weights(synth.synth_state_dict(SPEC, seed=int(fx["weight_seed"]), perturb=True))


def test_fixture_is_data_of_the_expected_shape(fx, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, NAME)) < (1 << 20)
    assert SPEC.n_class == 283 and sorted(fx["ts"].tolist()) == [0, 1, 99]
    assert all(v.dtype.kind in "fiub" for v in fx.values())            # numbers only: nothing a loader could execute
    for t in fx["ts"]:
        B = fx[f"tokens_{t}"].shape[0]
        assert fx[f"logits_{t}"].shape == (B, SPEC.seq_len, 283) and fx[f"post_{t}"].shape == (B, 283, SPEC.seq_len)
        assert (fx[f"tokens_{t}"] == SPEC.mask_id).any() or t == 0
    assert sum(fx[f"tokens_{t}"].shape[0] >= 2 for t in fx["ts"]) >= 2   # logits of at least two layouts at two timesteps
    assert fx["traj_states_after"].shape[0] == 10 and fx["traj_steps"].tolist() == R.timestep_list(100, 10)


def test_logits_and_posterior(fx, W):
    for t in fx["ts"]:
        t = int(t)
        tokens = torch.from_numpy(fx[f"tokens_{t}"].astype(np.int64))
        ref_logits, ref_post = torch.from_numpy(fx[f"logits_{t}"]), torch.from_numpy(fx[f"post_{t}"])
        scale = max(ref_logits.abs().max().item(), 1.0)
        assert (R.denoiser_logits(W, SPEC, tokens, t) - ref_logits).abs().max().item() <= 1e-5 * scale
        assert (R.denoiser_logits(W, SPEC, tokens, t, dtype=torch.float64).float() - ref_logits).abs().max().item() <= 1e-5 * scale
        post = R.q_posterior(W, SPEC, R.predict_start_from_logits(ref_logits), tokens, t)
        assert (post - ref_post).abs().max().item() <= 1e-5
        assert torch.equal(post.argmax(1), ref_post.argmax(1))
        dead = ref_post == ref_post.min()
        assert torch.equal(post[dead], ref_post[dead])


def test_greedy_trajectory_and_chosen_states(fx, W):
    ref = torch.from_numpy(fx["traj_states_after"].astype(np.int64))
    mine = torch.stack(R.sample_loop(W, SPEC, ref.shape[1], {"name": "deterministic", "num_timesteps": 10}, get_intermediate_results=True))
    assert torch.equal(mine, ref)
    assert (ref[-1] != SPEC.mask_id).all()
    # the states the GPU tests teacher-force: a clear greedy decision at every token, and not only steps that leave [MASK] alone
    spec = importlib.util.spec_from_file_location("make_wide_vocab_golden", os.path.join(ROOT, "tools", "make_wide_vocab_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    chosen, moves = tool.chosen_states(W, SPEC, ref)
    assert chosen == fx["traj_chosen"].tolist() and len(chosen) >= tool.MIN_CHOSEN and moves


def test_decode_of_the_final_tokens(fx):
    dec = R.decode_layouts(SPEC, torch.from_numpy(fx["traj_states_after"][-1].astype(np.int64)))
    assert dec["bbox"].dtype == torch.float32 and np.array_equal(dec["bbox"].numpy(), fx["decode_bbox"])
    assert np.array_equal(dec["label"].numpy(), fx["decode_label"]) and np.array_equal(dec["mask"].numpy(), fx["decode_mask"])
    assert fx["decode_mask"].any()


@pytest.mark.skipif(not ref_harness.reference_importable(), reason="the reference implementation is not on this machine")
def test_tool_regenerates_the_fixture_bit_for_bit(fx, tmp_path):
    spec = importlib.util.spec_from_file_location("make_wide_vocab_golden", os.path.join(ROOT, "tools", "make_wide_vocab_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = tool.main(str(tmp_path))
    assert os.path.basename(path) == os.path.basename(NAME)
    with np.load(path) as z:
        again = {k: z[k] for k in z.files}
    assert sorted(again) == sorted(fx)
    for k in fx:
        assert again[k].dtype == fx[k].dtype and np.array_equal(again[k], fx[k]), k
