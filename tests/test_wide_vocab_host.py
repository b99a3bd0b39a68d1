"""CPU: the wide-vocabulary forms of the step tail (layout_dm_amd/csrc/ldm_post_token.h) compiled for the host
(tests/cpu_wide_vocab_check.cpp).

  * the two slot maps kernels_post.hip / kernels_vb.hip instantiate above 192 classes cover every candidate of the four edge
    vocabularies exactly once and mark nothing beyond;
  * the one-lane form at 130 live classes (128 bins + [PAD] + [MASK]) draws R.single_step's tokens on identical uniforms for all
    five samplers."""
import io
import struct

import numpy as np
import pytest
import torch

from oracle import restatement as R

import _hostbuild as HB
import _wide_vocab as WV


@pytest.fixture(scope="module")
def harness():
    return HB.host_program("cpu_wide_vocab_check", extra=("-Wextra",))


@pytest.mark.parametrize("n_category,n_bin", WV.VOCABS, ids=WV.VOCAB_IDS)
def test_slot_maps_own_every_candidate_exactly_once(harness, n_category, n_bin):
    r = HB.run_host(harness, "slots", n_category, n_bin)
    assert r.returncode == 0, r.stderr
    C = n_category + 4 * n_bin + 2
    live = (n_category + 2) + 4 * (n_bin + 2)
    assert r.stdout.split() == ["ok", str(2 * live + 5 * C + C)]     # live + host maps, full map per attribute, vanilla


def _run(harness, tmp_path, spec, W, tokens, t_post, logits, cfg, step):
    B, S = tokens.shape
    C, A = spec.n_class, spec.n_attr
    N = B * S
    pos = np.tile(np.arange(S, dtype=np.int32), B)
    attr = pos % A
    start = np.array([int(spec.full_ids(a)[0]) for a in range(A)], np.int32)[attr]
    count = np.array([len(spec.full_ids(a)) - 2 for a in range(A)], np.int32)[attr]
    layout = np.repeat(np.arange(B, dtype=np.uint64), S) + np.uint64(WV.FIRST_LAYOUT)
    with io.BytesIO() as f:
        f.write(np.array([0x4C444D31, N, C, spec.pad_id, spec.mask_id, WV.KINDS[cfg["name"]], int(cfg.get("top_k", 1)), 1, 0, 0],
                         np.int32).tobytes())
        f.write(np.array([cfg.get("temperature", 1.0), cfg.get("top_p", 1.0)], np.float32).tobytes())
        f.write(struct.pack("<Q", WV.SEED))
        for arr in (tokens.numpy().reshape(-1), start, count, np.full(N, -1), np.zeros(N), np.zeros(N), pos, np.full(N, step)):
            f.write(np.ascontiguousarray(arr, np.int32).tobytes())
        f.write(layout.tobytes())
        f.write(np.ascontiguousarray(WV.sched_rows(spec, W, t_post)[attr], np.float32).tobytes())
        f.write(np.ascontiguousarray(logits.numpy().reshape(N, C), np.float32).tobytes())
        rc, raw = HB.run_host_io(harness, tmp_path, f.getvalue(), "draw")
    assert rc == 0, rc
    return torch.from_numpy(np.frombuffer(raw, np.int32).astype(np.int64)).view(B, S)


def _draw_cases(harness, tmp_path):
    """Every sampler setting of WV.sampler_cfgs at 519 classes (5 categories, 128 bins: live sets of 7 and 130), 25 layouts at
    t in {0, 5, 9}: 1 500 tokens per setting.  A stochastic draw may differ from the oracle's where float32 rounding moves a CDF
    edge across the uniform: the rate tests/test_post_token_scalar.py allows (2 per 2 000 tokens) on these 1 500 is 1; greedy and
    the samplers with nothing left to draw equal the oracle wherever its top-two gap exceeds float32 rounding (1e-4)."""
    spec, _, W = WV.tiny_model(5, 128)
    assert max(spec.sub_vocab_size(a) for a in range(spec.n_attr)) == 130
    bad, total = {}, 0
    for step, t in enumerate((0, 5, 9)):
        toks = WV.states(spec, B=25, seed=step)
        _, logits, logp = R.single_step(W, spec, toks, t, {"name": "deterministic"}, return_all=True)
        top2 = logp.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-4
        total += toks.numel()
        for name, cfg in WV.sampler_cfgs(spec, logp):
            out = _run(harness, tmp_path, spec, W, toks, t, logits, cfg, step)
            ref = WV.oracle_draw(logp, cfg, step)
            for a in range(spec.n_attr):   # never a class outside the position's sub-vocabulary
                assert torch.isin(out[:, a::spec.n_attr], torch.as_tensor(spec.full_ids(a))).all(), name
            if name in ("deterministic", "top_k1", "top_p_below_max"):
                assert torch.equal(out[clear], logp.argmax(1)[clear]), (name, t)
            n = WV.top_p_one_cut_is_rounding(out, ref, logp, cfg, step) if name == "top_p1.0" else int((out != ref).sum())
            bad[name] = bad.get(name, 0) + n
    return bad, total


def test_one_lane_form_at_130_live_classes_draws_the_oracles_tokens(harness, tmp_path):
    bad, total = _draw_cases(harness, tmp_path)
    print(f"[host form, 130 live classes] mismatches per setting over {total} tokens: {bad}")
    assert set(bad) >= {"deterministic", "random", "top_p0.9", "top_k_live", "gumbel"}
    assert max(bad.values()) <= 2 * total // 2000, bad


def test_one_lane_form_under_address_and_undefined_sanitizers(tmp_path):
    """the same cases and the slot maps on the ASan + UBSan build of the program: 130 slots of l0 / lp, 2 x 130 floats of scratch"""
    exe = HB.host_program("cpu_wide_vocab_check", sanitize=True, extra=("-Wextra",))
    for n_category, n_bin in WV.VOCABS:
        assert HB.run_host(exe, "slots", n_category, n_bin).returncode == 0
    bad, total = _draw_cases(exe, tmp_path)
    assert max(bad.values()) <= 2 * total // 2000, bad
