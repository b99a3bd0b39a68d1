"""Reference fixture of a WIDE vocabulary: the real reference (imported through oracle/ref_harness.py, CPU) with
num_bin_bboxes = 64 on Rico25 — 25 categories + 4 x 64 bins + [PAD] + [MASK] = 283 classes — on the synthetic checkpoint of
oracle/synth.py (the reference's init plus perturbed biases, as oracle/make_golden.py loads it).

    python tools/make_wide_vocab_golden.py [out_dir]      ->  tests/golden/wide_vocab/wide_vocab_rico25_64.npz  (data only)

(A directory of its own, like tests/golden/vb/: every .npz directly under tests/golden/ is one of oracle/make_golden.py's, and
tests/test_oracle_vs_reference.py holds that directory's listing to what that generator writes.)

Contents
  weight_seed                     seed of oracle.synth.synth_state_dict(perturb=True) the fixture was made with
  ts, tokens_<t>, logits_<t>      transformer logits (nn_lib.py:191-237) of LAYOUTS layouts at t = 99 and 1, one layout at t = 0
  post_<t>                        q_posterior(predict_start(...)) log-probabilities at t in {0, 1, 99} (constrained.py:135-206)
  traj_steps / traj_states_after  the greedy sample() with num_timesteps = 10 of T = 100 (base.py:293-371): state after each step
  traj_chosen                     indices of the steps whose state BEFORE the step is fit for teacher-forced greedy tests: the
                                  restated step's top-two gap exceeds 1e-3 x max |logit| at every token (oracle/restatement.py)
  decode_bbox / _label / _mask    LayoutSequenceTokenizer.decode of the final tokens (layout_tokenizer.py:255-266)

The weight seed is the first of 1, 2, ... for which at least MIN_CHOSEN steps qualify, among them one that unmasks tokens.
LAYOUTS = 2: three layouts put the file above the 1 MiB limit of a committed file (logits of 125 x 283 floats per layout)."""
from __future__ import annotations

import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_harness as rh      # noqa: E402
from oracle import restatement as R       # noqa: E402
from oracle import spec as SP             # noqa: E402
from oracle import synth                  # noqa: E402

NAME = "wide_vocab_rico25_64.npz"
SPEC = dataclasses.replace(SP.RICO25, name="rico25_64", n_bin=64)
LAYOUTS = 2
TS = ((99, LAYOUTS), (1, LAYOUTS), (0, 1))      # (timestep, layouts)
T_EVAL = 10
GAP_REL = 1e-3
MIN_CHOSEN = 5


def build_reference(n_bin=SPEC.n_bin):
    """The reference's diffusion module and tokenizer as oracle.ref_harness.build_reference_model builds them, on this tool's
    own data config (num_bin_bboxes = n_bin)."""
    rh.install_stubs()
    from trainer.helpers.layout_tokenizer import LayoutSequenceTokenizer
    from trainer.models.base_model import BaseModel
    from trainer.models.categorical_diffusion.constrained import ConstrainedMaskAndReplaceDiffusion
    from trainer.models.common.util import shrink

    data_cfg, dataset_cfg, backbone_cfg = rh.make_cfgs("rico25", SPEC.n_step)
    data_cfg.num_bin_bboxes = n_bin
    torch.manual_seed(0)
    tok = LayoutSequenceTokenizer(data_cfg, dataset_cfg)
    assert tok.N_total == SPEC.n_class and tok.N_bbox_per_var == n_bin and tok.max_token_length == SPEC.seq_len
    m = ConstrainedMaskAndReplaceDiffusion(backbone_cfg=shrink(backbone_cfg, 29 / 32), num_classes=tok.N_total,
                                           max_token_length=tok.max_token_length, num_timesteps=SPEC.n_step, pos_emb="elem_attr",
                                           transformer_type="flattened", auxiliary_loss_weight=0.1, tokenizer=tok)
    m.apply(lambda mod: BaseModel._init_weights(None, mod))
    m.eval()
    return m, tok


def random_valid_tokens(spec, B, mask_frac, g):
    tokens = torch.empty(B, spec.seq_len, dtype=torch.long)
    for a in range(spec.n_attr):
        ids = torch.as_tensor(spec.full_ids(a))
        tokens[:, a::spec.n_attr] = ids[torch.randint(0, len(ids) - 1, (B, spec.max_elem), generator=g)]   # any live class but [MASK]
    tokens[torch.rand(B, spec.seq_len, generator=g) < mask_frac] = spec.mask_id
    return tokens


def chosen_states(W, spec, states_after):
    """Steps of the greedy trajectory whose state before the step has the restated step's top-two gap above GAP_REL x max |logit|
    at EVERY token -> (indices, whether one of them unmasks tokens)."""
    n, B, _ = states_after.shape
    steps = R.timestep_list(spec.n_step, n)
    before = torch.cat([torch.full((1, B, spec.seq_len), spec.mask_id, dtype=torch.long), states_after[:-1]])
    chosen, moves, prev = [], False, spec.n_step
    for i, t in enumerate(steps):
        _, logits, logp = R.single_step(W, spec, before[i], t, {"name": "deterministic"}, skip_step=prev - t - 1, return_all=True)
        prev = t
        top2 = logp.topk(2, dim=1).values
        if bool(((top2[:, 0] - top2[:, 1]) > GAP_REL * float(logits.abs().max())).all()):
            chosen.append(i)
            moves |= bool(((before[i] == spec.mask_id) & (states_after[i] != spec.mask_id)).any())
    return chosen, moves


def cases(weight_seed):
    spec = SPEC
    m, tok = build_reference()      # (installs the import stubs)
    from trainer.models.categorical_diffusion.util import index_to_log_onehot

    ssd = synth.synth_state_dict(spec, seed=weight_seed, perturb=True, prefix="")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ssd.items()})
    out = {"weight_seed": np.int32(weight_seed), "ts": np.array([t for t, _ in TS], np.int32)}
    g = torch.Generator().manual_seed(123)
    for t, B in TS:
        tokens = random_valid_tokens(spec, B, t / (spec.n_step - 1), g)
        tt = torch.full((B,), t, dtype=torch.long)
        with torch.no_grad():
            logits = m.transformer(tokens, timestep=tt)["logits"]
            lz = index_to_log_onehot(tokens, spec.n_class)
            post = m.q_posterior(m.predict_start(lz, tt), lz, tt)
        out[f"tokens_{t}"] = tokens.numpy().astype(np.int16)
        out[f"logits_{t}"] = logits.numpy()
        out[f"post_{t}"] = post.numpy()
    torch.manual_seed(0)
    with torch.no_grad():
        full = m.sample(batch_size=LAYOUTS, cond=None, sampling_cfg=rh.sampling_cfg("deterministic", num_timesteps=T_EVAL),
                        get_intermediate_results=True)
    states = torch.stack(full)
    out["traj_steps"] = np.array(R.timestep_list(spec.n_step, T_EVAL), np.int32)
    out["traj_states_after"] = states.numpy().astype(np.int16)
    W = R.as_torch_weights(synth.synth_state_dict(spec, seed=weight_seed, perturb=True))
    chosen, moves = chosen_states(W, spec, states)
    out["traj_chosen"] = np.array(chosen, np.int32)
    dec = tok.decode(states[-1].clone())
    out["decode_bbox"], out["decode_label"], out["decode_mask"] = dec["bbox"].numpy(), dec["label"].numpy(), dec["mask"].numpy()
    return out, len(chosen) >= MIN_CHOSEN and moves


def main(out_dir=None):
    out_dir = out_dir or os.path.join(ROOT, "tests", "golden", "wide_vocab")
    os.makedirs(out_dir, exist_ok=True)
    for weight_seed in range(1, 9):
        out, ok = cases(weight_seed)
        print(f"weight seed {weight_seed}: chosen steps {out['traj_chosen'].tolist()}" + ("" if ok else " — too few, next seed"), file=sys.stderr)
        if ok:
            break
    else:
        raise SystemExit("no weight seed gives enough states with a clear greedy decision")
    path = os.path.join(out_dir, NAME)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes", file=sys.stderr)
    assert size < (1 << 20), "the fixture must stay below 1 MiB"
    return path


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
