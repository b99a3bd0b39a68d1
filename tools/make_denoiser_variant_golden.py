"""Reference fixtures of the denoiser variants the reference's LayoutDM class can train beyond its default (elem_attr positions,
adalayernorm): the real reference (imported through oracle/ref_harness.py, CPU) on its own backbone, Rico25, LAYOUTS layouts, with
the synthetic checkpoint of layout_dm_amd.synthetic.synth_state_dict(perturb=True, pos_emb=, timestep_type=).

    python tools/make_denoiser_variant_golden.py [out_dir]      ->  tests/golden/variants/<variant>.npz  (data only)

Variants (VARIANTS)
  vanilla_default   q_type=vanilla + pos_emb=default: the reference's shipped preset experiment/vqdiffusion.yaml
  abs               timestep_type=adalayernorm_abs   (SinusoidalPosEmb, transformer_utils.py:34-49)
  none              timestep_type=None               (norm1 = nn.LayerNorm, transformer_utils.py:155)
  adainnorm         timestep_type=adainnorm          (AdaInsNorm, transformer_utils.py:86-100)
  adainnorm_abs     timestep_type=adainnorm_abs

Contents of each file
  manifest_names / manifest_shapes   the reference's state_dict(): names and shapes (shapes as "a,b" strings; "" for a scalar)
  weight_seed                        seed of the synthetic checkpoint
  ts, tokens_<t>, logits_<t>         transformer logits (nn_lib.py:191-237) of LAYOUTS layouts at t = 99 and 1, one layout at t = 0
  post_<t>                           q_posterior(predict_start(...)) log-probabilities at the same t
  traj_steps / traj_states_after     the greedy sample() with num_timesteps = 10 of T = 100 (base.py:293-371): state after each step
  traj_chosen                        indices of the steps whose state BEFORE the step is fit for teacher-forced greedy tests: the
                                     top-two gap of the log-probabilities the reference decides on (base.py:215-240) exceeds 1e-3 x
                                     max |logit| at every token
  the two *_abs files also:
  sinusoid                           the reference's own [T][D] float32 table, norm1.emb(arange(T))
  logits_patched_<t>                 the reference's logits with restated_sinusoid(T, D) in place of its own table in every block

The weight seed is 1, the seed of the default variant's goldens (oracle/make_golden.py WEIGHT_SEED), so that an engine's error on a
variant can be set against its error on tests/golden/rico25_step_cases.npz."""
from __future__ import annotations

import dataclasses
import os
import sys
from typing import NamedTuple, Optional

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from layout_dm_amd import synthetic       # noqa: E402
from oracle import ref_harness as rh      # noqa: E402
from oracle import spec as SP             # noqa: E402

SPEC = synthetic.RICO25
LAYOUTS = 2
TS = ((99, LAYOUTS), (1, LAYOUTS), (0, 1))      # (timestep, layouts)
T_EVAL = 10
GAP_REL = 1e-3
WEIGHT_SEED = 1
RESCALE_STEPS = 4000.0


class Variant(NamedTuple):
    name: str
    q_type: str = "constrained"
    pos_emb: str = "elem_attr"
    timestep_type: Optional[str] = "adalayernorm"

    @property
    def is_abs(self) -> bool:
        return bool(self.timestep_type) and self.timestep_type.endswith("_abs")

    @property
    def instance_norm(self) -> bool:
        return bool(self.timestep_type) and self.timestep_type.startswith("adainnorm")


VARIANTS = {v.name: v for v in (
    Variant("vanilla_default", q_type="vanilla", pos_emb="default"),
    Variant("abs", timestep_type="adalayernorm_abs"),
    Variant("none", timestep_type=None),
    Variant("adainnorm", timestep_type="adainnorm"),
    Variant("adainnorm_abs", timestep_type="adainnorm_abs"),
)}


def state_dict(v: Variant, seed: int = WEIGHT_SEED, spec=SPEC, prefix: str = ""):
    """The variant's synthetic checkpoint: layout_dm_amd.synthetic's weights; q_type=vanilla swaps the per-attribute schedule buffers
    for the one un-prefixed set vanilla.py:66-73 registers (oracle/spec.py)."""
    sd = synthetic.synth_state_dict(spec, seed=seed, perturb=True, prefix="", pos_emb=v.pos_emb, timestep_type=v.timestep_type)
    if v.q_type == "vanilla":
        per_attr = set(synthetic.schedule_buffers(spec))
        ospec = SP.ModelSpec(**dataclasses.asdict(spec))
        sd = {**{k: a for k, a in sd.items() if k not in per_attr}, **SP.schedule_buffers(ospec, "vanilla")}
    return {prefix + k: a for k, a in sd.items()}


def _sinusoid_arg32(T: int, D: int) -> np.ndarray:
    """[T][D / 2] float32 arguments x_t * f_k, every step in float64 rounded to float32 where the reference rounds."""
    f32, f64 = np.float32, np.float64
    half = D // 2
    x = ((np.arange(T).astype(f32).astype(f64) / f64(f32(T))).astype(f32).astype(f64) * RESCALE_STEPS).astype(f32)
    c = f32(-(np.log(10000.0) / (half - 1)))
    e = (np.arange(half).astype(f32).astype(f64) * f64(c)).astype(f32)
    freq = np.exp(e.astype(f64)).astype(f32)
    return (x.astype(f64)[:, None] * freq.astype(f64)[None, :]).astype(f32)


def restated_sinusoid(T: int, D: int) -> np.ndarray:
    """SinusoidalPosEmb(T, D)(arange(T)) (transformer_utils.py:34-49) with every step evaluated in float64 and rounded to float32
    where the reference rounds (layout_dm_amd/csrc/ldm_variant_core.h): [T][D] float32, sines | cosines."""
    arg = _sinusoid_arg32(T, D).astype(np.float64)
    return np.concatenate([np.sin(arg), np.cos(arg)], axis=1).astype(np.float32)


def sinusoid_args(T: int, D: int) -> np.ndarray:
    """|x_t * f_k|, what the sine and the cosine of an entry are taken of, for every entry of the [T][D] table, float64."""
    arg = np.abs(_sinusoid_arg32(T, D).astype(np.float64))
    return np.concatenate([arg, arg], axis=1)


def sinusoid_x(T: int, D: int) -> np.ndarray:
    """x_t = t / T * 4000, the argument SinusoidalPosEmb.forward is called with after its rescaling, for every entry of the [T][D]
    table (constant along a row), float64 of the float32 value."""
    f32, f64 = np.float32, np.float64
    x = ((np.arange(T).astype(f32).astype(f64) / f64(f32(T))).astype(f32).astype(f64) * RESCALE_STEPS).astype(f32).astype(f64)
    return np.repeat(x[:, None], D, axis=1)


def sinusoid_bound(T: int, D: int) -> np.ndarray:
    """Per-entry bound of a correctly rounded table against the reference's own, 2^-23 |x_t| + 2^-22: torch's float32 exp may be one
    ulp off — at most 2^-23 absolute, every frequency being <= 1 — which moves the product by at most 2^-23 |x_t|; plus the output
    roundings."""
    return 2.0 ** -23 * sinusoid_x(T, D) + 2.0 ** -22


def build_reference(v: Variant):
    """The reference's diffusion module for the variant, as oracle.ref_harness.build_reference_model builds the default one."""
    rh.install_stubs()
    from trainer.helpers.layout_tokenizer import LayoutSequenceTokenizer
    from trainer.models.base_model import BaseModel
    from trainer.models.categorical_diffusion.constrained import ConstrainedMaskAndReplaceDiffusion
    from trainer.models.categorical_diffusion.vanilla import VanillaMaskAndReplaceDiffusion
    from trainer.models.common.util import shrink

    data_cfg, dataset_cfg, backbone_cfg = rh.make_cfgs("rico25", SPEC.n_step)
    backbone_cfg.encoder_layer.timestep_type = v.timestep_type
    torch.manual_seed(0)
    tok = LayoutSequenceTokenizer(data_cfg, dataset_cfg)
    assert tok.N_total == SPEC.n_class and tok.max_token_length == SPEC.seq_len
    cls = VanillaMaskAndReplaceDiffusion if v.q_type == "vanilla" else ConstrainedMaskAndReplaceDiffusion
    m = cls(backbone_cfg=shrink(backbone_cfg, 29 / 32), num_classes=tok.N_total, max_token_length=tok.max_token_length,
            num_timesteps=SPEC.n_step, pos_emb=v.pos_emb, transformer_type="flattened", auxiliary_loss_weight=0.1, tokenizer=tok)
    m.apply(lambda mod: BaseModel._init_weights(None, mod))
    m.eval()
    return m, tok


def manifest(m):
    sd = m.state_dict()
    names = sorted(sd)
    return np.array(names), np.array([",".join(str(int(n)) for n in sd[k].shape) for k in names])


def random_valid_tokens(spec, B, mask_frac, g):
    tokens = torch.empty(B, spec.seq_len, dtype=torch.long)
    for a in range(spec.n_attr):
        ids = torch.as_tensor(spec.full_ids(a))
        tokens[:, a::spec.n_attr] = ids[torch.randint(0, len(ids) - 1, (B, spec.max_elem), generator=g)]   # any live class but [MASK]
    tokens[torch.rand(B, spec.seq_len, generator=g) < mask_frac] = spec.mask_id
    return tokens


class _Table(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, t):
        return self.table[t]


def chosen_states(m, spec, states_after):
    """Steps of the greedy trajectory whose state before the step has the top-two gap of the reference's log-probabilities above
    GAP_REL x max |logit| at EVERY token -> (indices, whether one of them unmasks tokens)."""
    from trainer.models.categorical_diffusion.util import index_to_log_onehot

    from layout_dm_amd.diffusion import timestep_schedule

    n, B, _ = states_after.shape
    t_model, t_post = timestep_schedule(spec.n_step, n)
    before = torch.cat([torch.full((1, B, spec.seq_len), spec.mask_id, dtype=torch.long), states_after[:-1]])
    chosen, moves = [], False
    for i in range(n):
        tm, tp = torch.full((B,), t_model[i], dtype=torch.long), torch.full((B,), t_post[i], dtype=torch.long)
        with torch.no_grad():
            logits = m.transformer(before[i], timestep=tm)["logits"]
            lz = index_to_log_onehot(before[i], spec.n_class)
            logp = m.q_posterior(m.predict_start(lz, tm), lz, tp)
        assert torch.equal(logp.argmax(dim=1), states_after[i]), i
        top2 = logp.topk(2, dim=1).values
        if bool(((top2[:, 0] - top2[:, 1]) > GAP_REL * float(logits.abs().max())).all()):
            chosen.append(i)
            moves |= bool(((before[i] == spec.mask_id) & (states_after[i] != spec.mask_id)).any())
    return chosen, moves


def cases(v: Variant, weight_seed: int = WEIGHT_SEED):
    spec = SPEC
    m, _ = build_reference(v)      # (installs the import stubs)
    from trainer.models.categorical_diffusion.util import index_to_log_onehot

    from layout_dm_amd.diffusion import timestep_schedule

    names, shapes = manifest(m)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in state_dict(v, weight_seed).items()})   # (strict: the key sets are equal)
    out = {"manifest_names": names, "manifest_shapes": shapes, "weight_seed": np.int32(weight_seed),
           "ts": np.array([t for t, _ in TS], np.int32)}
    g = torch.Generator().manual_seed(123)
    toks = {}
    for t, B in TS:
        tokens = toks[t] = random_valid_tokens(spec, B, t / (spec.n_step - 1), g)
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
    out["traj_steps"] = np.array(timestep_schedule(spec.n_step, T_EVAL)[0], np.int32)
    out["traj_states_after"] = states.numpy().astype(np.int16)
    chosen, moves = chosen_states(m, spec, states)
    out["traj_chosen"] = np.array(chosen, np.int32)
    if v.is_abs:
        layers = m.transformer.backbone.layers
        with torch.no_grad():
            out["sinusoid"] = layers[0].norm1.emb(torch.arange(spec.n_step)).numpy()
        assert out["sinusoid"].shape == (spec.n_step, spec.d_model) and out["sinusoid"].dtype == np.float32
        table = torch.from_numpy(restated_sinusoid(spec.n_step, spec.d_model))
        for layer in layers:
            layer.norm1.emb = _Table(table)
        for t, B in TS:
            with torch.no_grad():
                out[f"logits_patched_{t}"] = m.transformer(toks[t], timestep=torch.full((B,), t, dtype=torch.long))["logits"].numpy()
    return out, chosen, moves


def main(out_dir=None):
    out_dir = out_dir or os.path.join(ROOT, "tests", "golden", "variants")
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for v in VARIANTS.values():
        out, chosen, moves = cases(v)
        path = os.path.join(out_dir, v.name + ".npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(f"{path}: {size} bytes; chosen steps {chosen}, unmasking among them: {moves}", file=sys.stderr)
        assert size < (1 << 20), "a fixture must stay below 1 MiB"
        assert chosen, "no state with a clear greedy decision at every token"
        paths.append(path)
    return paths


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
