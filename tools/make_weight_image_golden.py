"""Dev tool (needs the MI355X): record what every engine computes from a freshly loaded checkpoint, bit for bit, so that a change to
the weights path (layout_dm_amd/csrc/ldm_weights.cpp: fp16 / split copies, LDS images, padded biases, load-time tables) that must
not move a single bit can prove it.

    python tools/make_weight_image_golden.py [out.npz]      # default tests/golden/weight_images/parent.npz

Run it at the commit whose results are to be kept; tests/test_weight_images_gpu.py replays the same cases on the tree under test
and requires EQUALITY.  Every case: a fresh engine (max_batch = 8), synthetic weights (seed 1, perturbed), LAYOUTS layouts of random
valid tokens (half of them [MASK]), ONE denoise_logits call at each of two timesteps; recorded: the sha256 of the logits' bit pattern
and every 97th word of it as uint32.  Cases (CASES):

  * the eleven configurations of tests/test_launch_sequence_gpu.py (LAUNCH_CASES: the same geometry, precision and knobs), the
    reference backbone cut to two layers (the fewest that catch a per-layer indexing slip) and 20 steps;
  * split and exact on 64 bins (283 classes: a vocabulary head of more tiles);
  * split on every non-default denoiser variant of tests/golden/variants/ (q_type vanilla + pos_emb default, *_abs, None, the two
    adainnorm kinds), the instance-norm ones on exact as well.

(The one-launch loop's parameter tables and images: tests/test_fast_loop_bitwise_gpu.py against its own recording.)"""
import contextlib
import dataclasses
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "weight_images", "parent.npz")
LAYOUTS, MAX_BATCH, WEIGHT_SEED, LOGIT_STRIDE = 5, 8, 1, 97
KNOBS = ("LDM_DEV", "LDM_X3_LNGEMM", "LDM_X3_ATTNOUT", "LDM_X3_HIDPANEL", "LDM_HYB_FFN", "LDM_FUSED_ATTN")
# id: (geometry, precision, knobs) — tests/test_launch_sequence_gpu.py CASES (the test holds the two tables against each other)
LAUNCH_CASES = {
    "fast": ("reference", "fast", {}),
    "fast_generic_geometry": ("small", "fast", {}),
    "exact": ("reference", "exact", {}),
    "split": ("reference", "split", {}),
    "mixed": ("reference", "mixed", {}),
    "hybrid": ("reference", "hybrid", {}),
    "split_lngemm_0": ("reference", "split", {"LDM_X3_LNGEMM": "0"}),
    "split_attnout_0": ("reference", "split", {"LDM_X3_ATTNOUT": "0"}),
    "split_hidpanel_0": ("reference", "split", {"LDM_X3_HIDPANEL": "0"}),
    "hybrid_ffn_0": ("reference", "hybrid", {"LDM_HYB_FFN": "0"}),
    "split_generic_geometry": ("small", "split", {}),
}
VARIANT_CASES = {   # id: (variant of tools/make_denoiser_variant_golden.py, precision)
    "variant_vanilla_default_split": ("vanilla_default", "split"),
    "variant_abs_split": ("abs", "split"),
    "variant_none_split": ("none", "split"),
    "variant_adainnorm_split": ("adainnorm", "split"),
    "variant_adainnorm_abs_split": ("adainnorm_abs", "split"),
    "variant_adainnorm_exact": ("adainnorm", "exact"),
    "variant_adainnorm_abs_exact": ("adainnorm_abs", "exact"),
}
WIDE_CASES = {"bins64_split": "split", "bins64_exact": "exact"}
CASES = (*LAUNCH_CASES, *WIDE_CASES, *VARIANT_CASES)


def geometries():
    from oracle import spec as SP

    ref = dataclasses.replace(SP.SPECS["rico25"], n_layer=2, n_step=20)
    return {"reference": ref,
            "small": dataclasses.replace(ref, name="small", d_model=256, n_head=4, d_ff=1024),
            "bins64": dataclasses.replace(ref, name="rico25_bins64", n_bin=64)}


def timesteps(spec):
    return (spec.n_step * 2 // 3, 1)


def probe_tokens(spec, seed=3):
    """LAYOUTS rows of valid tokens, half of them [MASK]."""
    rng = np.random.RandomState(seed)
    tok = np.empty((LAYOUTS, spec.seq_len), dtype=np.int64)
    for a in range(spec.n_attr):
        ids = np.asarray(spec.full_ids(a))
        tok[:, a::spec.n_attr] = ids[rng.randint(0, len(ids) - 1, size=(LAYOUTS, spec.max_elem))]
    tok[rng.rand(LAYOUTS, spec.seq_len) < 0.5] = spec.mask_id
    return tok


def case_setup(case, seed=WEIGHT_SEED):
    """-> (spec, precision, knobs, extra Engine arguments, state dict)"""
    from oracle import synth

    geo = geometries()
    if case in LAUNCH_CASES:
        g, precision, knobs = LAUNCH_CASES[case]
        return geo[g], precision, knobs, {}, synth.synth_state_dict(geo[g], seed=seed, perturb=True)
    if case in WIDE_CASES:
        return geo["bins64"], WIDE_CASES[case], {}, {}, synth.synth_state_dict(geo["bins64"], seed=seed, perturb=True)
    import make_denoiser_variant_golden as V

    name, precision = VARIANT_CASES[case]
    v = V.VARIANTS[name]
    vspec = dataclasses.replace(V.SPEC, n_layer=2, n_step=20)
    return geo["reference"], precision, {}, {"q_type": v.q_type, "timestep_type": v.timestep_type}, V.state_dict(v, seed=seed, spec=vspec)


@contextlib.contextmanager
def knob_env(knobs):
    """The create-time knobs (csrc/ldm_knobs.h) of one case in the environment, the caller's own put back afterwards."""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        if knobs:
            os.environ.update({"LDM_DEV": "1", **knobs})
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def make_engine(spec, precision, knobs, extra):
    from layout_dm_amd.binding import Engine

    with knob_env(knobs):
        return Engine(n_category=spec.n_category, n_bin=spec.n_bin, max_elem=spec.max_elem, d_model=spec.d_model, n_head=spec.n_head,
                      d_ff=spec.d_ff, n_layer=spec.n_layer, n_step=spec.n_step, precision=precision, max_batch=MAX_BATCH, **extra)


def logits_bits(e, spec, device="cuda:0"):
    """{t: the uint32 words of denoise_logits at t} on the probe tokens"""
    import torch

    probe = torch.from_numpy(probe_tokens(spec)).int().to(device)
    return {t: e.denoise_logits(probe, t).cpu().numpy().view(np.uint32).ravel() for t in timesteps(spec)}


def record(device="cuda:0", cases=CASES):
    """name -> array of everything the golden file holds, computed by the library of this tree."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    out = {}
    for case in cases:
        spec, precision, knobs, extra, sd = case_setup(case)
        e = make_engine(spec, precision, knobs, extra)
        try:
            e.load_state_dict(sd)
            for t, bits in logits_bits(e, spec, device).items():
                out[f"{case}/logits_t{t}/sha256"] = np.frombuffer(hashlib.sha256(bits.tobytes()).digest(), dtype=np.uint8).copy()
                out[f"{case}/logits_t{t}/every{LOGIT_STRIDE}"] = bits[::LOGIT_STRIDE].copy()
        finally:
            e.close()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    got = record()
    np.savez_compressed(path, **got)
    print(f"{path}: {len(got)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
