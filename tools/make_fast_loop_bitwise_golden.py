"""Dev tool (needs the MI355X): record what the fast mode's stack kernels compute, bit for bit, so that a change that must
not move a single bit (instruction scheduling, LDS maps, register moves) can prove it.

    python tools/make_fast_loop_bitwise_golden.py [out.npz]      # default tests/golden/fast_loop_bitwise/parent.npz

Run it at the commit whose results are to be kept; tests/test_fast_loop_bitwise_gpu.py replays the same cases on the
tree under test and requires EQUALITY.  Cases (synthetic weights, seed 0; B = 3 layouts, first_layout = 5; 10 reverse
steps strided over the 100-step model; one workgroup per layout, so ten steps enter the FFN ring of each of the four
layers ten times — both parities of its double iteration and the odd single iteration behind them):

  * vocabularies Rico25 and PubLayNet at S = 125, and Rico25 at S = 105 (21 elements: 23 padded rows per layout);
  * the tokens after EVERY step for the samplers random / deterministic / top_p, unconditional and cond = c;
  * the logits of one denoiser pass (the HEAD 1 form of the kernel) at two timesteps: sha256 of their bit pattern and
    every 97th word of it as uint32.
"""
import dataclasses
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "fast_loop_bitwise", "parent.npz")
B, FIRST_LAYOUT, SEED, N_STEPS = 3, 5, 17, 10
SAMPLERS = ("random", "deterministic", "top_p")
LOGIT_T = (40, 5)
LOGIT_STRIDE = 97


def specs():
    from oracle import spec as SP

    return {
        "rico25": SP.RICO25,
        "publaynet": SP.PUBLAYNET,
        "rico25_s105": dataclasses.replace(SP.RICO25, name="rico25_e21", max_elem=21),
    }


def probe_tokens(spec, seed=0):
    """B rows of valid tokens, half of them [MASK] (the input of the single denoiser passes)."""
    rng = np.random.RandomState(seed)
    tok = np.empty((B, spec.seq_len), dtype=np.int64)
    for a in range(spec.n_attr):
        ids = np.asarray(spec.full_ids(a))
        tok[:, a::spec.n_attr] = ids[rng.randint(0, len(ids) - 1, size=(B, spec.max_elem))]
    tok[rng.rand(B, spec.seq_len) < 0.5] = spec.mask_id
    return tok


def record(device="cuda:0"):
    """name -> array of everything the golden file holds, computed by the library of this tree."""
    import torch

    from layout_dm_amd.binding import Engine
    from oracle import restatement as R
    from oracle import synth

    out = {}
    for key, spec in specs().items():
        sd = synth.synth_state_dict(spec, seed=0, perturb=True)
        steps = R.timestep_list(spec.n_step, N_STEPS)
        assert len(steps) == N_STEPS
        e = Engine(n_category=spec.n_category, n_bin=spec.n_bin, max_elem=spec.max_elem, d_model=spec.d_model,
                   n_head=spec.n_head, d_ff=spec.d_ff, n_layer=spec.n_layer, n_step=spec.n_step, precision="fast", max_batch=8)
        e.load_state_dict(sd)
        c = synth.synth_cond_c(spec, B, seed=4)
        for sampler in SAMPLERS:
            cfg = {"name": sampler, "temperature": 1.0, "top_p": 0.9}
            tok = torch.full((B, spec.seq_len), spec.mask_id, dtype=torch.int32, device=device)
            _, inter = e.sample_loop(tok, steps, steps, cfg, seed=SEED, first_layout=FIRST_LAYOUT, intermediates=True, use_graph=True)
            out[f"{key}/{sampler}/uncond"] = inter.cpu().numpy().astype(np.int16)
            cond = {"seq": c["seq"], "mask": c["mask"], "type": "c"}
            tok = torch.from_numpy(c["seq"]).int().to(device)
            _, inter = e.sample_loop(tok, steps, steps, cfg, cond=cond, seed=SEED, first_layout=FIRST_LAYOUT, intermediates=True,
                                     use_graph=True)
            out[f"{key}/{sampler}/cond_c"] = inter.cpu().numpy().astype(np.int16)
        probe = torch.from_numpy(probe_tokens(spec)).int().to(device)
        for t in LOGIT_T:
            bits = e.denoise_logits(probe, t).cpu().numpy().view(np.uint32).ravel()
            out[f"{key}/logits_t{t}/sha256"] = np.frombuffer(hashlib.sha256(bits.tobytes()).digest(), dtype=np.uint8).copy()
            out[f"{key}/logits_t{t}/every{LOGIT_STRIDE}"] = bits[::LOGIT_STRIDE].copy()
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
