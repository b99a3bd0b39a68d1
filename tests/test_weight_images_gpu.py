"""Every engine's logits from a freshly loaded checkpoint against tests/golden/weight_images/parent.npz — what the SAME cases computed
at the commit before ldm_finalize_weights went to "plan on the host, build every derived buffer once from the checkpoint's host copy"
(tools/make_weight_image_golden.py records and documents the cases).  That change moves where the fp16 / split copies, LDS images,
padded biases and parameter tables are built, and no value in them, so the requirement is EQUALITY of the bit pattern of
denoise_logits: the eleven configurations of tests/test_launch_sequence_gpu.py, split and exact on 64 bins, split on every non-default
denoiser variant (the instance-norm ones on exact as well).  A second load on one handle — the derived set dropped and rebuilt —
gives the logits of a fresh handle.  (The one-launch loop, which reads the parameter tables: tests/test_fast_loop_bitwise_gpu.py.)"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_weight_image_golden as G      # noqa: E402
import test_launch_sequence_gpu as LS     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "weight_images", "parent.npz")


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_cases_are_the_launch_sequence_configurations_and_the_golden_holds_them_all(golden):   # (no device: runs with the CPU suite)
    assert set(G.LAUNCH_CASES) == set(LS.CASES)
    geo = G.geometries()
    for case, (spec, precision, knobs, _, _) in LS.CASES.items():
        g, gprecision, gknobs = G.LAUNCH_CASES[case]
        assert (gprecision, gknobs) == (precision, knobs), case
        cut = geo[g]
        assert (cut.d_model, cut.n_head, cut.d_ff, cut.n_category, cut.n_bin, cut.max_elem) == \
            (spec.d_model, spec.n_head, spec.d_ff, spec.n_category, spec.n_bin, spec.max_elem), case
        assert cut.n_layer == 2   # the fewest layers that catch a per-layer indexing slip
    assert set(golden) == {f"{case}/logits_t{t}/{what}" for case in G.CASES for t in G.timesteps(geo["reference"])
                           for what in ("sha256", f"every{G.LOGIT_STRIDE}")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", G.CASES)
def test_logits_bit_identical_to_the_recording(cuda, golden, case):
    got = G.record(cases=(case,))
    assert got, case
    for name, a in got.items():
        b = golden[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        diff = np.argwhere(a != b)
        assert diff.size == 0, f"{name}: {len(diff)} of {a.size} words differ, first at {diff[0].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fast", "split"])
def test_a_second_load_rebuilds_what_a_fresh_handle_builds(cuda, case):
    """load(seed 1), load(seed 2) on one handle: the derived set of seed 1 is dropped and rebuilt — the logits are a fresh handle's at
    seed 2, and not those of seed 1."""
    spec, precision, knobs, extra, sd1 = G.case_setup(case, seed=1)
    sd2 = G.case_setup(case, seed=2)[4]
    bits = []
    for loads in ((sd1, sd2), (sd2,), (sd1,)):
        e = G.make_engine(spec, precision, knobs, extra)
        try:
            for sd in loads:
                e.load_state_dict(sd)
            bits.append(G.logits_bits(e, spec))
        finally:
            e.close()
    for t in G.timesteps(spec):
        assert np.array_equal(bits[0][t], bits[1][t]), t
        assert not np.array_equal(bits[0][t], bits[2][t]), t
