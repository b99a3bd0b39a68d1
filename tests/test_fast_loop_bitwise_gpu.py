"""The fast mode's stack kernels against tests/golden/fast_loop_bitwise/parent.npz — what the SAME cases computed at the
commit before the FFN ring of the stack kernel went to the interleaved LDS map with double iterations
(tools/make_fast_loop_bitwise_golden.py records and documents the cases).  That change and the ones riding with it
reorder no floating-point operation, so the requirement is EQUALITY: the tokens after every one of ten reverse steps
(random / deterministic / top_p, unconditional and cond = c; Rico25 and PubLayNet at S = 125, Rico25 at S = 105) and the
bit pattern of the single-pass logits at two timesteps.  Ten steps x four layers enter the ring with both parities of
the double iteration and run the odd single iteration behind them; B = 3 is one workgroup per layout."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "fast_loop_bitwise", "parent.npz")


@pytest.fixture(scope="module")
def recorded():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import make_fast_loop_bitwise_golden as G

    return G, G.record("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_covers_the_cases(recorded, golden):
    G, got = recorded
    assert set(got) == set(golden)
    assert len(got) == 3 * (len(G.SAMPLERS) * 2 + 2 * len(G.LOGIT_T))


@pytest.mark.parametrize("key", ["rico25", "publaynet", "rico25_s105"])
@pytest.mark.parametrize("cond", ["uncond", "cond_c"])
def test_tokens_of_every_step_bit_identical(recorded, golden, key, cond):
    G, got = recorded
    for sampler in G.SAMPLERS:
        name = f"{key}/{sampler}/{cond}"
        a, b = got[name], golden[name]
        assert a.shape == b.shape and a.shape[0] == G.N_STEPS and a.shape[1] == G.B, (name, a.shape, b.shape)
        diff = np.argwhere(a != b)
        assert diff.size == 0, f"{name}: {len(diff)} tokens differ, first at (step, layout, position) {diff[0].tolist()}"


@pytest.mark.parametrize("key", ["rico25", "publaynet", "rico25_s105"])
def test_single_pass_logits_bit_identical(recorded, golden, key):
    G, got = recorded
    for t in G.LOGIT_T:
        a, b = got[f"{key}/logits_t{t}/every{G.LOGIT_STRIDE}"], golden[f"{key}/logits_t{t}/every{G.LOGIT_STRIDE}"]
        assert a.dtype == np.uint32 and a.shape == b.shape
        diff = np.argwhere(a != b)
        assert diff.size == 0, f"{key} t={t}: {len(diff)} sampled logit words differ, first at {diff[0].tolist()}"
        assert bytes(got[f"{key}/logits_t{t}/sha256"]) == bytes(golden[f"{key}/logits_t{t}/sha256"]), f"{key} t={t}: logits bit pattern"
