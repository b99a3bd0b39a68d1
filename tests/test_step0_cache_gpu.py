"""The step-0 logits cache of the one-launch loop (fast engine): a layout that starts all-[MASK] reads the logits of its
first reverse step from a handle-owned table instead of running the denoiser pass (kernels_stack.hip, ldm_loop.cpp
run_loop_fused).  The table is written and read by the same kernel in register order, so the requirement is EQUALITY
with an engine whose cache is switched off (LDM_DEV=1 LDM_STEP0_CACHE=0): numpy.array_equal on the tokens after EVERY
step.  The bits of a draw come from the layout index, so layouts keep their positions in both runs.  The per-layout
flags of ldm_dev_step0_flags prove which layouts took the shortcut.

Shapes: B = 3 (one workgroup per layout), ten strided steps unless the case is about the schedule; synthetic weights."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, FIRST_LAYOUT, SEED, N_STEPS = 3, 5, 17, 10
SAMPLERS = ("random", "deterministic", "top_p")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _specs():
    from oracle import spec as SP

    return {"rico25": SP.RICO25, "publaynet": SP.PUBLAYNET,
            "rico25_s105": dataclasses.replace(SP.RICO25, name="rico25_e21", max_elem=21)}


def _engine(spec, cache_on, sd):
    from layout_dm_amd.binding import Engine

    kw = dict(n_category=spec.n_category, n_bin=spec.n_bin, max_elem=spec.max_elem, d_model=spec.d_model, n_head=spec.n_head,
              d_ff=spec.d_ff, n_layer=spec.n_layer, n_step=spec.n_step, precision="fast", max_batch=8)
    if cache_on:
        e = Engine(**kw)
    else:
        with _env(LDM_DEV="1", LDM_STEP0_CACHE="0"):
            e = Engine(**kw)
    e.load_state_dict(sd)
    d = e.describe()
    assert d["loop"] == "one_launch" and d["step0_cache"]["enabled"] == cache_on, d
    return e


@pytest.fixture(scope="module")
def engines():
    """key -> (spec, engine with the cache, engine without it), both on the same synthetic weights; built on first use."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from oracle import synth

    made = {}

    def get(key):
        if key not in made:
            spec = _specs()[key]
            sd = synth.synth_state_dict(spec, seed=0, perturb=True)
            made[key] = (spec, _engine(spec, True, sd), _engine(spec, False, sd))
        return made[key]

    yield get
    for _, on, off in made.values():
        on.close()
        off.close()


def _steps(spec, n=N_STEPS):
    from layout_dm_amd.diffusion import timestep_schedule

    return timestep_schedule(spec.n_step, n)


def _run(e, spec, start, sched, sampler="random", cond=None, first_layout=FIRST_LAYOUT, intermediates=True):
    """-> (tokens after every step (n, B, S) or None, final tokens (B, S), step-0 flags (B,))"""
    import torch

    cfg = {"name": sampler, "temperature": 1.0, "top_p": 0.9}
    tok = torch.from_numpy(np.ascontiguousarray(start)).int().to("cuda:0")
    out, inter = e.sample_loop(tok, sched[0], sched[1], cfg, cond=cond, seed=SEED, first_layout=first_layout,
                               intermediates=intermediates, use_graph=True)
    torch.cuda.synchronize()
    nb = start.shape[0]
    flags = e.step0_flags(nb) if e.describe()["step0_cache"]["enabled"] else np.zeros(nb, np.uint8)
    return (inter.cpu().numpy() if inter is not None else None), out.cpu().numpy(), flags


def _all_mask(spec, nb=B):
    return np.full((nb, spec.seq_len), spec.mask_id, np.int32)


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = np.argwhere(a != b)
    assert np.array_equal(a, b), f"{what}: {len(diff)} tokens differ, first at {diff[0].tolist()}"


@pytest.mark.parametrize("key", ["rico25", "publaynet", "rico25_s105"])
def test_all_mask_start_equals_the_uncached_engine(engines, key):
    spec, on, off = engines(key)
    # ten steps (the first at t = 0.9 T decides about a tenth of the tokens under the random samplers), and two steps: the
    # first at t = T / 2 decides about half of them from the cached logits
    scheds = [_steps(spec), _steps(spec, 2)]
    for sched in scheds:
        for sampler in SAMPLERS:
            a, fa, flags = _run(on, spec, _all_mask(spec), sched, sampler)
            b, fb, _ = _run(off, spec, _all_mask(spec), sched, sampler)
            _same(a, b, f"{key}/{sampler}")
            _same(fa, fb, f"{key}/{sampler} final")
            _same(fa, a[-1], f"{key}/{sampler} final against the last step")
            assert flags.tolist() == [1, 1, 1], (key, sampler, flags)
            if sampler == "random" and len(sched[0]) == 2:
                assert (a[0] != spec.mask_id).mean() > 0.25, "the first step decides too few tokens to show wrong logits"
    assert on.describe()["step0_cache"]["entries"] == [[sc[0][0], spec.seq_len] for sc in scheds]
    assert off.describe()["step0_cache"]["entries"] == []


def test_one_preset_token_keeps_its_layout_off_the_shortcut(engines):
    spec, on, off = engines("rico25")
    start = _all_mask(spec)
    start[1, 7] = int(spec.full_ids(7 % spec.n_attr)[3])   # a body class of position 7's attribute
    sched = _steps(spec)
    a, _, flags = _run(on, spec, start, sched)
    b, _, _ = _run(off, spec, start, sched)
    _same(a, b, "preset token")
    assert flags.tolist() == [1, 0, 1], flags


def test_cond_c_misses_and_an_all_false_mask_hits(engines):
    from oracle import synth

    spec, on, off = engines("rico25")
    sched = _steps(spec)
    c = synth.synth_cond_c(spec, B, seed=4)
    cond = {"seq": c["seq"], "mask": c["mask"], "type": "c"}
    a, _, flags = _run(on, spec, c["seq"].astype(np.int32), sched, cond=cond)
    b, _, _ = _run(off, spec, c["seq"].astype(np.int32), sched, cond=cond)
    _same(a, b, "cond=c")
    assert flags.tolist() == [0, 0, 0], flags   # (every layout carries at least one known category token)
    # a cond dict that conditions nothing: the overrides act in the step's tail only, the layouts are all-[MASK]
    free = {"seq": _all_mask(spec).astype(np.int64), "mask": np.zeros((B, spec.seq_len), bool), "type": "c"}
    a, _, flags = _run(on, spec, _all_mask(spec), sched, cond=free)
    b, _, _ = _run(off, spec, _all_mask(spec), sched, cond=free)
    _same(a, b, "all-false mask")
    assert flags.tolist() == [1, 1, 1], flags


def test_two_schedules_back_to_back(engines):
    from oracle import synth

    spec = _specs()["rico25"]
    _, _, off = engines("rico25")
    on = _engine(spec, True, synth.synth_state_dict(spec, seed=0, perturb=True))   # (its own engine: the entry list is the subject)
    try:
        full, strided = _steps(spec, 100), _steps(spec, 25)
        assert full[0][0] != strided[0][0]
        for sched in (full, strided, full):
            a, _, flags = _run(on, spec, _all_mask(spec), sched)
            b, _, _ = _run(off, spec, _all_mask(spec), sched)
            _same(a, b, f"schedule of {len(sched[0])} steps")
            assert flags.tolist() == [1, 1, 1], flags
        assert on.describe()["step0_cache"]["entries"] == [[full[0][0], spec.seq_len], [strided[0][0], spec.seq_len]]
    finally:
        on.close()


def test_weight_reload_drops_the_entries(engines):
    """A stale table would be seen: the tokens of the reloaded engine equal an uncached engine on the NEW weights and differ
    from what the old weights gave."""
    from oracle import synth

    spec = _specs()["rico25"]
    # two steps, the first at t = T / 2: about half of the tokens are decided by the first step's logits (at t close to T,
    # and always under greedy decoding, nearly every token stays [MASK] whatever the logits say)
    sched = _steps(spec, 2)
    sd_a = synth.synth_state_dict(spec, seed=3, perturb=False)
    sd_b = synth.synth_state_dict(spec, seed=3, perturb=True)
    on = _engine(spec, True, sd_a)
    off = _engine(spec, False, sd_b)
    try:
        before, _, flags = _run(on, spec, _all_mask(spec), sched, "random")
        assert flags.tolist() == [1, 1, 1] and len(on.describe()["step0_cache"]["entries"]) == 1
        on.load_state_dict(sd_b)
        assert on.describe()["step0_cache"]["entries"] == []
        after, _, flags = _run(on, spec, _all_mask(spec), sched, "random")
        ref, _, _ = _run(off, spec, _all_mask(spec), sched, "random")
        _same(after, ref, "reloaded weights")
        assert flags.tolist() == [1, 1, 1] and len(on.describe()["step0_cache"]["entries"]) == 1
        assert not np.array_equal(before[0], after[0]), "the two checkpoints give the same first step: the case proves nothing"
    finally:
        on.close()
        off.close()


def test_single_step_and_a_call_longer_than_one_launch(engines):
    spec, on, off = engines("rico25")
    one = _steps(spec, 100)
    one = (one[0][:1], one[1][:1])   # step 0 is also the last: tokens_out is written behind the shortcut
    a, fa, flags = _run(on, spec, _all_mask(spec), one)
    b, fb, _ = _run(off, spec, _all_mask(spec), one)
    _same(a, b, "one step")
    _same(fa, fb, "one step, final")
    _same(fa, a[0], "one step, final against the step")
    assert flags.tolist() == [1, 1, 1], flags
    # 130 steps = two launch segments (128 + 2); the second one starts from sampled tokens and must not hit
    t = [int(x) for x in np.linspace(spec.n_step - 1, 0, 130)]
    a, _, flags = _run(on, spec, _all_mask(spec, 1), (t, t))
    b, _, _ = _run(off, spec, _all_mask(spec, 1), (t, t))
    assert a.shape[0] == 130
    _same(a, b, "130 steps")
    assert flags.tolist() == [1], flags


def test_first_layout_offset_and_no_intermediates(engines):
    spec, on, off = engines("publaynet")
    sched = _steps(spec)
    a, fa, flags = _run(on, spec, _all_mask(spec), sched, first_layout=1000)
    b, fb, _ = _run(off, spec, _all_mask(spec), sched, first_layout=1000)
    _same(a, b, "first_layout = 1000")
    assert flags.tolist() == [1, 1, 1], flags
    base, _, _ = _run(on, spec, _all_mask(spec), sched)
    assert not np.array_equal(a, base), "the layout offset does not reach the draws"
    _, fc, flags = _run(on, spec, _all_mask(spec), sched, first_layout=1000, intermediates=False)
    _same(fc, fb, "without intermediates")
    assert flags.tolist() == [1, 1, 1], flags


def test_near_tie_flags_of_a_deterministic_call(engines):
    spec, on, off = engines("rico25")
    sched = _steps(spec)
    got = []
    for e in (on, off):
        e.set_tie_report(0.05, 0.0)
        try:
            inter, _, _ = _run(e, spec, _all_mask(spec), sched, "deterministic")
            got.append((inter, e.tie_flags(N_STEPS, B).cpu().numpy()))
        finally:
            e.set_tie_report(0.0, 0.0)
    _same(got[0][0], got[1][0], "deterministic tokens")
    print("near-tie flags set:", int(got[0][1].sum()), "of", got[0][1].size)
    assert np.array_equal(got[0][1], got[1][1])
    assert got[1][1].any(), "no near-tie flag at this threshold: the case compares two empty reports"
