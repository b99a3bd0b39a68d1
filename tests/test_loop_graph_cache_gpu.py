"""The per-lane hipGraph loop of ldm_sample_loop (layout_dm_amd/csrc/ldm_loop.cpp) and the handle's cache of captured loops
(ldm_handle.h GraphCache), through Engine.graph_cache(): entries held now and keys captured since create.

  * ragged and balanced cuts (ldm_loop_plan.h cut_call) through the graphs: at max_batch 16, chunk 8 — two lanes — B = 16 (8 + 8),
    13 (the balanced 7 + 6), 8 and 3 (one lane) give the tokens and intermediates of the loop without graphs;
  * hit, miss and eviction at 8 entries, counted — a loop that silently re-captured on every call would pass every token check;
  * cond tensors that move between calls replay ONE captured loop;
  * growth of the relation edge staging drops the graphs that recorded the old address, and only those.

Geometry: test_launch_sequence_gpu.py's SMALL (the per-step path in exact and in fast, where it takes the generic16 structure); the
relation case names its own.  Synthetic weights, all-[MASK] starts, a handful of steps."""
import dataclasses

import numpy as np
import pytest
import torch

import test_hip_parity as HP
from oracle import synth
from test_launch_sequence_gpu import REFERENCE, SMALL

pytestmark = pytest.mark.gpu

GREEDY = {"name": "deterministic"}
RANDOM = {"name": "random", "temperature": 1.0}


def _engine(spec, precision, max_batch, chunk=0):
    from layout_dm_amd.binding import Engine

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    e = Engine(n_category=spec.n_category, n_bin=spec.n_bin, max_elem=spec.max_elem, d_model=spec.d_model, n_head=spec.n_head,
               d_ff=spec.d_ff, n_layer=spec.n_layer, n_step=spec.n_step, precision=precision, max_batch=max_batch, chunk=chunk)
    e.load_state_dict(synth.synth_state_dict(spec, seed=1, perturb=True))
    return e


def _steps(spec, n):
    """n timesteps from T - 1 down to 0 ([0] for n = 1): another n is another graph key, and the last step leaves no [MASK]"""
    return [(n - 1 - k) * (spec.n_step - 1) // max(n - 1, 1) for k in range(n)]


def _loop(e, spec, B, ts, cfg, use_graph, seed=3, intermediates=False, start=None, **kw):
    tok = torch.full((B, spec.seq_len), spec.mask_id, dtype=torch.int32, device=e.device) if start is None else e._tok(start).clone()
    out, inter = e.sample_loop(tok, ts, ts, cfg, seed=seed, intermediates=intermediates, use_graph=use_graph, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (inter.cpu().numpy() if inter is not None else None)


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_ragged_and_balanced_cuts_replay_the_tokens_of_the_loop_without_graphs(precision):
    e = _engine(SMALL, precision, max_batch=16, chunk=8)
    try:
        assert (e.chunk, e.lanes) == (8, 2)
        ts = _steps(SMALL, 5)
        for B in (16, 13, 8, 3):
            for cfg in (GREEDY, RANDOM):
                before = e.graph_cache()[1]
                graph, graph_inter = _loop(e, SMALL, B, ts, cfg, True, intermediates=True)
                assert e.graph_cache()[1] == before + 1, (B, cfg["name"])          # the graphs ran: this key was captured
                eager, eager_inter = _loop(e, SMALL, B, ts, cfg, False, intermediates=True)
                assert np.array_equal(graph, eager) and np.array_equal(graph_inter, eager_inter), (B, cfg["name"])
                assert np.array_equal(graph_inter[-1], graph) and (graph != SMALL.mask_id).all(), (B, cfg["name"])
    finally:
        e.close()


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_hit_miss_and_eviction_are_counted(precision):
    """Nine keys (loops of 1..9 steps, 5 on average, at B = 8) through a cache of 8."""
    e = _engine(SMALL, precision, max_batch=16, chunk=8)
    try:
        assert e.graph_cache() == (0, 0)
        first = {}
        for n in range(1, 10):
            first[n] = _loop(e, SMALL, 8, _steps(SMALL, n), RANDOM, True)[0]
            assert e.graph_cache() == (min(n, 8), n)
        assert e.graph_cache() == (8, 9)
        again = _loop(e, SMALL, 8, _steps(SMALL, 9), RANDOM, True)[0]             # a hit: nothing captured
        assert e.graph_cache() == (8, 9) and np.array_equal(again, first[9])
        evicted = _loop(e, SMALL, 8, _steps(SMALL, 1), RANDOM, True)[0]           # the oldest key went when the ninth came
        assert e.graph_cache() == (8, 10)
        assert np.array_equal(evicted, _loop(e, SMALL, 8, _steps(SMALL, 1), RANDOM, False)[0]) and np.array_equal(evicted, first[1])
        assert e.graph_cache() == (8, 10)                                           # (the loop without graphs touches no cache)
        e.set_tie_report(1e-3)                                                      # new thresholds: every captured loop goes
        assert e.graph_cache() == (0, 10)
        _loop(e, SMALL, 8, _steps(SMALL, 2), GREEDY, True)
        assert e.graph_cache() == (1, 11)
        e.load_state_dict(synth.synth_state_dict(SMALL, seed=1, perturb=True))      # ... and with every (re)load of the weights
        assert e.graph_cache() == (0, 11)
    finally:
        e.close()


def test_moving_cond_tensors_replay_one_captured_loop():
    """The three-seed cond=c sequence of test_hip_parity.py test_loop_time_difference_and_cond_graph_reuse, counted."""
    e = _engine(SMALL, "exact", max_batch=16, chunk=8)
    try:
        ts = _steps(SMALL, 5)
        before = e.graph_cache()[1]
        outs = []
        for seed in (0, 1, 2):
            c = synth.synth_cond_c(SMALL, 4, seed=seed)
            cond = {"seq": torch.from_numpy(c["seq"]), "mask": torch.from_numpy(c["mask"]), "type": "c"}
            junk = torch.empty(1000 * (seed + 1), device="cuda")  # perturb the allocator between calls
            got = _loop(e, SMALL, 4, ts, GREEDY, True, cond=cond)[0]
            want = _loop(e, SMALL, 4, ts, GREEDY, False, cond=cond)[0]
            del junk
            assert np.array_equal(got, want), seed
            assert (got[c["mask"]] == c["seq"][c["mask"]]).all(), seed
            outs.append(got)
        assert e.graph_cache() == (1, before + 1)
        assert not np.array_equal(outs[0], outs[1])
    finally:
        e.close()


def _complete_graph(spec, B, gen):
    """HP._random_graph's format with every layout full (max_elem elements) and every pair of its nodes an edge."""
    n = spec.max_elem
    ys, eis, eas, bts, seqs = [], [], [], [], []
    for b in range(B):
        lab = torch.randint(0, spec.n_category, (n,), generator=gen)
        ys.append(torch.cat([torch.zeros(1, dtype=torch.long), lab + 1]))
        i, j = torch.triu_indices(n + 1, n + 1, offset=1)
        eis.append(torch.stack([i, j]) + b * (n + 1))
        eas.append((1 << torch.randint(0, 4, i.shape, generator=gen)) | (1 << torch.randint(4, 10, i.shape, generator=gen)))
        bts.append(torch.full((n + 1,), b, dtype=torch.long))
        seq = torch.full((spec.seq_len,), spec.mask_id, dtype=torch.long)
        seq[0::spec.n_attr] = lab
        seqs.append(seq)
    return {"y": torch.cat(ys), "edge_index": torch.cat(eis, dim=1), "edge_attr": torch.cat(eas), "batch": torch.cat(bts)}, torch.stack(seqs)


def test_relation_edge_growth_drops_the_graphs_of_the_old_staging():
    """Call A (at most 66 edges per layout, under the initial 1024-edge staging), call B (complete graphs: 325 edges per layout, 2600
    in all — the staging grows and moves), call A again.  B's hyper-parameters differ from A's: the staging holds the edges, the key
    only their address, so a B with A's scalars would be A's key at the new address."""
    spec = dataclasses.replace(REFERENCE, n_layer=1)
    e = _engine(spec, "exact", max_batch=8)
    try:
        B, ts = 8, [90, 50, 10]      # t >= 10: every step is an adjusted one (logit_adjustment.py:107)
        gen = torch.Generator().manual_seed(29)
        centres = np.stack([np.linspace(0, 1 - 1 / 32, 32), np.linspace(0, 1 - 1 / 32, 32), np.linspace(1 / 32, 1, 32), np.linspace(1 / 32, 1, 32)])
        calls = {}
        for name, (graph, seq), lam in (("A", HP._random_graph(spec, B, gen), 2e4), ("B", _complete_graph(spec, B, gen), 1e4)):
            n_edges = torch.bincount(graph["batch"][graph["edge_index"][0]], minlength=B)
            assert int(n_edges.max()) <= (100 if name == "A" else 512) and (name == "A") == (int(n_edges.sum()) <= 1024)
            calls[name] = (seq, {"seq": seq, "mask": seq != spec.mask_id, "type": "relation"},
                           e.make_relation(graph, centres, [16, 16, 31, 31], lam, 2, B))

        def run(name, use_graph):
            seq, cond, rel = calls[name]
            return _loop(e, spec, B, ts, RANDOM, use_graph, start=seq, cond=cond, relation=rel)[0]

        want = {name: run(name, False) for name in calls}
        assert e.graph_cache() == (0, 0) and not np.array_equal(want["A"], want["B"])
        for name, cache in (("A", (1, 1)), ("B", (1, 2)), ("A", (2, 3))):   # after B the entry captured for A is gone; the second A captures again
            assert np.array_equal(run(name, True), want[name]), name
            assert e.graph_cache() == cache, name
    finally:
        e.close()
