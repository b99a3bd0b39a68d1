"""CPU: the inputs of tests/test_relation_kernel_gpu.py pinned without a device (tests/_relation_cases.py) —

  * the NumPy float64 restatement of the logit adjustment equals oracle.restatement.relation_update (autograd) run in float64 on every case,
    to 1e-12 of each row's path length, and the reference-produced tests/golden/rico25_relation.npz within that file's float32 bound (1e-5 of the largest update);
  * every value case holds a float64 margin of 1e-4 on its hinge arguments, at the seed the search returns; the one-edge cases have exactly
    the hinges active that their names say, the inactive ones none;
  * edge counts and geometries are what the issue's table says;
  * the bars (4 x the worst row of the float32 emulation — the larger of its two evaluations, the analytic restatement and the autograd oracle,
    which differ from each other by up to 14 x on a case: one-eq-pair-lo-on 4.2e-5 | 3.1e-6 — nothing from a device) are pinned: 0 exactly where nothing moves, and between
    4e-7 and 1e-3 of a row's path length elsewhere — the printed table is profiles/relation_alone_check.txt."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import _relation_cases as RC
from oracle import restatement as R
from oracle import spec as SP

CASES = RC.cases()
IDS = [c.id for c in CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_f64(case, start=None):
    spec = dataclasses.replace(SP.RICO25, name=case.id, n_category=case.n_category, n_bin=case.NB, max_elem=case.E)
    assert spec.pad_id == case.pad_id
    x = torch.from_numpy(np.array(RC.logp(case) if start is None else start, dtype=np.float64))
    g = RC.oracle_graph(case)
    # (lr scaled so that the oracle's mean over its B graphs is the case's step: n_graph may differ from B)
    lr = case.lr * case.B / case.graphs
    return R.relation_update(spec, x, RC.cond_seq(case).astype(np.int64), g, RC.centres(case.NB), RC.canvas_bins(case.NB), lr, case.num_update, 40).numpy()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float64_restatement_equals_the_autograd_oracle(case):
    ref = RC.reference(case)
    want = oracle_f64(case)
    err, where = RC.row_error(case, want, ref)
    m = RC.body_mask(case)
    print(f"{case.id:30s} worst row {err:.2e} at {where}")
    assert err <= 1e-12
    assert np.array_equal(want[~m], ref.out[~m]) and np.array_equal(ref.out[~m], RC.logp(case).astype(np.float64)[~m])
    still = ref.path == 0                                            # rows that never move: equal to the input in both
    for b, e, x in zip(*np.nonzero(still)):
        c0 = case.n_category + x * case.NB
        assert np.array_equal(want[b, c0:c0 + case.NB, e * RC.A + 1 + x], ref.out[b, c0:c0 + case.NB, e * RC.A + 1 + x])


def test_float64_restatement_equals_the_reference_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "rico25_relation.npz"))
    seq, batch, ei = g["cond_seq"].astype(np.int64), g["batch"], g["edge_index"]
    B = seq.shape[0]
    first = np.concatenate([[0], np.cumsum(np.bincount(batch, minlength=B))])
    cats = tuple(tuple(int(c) if c != SP.RICO25.pad_id else -1 for c in seq[b, ::RC.A]) for b in range(B))
    edges = tuple(tuple((int(s - first[b]), int(d - first[b]), int(a)) for s, d, a in zip(ei[0], ei[1], g["edge_attr"]) if batch[s] == b) for b in range(B))
    case = RC.Case("golden", "golden", 25, 32, cats, edges, float(g["lr"]), int(g["num_update"]), 0)
    assert np.allclose(g["centres"], RC.centres(32), rtol=0, atol=1e-15) and list(g["canvas_bins"]) == RC.canvas_bins(32)
    assert np.array_equal(RC.cond_seq(case)[:, ::RC.A], seq[:, ::RC.A])
    out = RC.run(case, np.float64, start=g["logp_in"])
    ref = g["logp_out_t50"].astype(np.float64)
    # The file is float32 output of steps up to O(1e4) that cancel back to O(1): its own rounding is ulp(1e4) ~ 1e-3 absolute.  The bound that
    # holds a float32 result of this file is tests/test_hip_parity.py _rel_close: 1e-5 of the largest update.  (The pointwise 5e-6 max(|ref|, 1)
    # of tests/test_oracle_golden.py holds between two float32 runs of the same operations; against float64 17 of 38 750 entries exceed it, the
    # worst by 3.9e-4 at a value of -0.55 — as far as the float32 emulation here is from the file, 2.6e-4.)
    scale = max(1.0, float(np.abs(ref - g["logp_in"]).max()))
    worst = float(np.abs(out.out - ref).max())
    print(f"golden: max |float64 - file| {worst:.2e}, largest update {scale:.2e}, ratio {worst / scale:.2e}")
    assert worst <= 1e-5 * scale
    assert np.array_equal(RC.run(case, np.float64, start=g["logp_in"].astype(np.float64)).out[~RC.body_mask(case)], g["logp_out_t50"][~RC.body_mask(case)])
    assert (out.out != g["logp_in"]).any()


@pytest.mark.parametrize("cid", list(RC.MAKERS), ids=list(RC.MAKERS))
def test_the_committed_seed_is_the_first_that_holds_the_margin(cid):
    assert RC.first_seed(RC.MAKERS[cid]) == RC.SEEDS[cid]
    c = RC.case(cid)
    r = RC.reference(c)
    print(f"{cid:30s} seed {c.seed:3d} margin {r.margin:.2e} active in the first iteration: {r.active0}")
    if c.family == "zero argument":      # the tie: the argument is the eps of less() exactly, or exactly 0 under less_equal()
        z, on, _, _ = RC.hinges(r.boxes[0][0], np.array([1]), np.array([2]), np.array([c.edges[0][0][2]]), np.float64)
        z4 = RC.hinges(RC.emulation(c).boxes[0][0], np.array([1]), np.array([2]), np.array([c.edges[0][0][2]]), np.float32)[0]
        tie = np.abs(z[on]) <= 1e-8
        assert tie.sum() == 1 and np.array_equal(z4[on][tie], z[on][tie].astype(np.float32)) and (np.abs(z[on][~tie]) >= RC.MARGIN).all()
        assert c.num_update == 1 and RC.emulation(c).active0 == c.want_active
    else:
        assert r.margin >= RC.MARGIN
    if c.want_active is not None:
        assert r.active0 == c.want_active
        assert (r.path > 0).any() == bool(c.want_active)


def test_one_edge_cases_cover_the_14_costs_and_every_hinge_on_both_sides():
    zero = [c for c in CASES if c.family == "zero argument"]
    assert {t for c in zero for t in c.want_active} == {"c_1", "c_2", "ov_1", "ov_2"} and sum(1 for c in zero if not c.want_active) == 4
    one = [c for c in CASES if c.family == "one edge"]
    assert all(c.B == 1 and c.n_edges == [1] for c in one)
    on = set().union(*(c.want_active for c in one))
    assert on == set(RC.TERMS)
    # inactive: the edge carries the term's attribute, the cost applies, and nothing is active
    applies = set()
    for c in one:
        if not c.want_active:
            r = RC.reference(c)
            ed = np.asarray(c.edges[0]).reshape(-1, 3)
            _, cond, _, _ = RC.hinges(r.boxes[0][0], ed[:, 0], ed[:, 1], ed[:, 2], np.float64)
            applies |= {RC.TERMS[t] for t in range(16) if cond[t].any()}
    assert applies == set(RC.TERMS)
    # each of the 14 costs: 3 sizes x {canvas, pair}, 3 canvas locations, 5 pair locations
    costs = set()
    for c in one:
        if c.want_active:
            s, d, a = c.edges[0][0]
            for v in (RC.SM, RC.EQ, RC.LG, RC.LEFT, RC.TOP, RC.RIGHT, RC.BOTTOM, RC.CENTER):
                if a & (1 << v):
                    costs.add((v, s == 0))
    assert len(costs) == 6 + 3 + 5 and {(RC.LEFT, True), (RC.RIGHT, True)}.isdisjoint(costs)
    assert sum(1 for c in one if c.edges[0][0][1] == 0) >= 6         # the canvas as dst


def test_geometries_and_edge_counts_are_what_the_table_says():
    by = {c.id: c for c in CASES}
    assert {(c.E, c.NB) for c in CASES if c.family == "geometry"} == {(1, 32), (3, 8), (5, 16), (7, 17), (25, 32), (30, 32), (32, 32), (32, 31)}
    assert all(c.B <= 4 for c in CASES)
    assert by["geo-E25-NB32-wideC"].C > 25 + 4 * 32 + 2 and by["geo-E25-NB32-lambda3e6"].lr == 3e6
    assert len(RC.nodes_of(by["map-no-element"], 1)) == 0 and by["map-no-element"].n_edges[1] == 0
    assert all(s == 0 for s, d, a in by["map-canvas-edges-only"].edges[0])
    c = by["map-node-without-edge"]
    touched = {n for s, d, a in c.edges[0] for n in (s, d)}
    assert set(range(1, len(RC.nodes_of(c, 0)) + 1)) - touched == {2} and (RC.reference(c).path[0, RC.nodes_of(c, 0)[1]] == 0).all()
    c = by["map-pad-between-nodes"]
    assert all(list(RC.nodes_of(c, b)) != list(range(len(RC.nodes_of(c, b)))) for b in range(c.B))
    assert all(len(RC.nodes_of(by["map-all-32-nodes"], b)) == 32 for b in range(2))
    assert by["edges-none"].n_edges == [0, 0] and by["edges-one"].n_edges == [1, 0]
    c = by["edges-duplicates"]
    assert len(set(c.edges[0])) < len(c.edges[0]) and len(set(c.edges[1])) * 2 == len(c.edges[1])
    assert any(d == 0 for s, d, a in by["edges-canvas-as-dst"].edges[0])
    c = by["edges-star-63"]
    assert sum(1 for s, d, a in c.edges[0] if 1 in (s, d)) > 60
    assert [by[k].n_edges for k in ("edges-512", "edges-513", "edges-528", "edges-528-as-512+16", "edges-1056")] == [[512], [513], [528], [512, 16], [1056]]
    full = by["edges-528"]
    assert len({(s, d) for s, d, a in full.edges[0]}) == 33 * 32 // 2 and full.E == 32
    share = np.mean([a != RC.UNKNOWN for s, d, a in full.edges[0]])
    assert 0.1 < share < 0.3
    sp = by["edges-528-as-512+16"]
    assert sp.edges[0] + sp.edges[1] == full.edges[0] and sp.lr / sp.B == full.lr / full.B
    assert by["edges-512"].edges[0] == full.edges[0][:512] and by["edges-1056"].edges[0] == full.edges[0] * 2
    d = RC.edge_513_with_dead_last()
    assert d.edges[0][:512] == by["edges-512"].edges[0] and d.edges[0][512][2] == RC.UNKNOWN and d.seed == by["edges-512"].seed
    assert {by[f"iter-{n}"].num_update for n in (1, 2, 4)} == {1, 2, 4} and RC.noop_case().num_update == 0
    # moderate steps: the largest update of a value case is O(10) .. O(1e3), except at the reference's default lambda
    for c in CASES:
        big = RC.reference(c).path.max()
        assert big == 0 or 1.0 < big < 2e3 or c.id == "geo-E25-NB32-lambda3e6", (c.id, big)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bars_are_pinned(case):
    ref, emu = RC.reference(case), RC.emulation(case)
    where = RC.row_error(case, emu.out)[1]
    err, err_autograd = RC.emulation_errors(case)
    bar = RC.bar(case)
    assert bar == 4.0 * max(err, err_autograd)
    m = RC.body_mask(case)
    moving = ref.path[ref.path > 0]
    print(f"{case.id:30s} B {case.B} E {case.E:2d} NB {case.NB:2d} edges {str(case.n_edges):16s} emulation {err:.2e} at {where} | autograd {err_autograd:.2e}  bar {bar:.2e}  "
          f"path lengths {moving.min() if moving.size else 0:.1e} .. {moving.max() if moving.size else 0:.1e}  margin {ref.margin:.1e}")
    assert np.array_equal(emu.out[~m], RC.logp(case)[~m])
    assert np.array_equal((emu.path > 0), (ref.path > 0))          # the same rows move in both
    if not moving.size:
        assert bar == 0 and np.array_equal(emu.out, RC.logp(case))
    else:
        assert 4e-7 <= bar <= 1e-3, bar          # no better than float32's own rounding of a row, no looser than 1e-3 of its path
    st = RC.still_mask(case)
    assert np.array_equal(emu.out[st], RC.logp(case)[st])


def test_the_windows_case_holds_its_margin():
    c = RC.windows_case()
    assert c.B == 6 and RC.first_seed(RC._windows) == RC.WINDOWS_SEED and RC.reference(c).margin >= RC.MARGIN and 4e-7 <= RC.bar(c) <= 1e-3
    assert np.abs(oracle_f64(c) - RC.reference(c).out).max() <= 1e-12 * RC.reference(c).path.max()


def test_the_library_exports_the_hook():
    """A development hook (csrc/ldm_dev.cpp), like ldm_dev_gemm_run outside include/ldm_hip.h and binding.EXPORTS: the GPU test declares it itself"""
    import ctypes

    from layout_dm_amd import build

    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "ldm_dev_relation_run")
    lib.ldm_dev_relation_run.argtypes, lib.ldm_dev_relation_run.restype = [ctypes.c_void_p], ctypes.c_int
    assert lib.ldm_dev_relation_run(None) == -1       # (a null io is refused before anything touches a device)
