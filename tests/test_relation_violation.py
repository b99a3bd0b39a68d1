"""Relation violation score (compute_violation, trainer/helpers/metric.py:62-95; detect_size_relation / detect_loc_relation,
trainer/data/util.py:33-69) — CPU side.

The host build of the kernel's one source (csrc/ldm_relation_detect_core.h, through tests/cpu_relation_detect_check.cpp)
against tests/golden/relation_violation/reference.npz, which tools/make_relation_violation_golden.py writes from the reference's own
functions: every per-edge size code, loc code, `failure` and `valid` and every per-layout score BIT FOR BIT, float32 and
float64, NaN compared by position.  No tolerance: the counts are small integers and a score is one correctly rounded float32
division.  Also: the hand-made boundary inputs are reproducible without the reference and hit what they aim at, the fixture
regenerates bit for bit where the reference is importable, and the C-ABI exports the two entry points and refuses bad
arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import _hostbuild as HB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("make_relation_violation_golden",
                                                  os.path.join(ROOT, "tools", "make_relation_violation_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()
CASES = [(s, p) for s in G.SETS for p in G.PRECISIONS]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "relation_violation", "reference.npz"))


@pytest.fixture(scope="module")
def host_exe():
    return HB.host_program("cpu_relation_detect_check")


def csr_of(y, edge_index, edge_attr, batch):
    from layout_dm_amd.relation import graph_to_csr

    data = {"y": torch.from_numpy(y), "edge_index": torch.from_numpy(edge_index), "edge_attr": torch.from_numpy(edge_attr),
            "batch": torch.from_numpy(batch)}
    n_graph = int(batch.max()) + 1
    off, src, dst, attr, first, order = graph_to_csr(data, n_graph, with_nodes=True)
    return n_graph, off.numpy(), src.numpy(), dst.numpy(), attr.numpy(), first.numpy(), order.numpy()


def host_run(exe, tmp_path, box, y, edge_index, edge_attr, batch):
    """-> (exit code, per-edge (E,4) int32 in edge_index's order, scores (n_graph,) float32)"""
    n_graph, off, src, dst, attr, first, order = csr_of(y, edge_index, edge_attr, batch)
    payload = np.array([box.dtype == np.float64, len(box), len(y), n_graph, len(attr)], np.int32).tobytes()
    for a, dt in ((box, box.dtype), (y == 0, np.uint8), (off, np.int32), (src, np.int32), (dst, np.int32), (attr, np.int32),
                  (first, np.int64)):
        payload += np.ascontiguousarray(a, dt).tobytes()
    rc, raw = HB.run_host_io(exe, tmp_path, payload)
    raw = np.frombuffer(raw, np.uint8)
    E = len(attr)
    edge_csr = raw[:16 * E].view(np.int32).reshape(E, 4)
    edge = np.empty_like(edge_csr)
    edge[order] = edge_csr
    return rc, edge, raw[16 * E:].view(np.float32)


def assert_same_scores(got, want, what):
    """bit for bit on every layout; NaN by position"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", np.flatnonzero(np.isnan(got) != np.isnan(want))[:8])
    ok = ~np.isnan(want)
    bad = got[ok].view(np.uint32) != want[ok].view(np.uint32)
    assert not bad.any(), (what, np.flatnonzero(ok)[bad][:8], got[ok][bad][:8], want[ok][bad][:8])


@pytest.mark.parametrize("name,prec", CASES)
def test_host_build_equals_the_reference_bit_for_bit(host_exe, tmp_path, fx, name, prec):
    box, y, ei, ea, batch = G.load_inputs(fx)[name][prec]
    assert box.dtype == G.DTYPE[prec]
    rc, edge, score = host_run(host_exe, tmp_path, box, y, ei, ea, batch)
    assert rc == 0
    for col, key in enumerate(("size", "loc", "failure", "valid")):
        want = fx[f"{name}_{key}_{prec}"]
        assert want.shape == (ea.size,)
        bad = np.flatnonzero(edge[:, col] != want)
        assert bad.size == 0, (name, prec, key, bad[:8], edge[bad[:8], col], want[bad[:8]])
    assert_same_scores(score, fx[f"{name}_score_{prec}"], (name, prec))
    assert len(score) == int(batch.max()) + 1


def test_host_build_refuses_a_row_beyond_the_boxes(host_exe, tmp_path, fx):
    box, y, ei, ea, batch = G.load_inputs(fx)["edge"]["f32"]
    rc, _, _ = host_run(host_exe, tmp_path, box[:-1], y, ei, ea, batch)   # the last node has edges
    assert int(ei.max()) == len(box) - 1 and rc == 3


def test_host_build_under_address_and_undefined_sanitizers(tmp_path, fx):
    """every host-build case above on the ASan + UBSan build: boxes, canvas flags and the CSR arrays are exact-size allocations
    (the two `empty` sets write zero edges: nothing is handed to fwrite there)"""
    exe = HB.host_program("cpu_relation_detect_check", sanitize=True)
    for name, prec in CASES:
        test_host_build_equals_the_reference_bit_for_bit(exe, tmp_path, fx, name, prec)
    test_host_build_refuses_a_row_beyond_the_boxes(exe, tmp_path, fx)


def test_handmade_inputs_are_reproducible_and_hit_their_boundaries(fx):
    for p in G.PRECISIONS:
        T = G.DTYPE[p]
        box, y, ei, ea, batch = G.handmade(T)
        assert box.dtype == T and np.array_equal(box, fx[f"edge_box_{p}"])
        for k, v in (("y", y), ("edge_index", ei), ("edge_attr", ea), ("batch", batch)):
            assert np.array_equal(v, fx[f"edge_{k}"]), k
        size, loc = fx[f"edge_size_{p}"], fx[f"edge_loc_{p}"]
        assert set(size.tolist()) == {1, 2, 3} and set(loc.tolist()) == {5, 6, 7, 8, 9}
        # the size thresholds: node 1 is b1, nodes 2.. carry a2 = lo, lo-, lo+, hi, hi-, hi+, a1, a1-, a1+
        a1 = T(box[1, 2] * box[1, 3])
        lo, hi = T(T(1 - 0.1) * a1), T(T(1 + 0.1) * a1)
        assert box[2, 2] == lo and box[5, 2] == hi and box[3, 2] < lo < box[4, 2] and box[6, 2] < hi < box[7, 2]
        code = {int(d): int(size[e]) for e, (s, d) in enumerate(ei.T) if s == 1 and 2 <= d <= 10}
        assert [code[k] for k in range(2, 11)] == [1, 1, 2, 3, 2, 3, 2, 2, 2], (p, code)     # strict < on both sides
        # touching boxes count (<=), one ulp of overlap does not; a corner where TOP and LEFT both hold says TOP
        g1 = np.flatnonzero(batch == 1)
        b1 = g1[1]
        pairs = {(float(box[d, 0]), float(box[d, 1])): int(loc[e]) for e, (s, d) in enumerate(ei.T) if s == b1}
        up = float(np.nextafter(T(0.25), T(2)))
        assert pairs[(0.5, 0.25)] == 6 and pairs[(0.5, up)] == 9 and pairs[(0.25, 0.5)] == 5 and pairs[(up, 0.5)] == 9
        assert pairs[(0.5, 0.75)] == 8 and pairs[(0.75, 0.5)] == 7 and pairs[(0.25, 0.25)] == 6 and pairs[(0.25, 0.75)] == 8
        # canvas thirds: the rounded third itself is CENTER in float32 (it lies above 1/3), TOP one ulp below
        g2 = np.flatnonzero(batch == 2)
        third = {float(box[d, 1]): int(loc[e]) for e, (s, d) in enumerate(ei.T) if s == g2[0]}
        t32 = np.float32(1.0 / 3)
        assert third[float(T(t32))] == 9 and third[float(np.nextafter(T(t32), T(-1)))] == (6 if p == "f32" else 9)
        assert third[float(T(1.0 / 3))] == 9 and third[float(np.nextafter(T(1.0 / 3), T(-1)))] == 6
        assert third[float(T(np.float32(2.0 / 3)))] == 8 and third[float(np.nextafter(T(2.0 / 3), T(-1)))] == 9
    # a y == 0 node that is not its graph's first, a duplicated edge, every kind of edge_attr
    y, batch, ei, ea = fx["edge_y"], fx["edge_batch"], fx["edge_edge_index"], fx["edge_edge_attr"]
    firsts = np.flatnonzero(np.r_[True, batch[1:] != batch[:-1]])
    assert np.setdiff1d(np.flatnonzero(y == 0), firsts).size == 1
    trip = np.stack([ei[0], ei[1], ea]).T
    assert len(np.unique(trip, axis=0)) < len(trip)
    assert set(G.GTS) <= set(ea.tolist())
    v = fx["edge_valid_f32"]
    assert {0, 1, 2} == set(v.tolist()) and {0, 1, 2} == set(fx["edge_failure_f32"].tolist())


def test_fixture_is_not_an_equality_of_zeros(fx):
    for p in G.PRECISIONS:
        s = fx[f"big_score_{p}"]
        f = s[~np.isnan(s)]
        assert s.dtype == np.float32 and len(s) == 512 and fx["big_edge_attr"].size > 10000
        assert np.isnan(s).sum() >= 20 and (f == 0).sum() >= 20 and (f != 0).sum() >= 300 and len(np.unique(f)) >= 50
        assert np.isnan(fx[f"empty_score_{p}"]).all() and len(fx[f"empty_score_{p}"]) == 3
        assert np.isnan(fx[f"edge_score_{p}"]).sum() == 2


def test_fixture_regenerates_from_reference(fx):
    from oracle import ref_harness as rh

    if not rh.reference_importable():
        pytest.skip("neither the reference tree nor oracle/_ref/ present")
    out = G.compute(G.inputs())
    assert set(out) == set(fx.files)
    for k, v in out.items():
        v = np.asarray(v)
        assert v.dtype == fx[k].dtype and np.array_equal(v, fx[k], equal_nan=v.dtype.kind == "f"), k


def test_csr_with_nodes_keeps_the_default_form():
    from layout_dm_amd.relation import graph_to_csr

    data = {"y": torch.tensor([0, 1, 0, 2, 3]), "batch": torch.tensor([0, 0, 1, 1, 1]),
            "edge_index": torch.tensor([[2, 0, 4, 1], [3, 1, 2, 0]]), "edge_attr": torch.tensor([5, 6, 7, 8])}
    plain = graph_to_csr(data, 2)
    full = graph_to_csr(data, 2, with_nodes=True)
    assert len(plain) == 4 and len(full) == 6 and all(torch.equal(a, b) for a, b in zip(plain, full))
    off, src, dst, attr, first, order = full
    assert off.tolist() == [0, 2, 4] and src.tolist() == [0, 1, 0, 2] and dst.tolist() == [1, 0, 1, 0]
    assert attr.tolist() == [6, 8, 5, 7] and first.tolist() == [0, 2] and order.tolist() == [1, 3, 0, 2]


def test_cabi_exports_and_refuses_bad_arguments():
    from layout_dm_amd import binding, build

    names = ("ldm_relation_violation", "ldm_relation_violation_dense")
    for name in names:
        assert name in binding.EXPORTS
    assert binding.ABI_VERSION == 5
    lib = C.CDLL(build.build(verbose=False))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    graph = [vp, i64, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.ldm_relation_violation.argtypes = [vp, i32, i64] + graph
    lib.ldm_relation_violation_dense.argtypes = [vp, i32, vp, i32, i32, vp] + graph
    d = C.c_void_p(16)   # never dereferenced: every call below is refused before it touches memory or launches

    def flat(bbox=d, f64=0, n_rows=8, canvas=d, n_nodes=8, off=d, src=d, dst=d, attr=d, first=d, n_graph=2, n_edge=4, out=d,
             edge=None, err=d):
        return lib.ldm_relation_violation(bbox, f64, n_rows, canvas, n_nodes, off, src, dst, attr, first, n_graph, n_edge, out,
                                          edge, err, None)

    def dense(bbox=d, f64=0, mask=d, B=2, S=4, rows=d, canvas=d, n_nodes=8, off=d, src=d, dst=d, attr=d, first=d, n_graph=2,
              n_edge=4, out=d, edge=None, err=d):
        return lib.ldm_relation_violation_dense(bbox, f64, mask, B, S, rows, canvas, n_nodes, off, src, dst, attr, first, n_graph,
                                                n_edge, out, edge, err, None)

    for call in (flat, dense):
        for bad in ({"bbox": None}, {"canvas": None}, {"off": None}, {"src": None}, {"dst": None}, {"attr": None},
                    {"first": None}, {"out": None}, {"err": None}, {"f64": 2}, {"n_graph": 0}, {"n_graph": -3}, {"n_edge": -1},
                    {"n_nodes": -1}):
            assert call(**bad) == -1, (call.__name__, bad)
    assert flat(n_rows=-1) == -1
    for bad in ({"mask": None}, {"rows": None}, {"B": 0}, {"B": -2}, {"S": 0}, {"B": 1 << 20, "S": 1 << 12}):
        assert dense(**bad) == -1, bad


def test_python_api_and_no_silent_cpu_path(fx):
    from layout_dm_amd import metrics

    for name in ("compute_violation", "relation_violation", "relation_detect"):
        assert callable(getattr(metrics, name))
    box, y, ei, ea, batch = G.load_inputs(fx)["edge"]["f32"]
    data = {"y": torch.from_numpy(y), "edge_index": torch.from_numpy(ei), "edge_attr": torch.from_numpy(ea),
            "batch": torch.from_numpy(batch)}
    if torch.cuda.is_available():
        assert_same_scores(metrics.compute_violation(torch.from_numpy(box), data).cpu().numpy(), fx["edge_score_f32"], "edge")
    else:
        with pytest.raises(RuntimeError, match="no CPU path"):
            metrics.compute_violation(torch.from_numpy(box), data)


def test_dropin_is_installed_only_behind_the_class_swap_and_a_gpu(monkeypatch):
    """layout_dm_amd/reference_hooks.py, with stand-ins for the reference's two modules: nothing is touched without the class
    swap or without a device; with both, trainer.test.compute_violation hands on to metrics.compute_violation, keeps the
    original, is installed once, and goes back to the original whenever no device is there at call time."""
    import sys
    import types

    from layout_dm_amd import metrics, reference_hooks as H

    class Ours:
        pass

    def reference(bbox_flatten, data):
        return "reference"

    ref_layoutdm = types.SimpleNamespace(LayoutDM=object)
    ref_test = types.SimpleNamespace(compute_violation=reference)
    monkeypatch.setattr(metrics, "compute_violation", lambda bbox_flatten, data: "dropin")
    gpu = [False]
    monkeypatch.setattr(torch.cuda, "is_available", lambda: gpu[0])
    monkeypatch.delitem(sys.modules, "trainer.test", raising=False)
    monkeypatch.delitem(sys.modules, "trainer.models.layoutdm", raising=False)
    assert H.install_violation_dropin(Ours) is False                     # the reference is not even imported
    monkeypatch.setitem(sys.modules, "trainer.models.layoutdm", ref_layoutdm)
    monkeypatch.setitem(sys.modules, "trainer.test", ref_test)
    gpu[0] = True
    assert H.install_violation_dropin(Ours) is False and ref_test.compute_violation is reference      # no class swap
    ref_layoutdm.LayoutDM = Ours
    gpu[0] = False
    assert H.install_violation_dropin(Ours) is False and ref_test.compute_violation is reference      # no device
    gpu[0] = True
    assert H.install_violation_dropin(Ours) is True
    installed = ref_test.compute_violation
    assert installed is not reference and installed.reference is reference and installed(None, None) == "dropin"
    assert H.install_violation_dropin(Ours) is True and ref_test.compute_violation is installed       # once
    gpu[0] = False
    assert installed(None, None) == "reference"
