"""Max-IoU, DocSim and average IoU (trainer/helpers/metric.py:206-507; eval.py:173-176,211-215) — CPU side.

The host build of the kernels' one source (csrc/ldm_eval_iou_core.h, through tests/cpu_eval_iou_check.cpp) against
tests/golden/eval_iou/reference.npz, which tools/make_eval_iou_golden.py writes from the reference's own functions: IoU entries and
perceptual (BLT) entries bit for bit, pair / layout scores within rtol 1e-6 (float32) and 1e-12 (float64 and the mixed
float32 x float64 call).  Also: the fixture's inputs are reproducible from the generator's seed, the fixture regenerates
bit for bit where the reference is importable, and the C-ABI exports the three entry points and refuses bad arguments."""
import importlib.util
import os

import numpy as np
import pytest

import _hostbuild as HB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = {"f32": 1e-6, "f64": 1e-12, "mix": 1e-12}


def _gen():
    spec = importlib.util.spec_from_file_location("make_eval_iou_golden", os.path.join(ROOT, "tools", "make_eval_iou_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_iou", "reference.npz"))


def _sets(fx, name, prec, which):
    return G.cast(G.unflatten(fx[f"{name}_box"], fx[f"{name}_label"], fx[f"{name}_n"]), prec, which)


def _close(a, b, rtol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = ~(np.abs(a - b) <= rtol * np.abs(b) + 1e-300)
    assert not bad.any(), (what, np.flatnonzero(bad)[:4], a[bad][:4], b[bad][:4])


@pytest.fixture(scope="module")
def host_exe():
    return HB.host_program("cpu_eval_iou_check")


def _pack(layouts, S):
    f64 = any(b.dtype == np.float64 for b, _ in layouts)
    box = np.zeros((len(layouts), S, 4), np.float64 if f64 else np.float32)
    lab = np.zeros((len(layouts), S), np.int64)
    n = np.zeros(len(layouts), np.int32)
    for r, (b, l) in enumerate(layouts):
        box[r, :len(l)], lab[r, :len(l)], n[r] = b, l, len(l)
    return f64, box, lab, n


def _host(exe, tmp_path, mode, set1, set2=None, S=None):
    set2 = set1 if set2 is None else set2
    S = S or max(1, max(len(l) for _, l in set1 + set2))
    p1, p2 = _pack(set1, S), _pack(set2, S)
    payload = np.array([mode, p1[0], p2[0], len(set1), S], np.int32).tobytes()
    payload += b"".join(np.ascontiguousarray(a).tobytes() for p in (p1, p2) for a in p[1:])
    rc, raw = HB.run_host_io(exe, tmp_path, payload)
    return rc, np.frombuffer(raw, np.float64)


def _sorted(layout):
    b, l = layout
    o = np.argsort(l, kind="stable")
    return b[o], l[o]


def maxiou_pair_list(a, b):
    """the fixture's Max-IoU pairs in its order: groups by first appearance in a, set-2 index outer, set-1 inner"""
    keys, g1, g2 = G.group_keys(a, b)
    s1, s2 = [], []
    for k in keys:
        for j in g2[k]:
            for i in g1[k]:
                s1.append(_sorted(a[i]))
                s2.append(_sorted(b[j]))
    return s1, s2


def test_fixture_inputs_reproducible_from_seed(fx):
    inp = G.inputs()
    assert int(fx["seed"]) == G.SEED
    for name in G.SETS:
        box, lab, n = G.flatten(inp[name])
        assert np.array_equal(box, fx[f"{name}_box"]) and np.array_equal(lab, fx[f"{name}_label"]), name
        assert np.array_equal(n, fx[f"{name}_n"]), name
    # what the fixture promises to cover
    assert {1, 2, 3, 25} <= set(fx["mx_a_n"].tolist())
    d = np.abs(fx["ds_gt_n"].astype(int) - fx["ds_gen_n"].astype(int))
    assert {0, 2, 3} <= set(d.tolist()) and 0 in fx["avg_n"] and 1 in fx["avg_n"]
    assert fx["maxiou_group_size_f32"].max() >= 10 and float(fx["maxiou_nokey_f32"]) == 0.0


def test_fixture_regenerates_from_reference(fx):
    from oracle import ref_harness as rh

    if not rh.reference_available():
        pytest.skip("reference tree not present")
    out = G.compute(G.inputs())
    assert set(out) == set(fx.files)
    for k, v in out.items():
        if k.startswith("maxiou_") and k[len("maxiou_"):] in G.PRECISIONS:
            # compute_maximum_iou averages over a set of string keys: its order (and so the last bit) follows the hash seed
            _close(v, fx[k], 1e-14, k)
        else:
            assert np.array_equal(np.asarray(v), fx[k]), k


@pytest.mark.parametrize("prec", G.PRECISIONS)
def test_iou_entries_bit_exact(host_exe, tmp_path, fx, prec):
    g, h = _sets(fx, "ds_gt", prec, 1), _sets(fx, "ds_gen", prec, 2)
    rc, out = _host(host_exe, tmp_path, 3, g, h)
    assert rc == 0
    S = max(1, max(len(l) for _, l in g + h))
    out = out.reshape(len(g), S, S)
    mine = np.concatenate([out[r, :len(x[1]), :len(y[1])].ravel() for r, (x, y) in enumerate(zip(g, h))])
    assert np.array_equal(mine, fx[f"iou_entries_{prec}"])


@pytest.mark.parametrize("prec", ("f32", "f64"))
def test_average_iou_and_perceptual_entries(host_exe, tmp_path, fx, prec):
    v = _sets(fx, "avg", prec, 1)
    rc, out = _host(host_exe, tmp_path, 0, v)
    assert rc == 0
    out = out.reshape(len(v), 3)
    _close(out[:, 0], fx[f"avgiou_blt_{prec}"], RTOL[prec], "BLT")
    _close(out[:, 1], fx[f"avgiou_vtn_{prec}"], RTOL[prec], "VTN")
    # perceptual entries: double(ai) / (cells / 1024) in the reference's flat order; a layout painting nothing gives one 0
    ent = []
    for (b, _), cells in zip(v, out[:, 2]):
        N = len(b)
        if N < 2:
            continue
        if cells == 0:
            ent.append(np.zeros(1))
            continue
        ii, jj = np.meshgrid(range(N), range(N))
        ii, jj = ii.ravel(), jj.ravel()
        keep = ii != jj
        ltrb = [b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2]
        l, t, r, bb = (x for x in ltrb)
        lm, rm = np.maximum(l[ii[keep]], l[jj[keep]]), np.minimum(r[ii[keep]], r[jj[keep]])
        tm, bm = np.maximum(t[ii[keep]], t[jj[keep]]), np.minimum(bb[ii[keep]], bb[jj[keep]])
        ai = np.where((lm < rm) & (tm < bm), (rm - lm) * (bm - tm), np.zeros_like(l[0]))
        ent.append(ai.astype(np.float64) / (cells / 1024.0))
    assert np.array_equal(np.concatenate(ent), fx[f"blt_entries_{prec}"])
    # the public result: the mean over layouts
    _close([out[:, 0].mean(), out[:, 1].mean()], fx[f"avgiou_{prec}"], RTOL[prec], "public")


@pytest.mark.parametrize("prec", G.PRECISIONS)
def test_docsim_pairs(host_exe, tmp_path, fx, prec):
    g, h = _sets(fx, "ds_gt", prec, 1), _sets(fx, "ds_gen", prec, 2)
    rc, out = _host(host_exe, tmp_path, 1, g, h)
    assert rc == 0
    _close(out, fx[f"docsim_pairs_{prec}"], RTOL[prec], "docsim pairs")
    _close(out.mean(), fx[f"docsim_{prec}"], RTOL[prec], "docsim")


@pytest.mark.parametrize("prec", G.PRECISIONS)
def test_maxiou_pairs(host_exe, tmp_path, fx, prec):
    a, b = _sets(fx, "mx_a", prec, 1), _sets(fx, "mx_b", prec, 2)
    s1, s2 = maxiou_pair_list(a, b)
    rc, out = _host(host_exe, tmp_path, 2, s1, s2)
    assert rc == 0
    _close(out, fx[f"maxiou_pairs_{prec}"], RTOL[prec], "max-iou pairs")


def test_solver_against_scipy_on_random_matrices(host_exe, tmp_path):
    """Segments up to 32 with tied and random IoU matrices: the solver's optimum equals scipy's (value, not assignment)."""
    from scipy.optimize import linear_sum_assignment

    rng = np.random.default_rng(7)
    s1, s2, want = [], [], []
    for n in (4, 5, 8, 17, 25, 32, 32):
        for grid in (True, False):
            b1, b2 = G._boxes(rng, n, grid), G._boxes(rng, n, grid)
            lab = np.zeros(n, np.int64)
            s1.append((b1, lab))
            s2.append((b2, lab))
            ii, jj = np.meshgrid(range(n), range(n))
            l1 = [b1[:, 0] - b1[:, 2] / 2, b1[:, 1] - b1[:, 3] / 2, b1[:, 0] + b1[:, 2] / 2, b1[:, 1] + b1[:, 3] / 2]
            l2 = [b2[:, 0] - b2[:, 2] / 2, b2[:, 1] - b2[:, 3] / 2, b2[:, 0] + b2[:, 2] / 2, b2[:, 1] + b2[:, 3] / 2]
            p, q = [x[ii.ravel()] for x in l1], [x[jj.ravel()] for x in l2]
            a1, a2 = (p[2] - p[0]) * (p[3] - p[1]), (q[2] - q[0]) * (q[3] - q[1])
            lm, rm, tm, bm = np.maximum(p[0], q[0]), np.minimum(p[2], q[2]), np.maximum(p[1], q[1]), np.minimum(p[3], q[3])
            ai = np.where((lm < rm) & (tm < bm), (rm - lm) * (bm - tm), 0.0)
            m = (ai / (a1 + a2 - ai)).reshape(n, n)
            r, c = linear_sum_assignment(m, maximize=True)
            want.append(m[r, c].sum() / n)
    rc, out = _host(host_exe, tmp_path, 2, s1, s2)
    assert rc == 0
    _close(out, want, 1e-12, "solver")


def test_nan_iou_sets_the_error_flag(host_exe, tmp_path):
    z = np.zeros((2, 4))   # two zero-area boxes at the same spot: IoU 0 / 0
    rc, _ = _host(host_exe, tmp_path, 2, [(z, np.zeros(2, np.int64))], [(z, np.zeros(2, np.int64))])
    assert rc == 3


def test_host_build_under_address_and_undefined_sanitizers(tmp_path, fx):
    """every host-build case above on the ASan + UBSan build: the solver's state arrays are kMaxS + 1 long, the box, label and
    count arrays are exact-size allocations"""
    exe = HB.host_program("cpu_eval_iou_check", sanitize=True)
    for prec in G.PRECISIONS:
        test_iou_entries_bit_exact(exe, tmp_path, fx, prec)
        test_docsim_pairs(exe, tmp_path, fx, prec)
        test_maxiou_pairs(exe, tmp_path, fx, prec)
    for prec in ("f32", "f64"):
        test_average_iou_and_perceptual_entries(exe, tmp_path, fx, prec)
    test_solver_against_scipy_on_random_matrices(exe, tmp_path)
    test_nan_iou_sets_the_error_flag(exe, tmp_path)


def test_cabi_exports_and_argument_checks():
    import ctypes as C

    from layout_dm_amd import binding

    for name in ("ldm_eval_average_iou", "ldm_eval_docsim", "ldm_eval_max_iou_pairs"):
        assert name in binding.EXPORTS
    assert binding.ABI_VERSION == 5
    lib_path = binding.LIB_PATH
    if not os.path.exists(lib_path):
        pytest.skip("libldm_hip.so not built")
    lib = C.CDLL(lib_path)
    for name in ("ldm_eval_average_iou", "ldm_eval_docsim", "ldm_eval_max_iou_pairs"):
        assert hasattr(lib, name)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.ldm_eval_average_iou.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    lib.ldm_eval_docsim.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp]
    lib.ldm_eval_max_iou_pairs.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp, i32, i64, i32, vp, vp, vp]
    d = C.c_void_p(16)   # never dereferenced: every call below is refused before it touches memory or launches
    assert lib.ldm_eval_average_iou(d, 0, d, 4, 33, d, None) == -1          # S over the limit
    assert lib.ldm_eval_average_iou(d, 0, d, -1, 8, d, None) == -1          # negative count
    assert lib.ldm_eval_average_iou(d, 2, d, 4, 8, d, None) == -1           # box_f64 not 0 / 1
    assert lib.ldm_eval_average_iou(None, 0, None, 0, 8, None, None) == 0   # nothing to do
    assert lib.ldm_eval_docsim(d, 0, d, d, d, 1, d, d, 4, 40, d, d, None) == -1
    assert lib.ldm_eval_docsim(d, 0, d, d, d, 1, d, d, -3, 8, d, d, None) == -1
    assert lib.ldm_eval_max_iou_pairs(d, 0, d, 4, d, 0, 4, 33, d, 1, 1, 4, d, d, None) == -1
    assert lib.ldm_eval_max_iou_pairs(d, 0, d, 4, d, 0, 4, 8, d, -1, 1, 4, d, d, None) == -1
    assert lib.ldm_eval_max_iou_pairs(d, 0, d, 4, d, 0, 4, 8, d, 1, -5, 4, d, d, None) == -1
    assert lib.ldm_eval_max_iou_pairs(d, 0, d, 4, d, 0, 4, 8, d, 1, 1, 9, d, d, None) == -1   # max segment > S
