"""Coordinate bins from raw boxes (layout_dm_amd/clustering.py, kernels_cluster.hip) — CPU side.

The host build of the kernels' one source of arithmetic and summation orders (csrc/ldm_cluster_core.h through
tests/cpu_cluster_check.cpp) against the fixture of tools/make_clustering_golden.py: the reference's own Percentile (the -1
pattern equal, centres within the recorded ulp distance + 1) and scikit-learn's explicit-start Lloyd (centres to 1e-12, n_iter
equal, direct-pass inertia to 1e-9).  Hand-made rows for the documented rules (a point on a midpoint, a cluster that empties,
k = 1, n = k, all values equal, NaN), the Philox stream against a numpy restatement, the
inverse-CDF pick on hand-given uniforms.  The same program as the ASan + UBSan build.  The exports, their refusals,
the kernels' resource report, and the Python API: its refusals (a float64 that is no float32 among them) and its raising without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _clustering_cases as CC
import _hostbuild as HB

ROOT = CC.ROOT
NEW_EXPORTS = ("ldm_cluster_workspace_bytes", "ldm_cluster_sort", "ldm_kmeans1d_fit", "ldm_kmeans1d_lloyd", "ldm_percentile_fit",
               "ldm_nearest_centre", "ldm_dev_cluster_stages")


@pytest.fixture(scope="module")
def host_exe():
    return CC.build_host()


@pytest.fixture(scope="module")
def san_exe():
    return CC.build_host(sanitize=True)


def test_feature_is_present():
    """fails without the feature: the module, the exports in the header and in binding.EXPORTS, the sources in the build"""
    import layout_dm_amd.clustering as cl
    from layout_dm_amd import binding, build

    hdr = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in binding.EXPORTS and f"int {name}(" in hdr, name
    assert "kernels_cluster.hip" in build.SOURCES and "ldm_cluster_api.cpp" in build.SOURCES
    for name in ("KMeans1D", "Percentile", "ClusterModel", "fit_coordinate_bins", "save_clusters"):
        assert hasattr(cl, name), name
    assert cl.N_CLUSTERS_LIST == (2, 4, 8, 16, 32, 64, 128, 256)
    import layout_dm_amd.clustering_entry  # noqa: F401


def _percentile_fixture(exe, tmp):
    g = CC.golden()
    for kind in ("cont", "grid"):
        for n in CC.PCT_N:
            x = g[f"pct_{kind}_{n}_x"]
            for k in CC.PCT_K:
                rc, m, got = CC.host_percentile(exe, tmp, x, k)
                assert rc == 0 and m == len(np.unique(x.clip(0, 1))), (kind, n, k, rc, m)
                CC.check_percentile(got, g, kind, n, k)


def _lloyd_fixture(exe, tmp):
    g = CC.golden()
    for n, k in CC.LLOYD_NK:
        x, c0 = g[f"lloyd_{n}_{k}_x"], g[f"lloyd_{n}_{k}_c0"]
        for M in CC.LLOYD_M:
            r = CC.host_lloyd(exe, tmp, x, c0, M, 0.0)
            assert r["rc"] == 0
            CC.check_lloyd(r["centres"], r["inertia"], r["n_iter"], g, n, k, M)
            # the trace ends in the centres; fewer iterations are a prefix of more
            assert np.array_equal(r["trace"][-1], r["centres"])
        full = CC.host_lloyd(exe, tmp, x, c0, 300, 0.0)["trace"]
        assert np.array_equal(CC.host_lloyd(exe, tmp, x, c0, 5, 0.0)["trace"], full[:5])


def f32(*v):
    return np.array(v, np.float32)


def _hand_rows(exe, tmp):
    # a point exactly on a midpoint goes to the lower cluster
    r = CC.host_lloyd(exe, tmp, f32(0.0, 0.5, 1.0), [0.0, 1.0], 1)
    assert r["rc"] == 0 and np.array_equal(r["centres"], [0.25, 1.0]) and r["n_iter"] == 1
    # a cluster that empties keeps its centre (sklearn would relocate it)
    x = f32(0.0, 0.125, 0.875, 1.0)
    r = CC.host_lloyd(exe, tmp, x, [0.0625, 0.5, 0.9375], 300)
    assert r["rc"] == 0 and np.array_equal(r["centres"], [0.0625, 0.5, 0.9375])
    assert r["inertia"] == 4 * 0.0625 ** 2
    # k = 1: the mean; the second iteration moves no boundary
    x = f32(0.25, 0.5, 0.75, 1.0)
    r = CC.host_lloyd(exe, tmp, x, [0.0], 300)
    assert r["rc"] == 0 and np.array_equal(r["centres"], [0.625]) and r["n_iter"] == 2
    assert r["inertia"] == float(((x.astype(np.float64) - 0.625) ** 2).sum())
    # n = k: every point its own centre, whatever order they come in
    x = f32(0.75, 0.1, 0.3)
    r = CC.host_lloyd(exe, tmp, x, x.astype(np.float64), 300)
    assert r["rc"] == 0 and np.array_equal(r["centres"], np.sort(x).astype(np.float64)) and r["inertia"] == 0.0
    # all values equal: refused for kmeans with the distinct count, one real bin for percentile
    x = np.full(9, 0.3, np.float32)
    assert CC.host_lloyd(exe, tmp, x, [0.1, 0.2], 3) == {"rc": 5, "distinct": 1}
    rc, m, got = CC.host_percentile(exe, tmp, x, 4)
    assert rc == 0 and m == 1 and np.array_equal(got, f32(-1, -1, -1, 0.3))
    # -0.0 and +0.0 are one value
    rc, m, got = CC.host_percentile(exe, tmp, f32(-0.0, 0.0, 1.0), 2)
    assert rc == 0 and m == 2 and np.array_equal(got, f32(0.0, 1.0))
    # NaN / infinity refused
    for bad in (np.nan, np.inf, -np.inf):
        assert CC.host_percentile(exe, tmp, f32(0.1, bad, 0.2), 2)[0] == 3
        assert CC.host_lloyd(exe, tmp, f32(0.1, bad, 0.2), [0.1, 0.2], 3)["rc"] == 3
    # sizes refused
    assert CC.host_percentile(exe, tmp, f32(0.1), 0)[0] == 2 and CC.host_percentile(exe, tmp, f32(0.1), 257)[0] == 2
    assert CC.host_percentile(exe, tmp, f32(), 2)[0] == 2


def _pick_rows(exe, tmp):
    """u -> the first index whose cumulative weight exceeds u * total; integer weights, so every sum is exact"""
    def want(w, u):
        cum = np.cumsum(w)
        hit = np.nonzero(cum > u * cum[-1])[0]
        return int(hit[0]) if len(hit) else int(np.nonzero(w > 0)[0][-1])

    one = 1 - 2.0 ** -53
    w = np.array([0, 0, 1, 2, 0, 3, 0], np.float64)                       # a zero-weight prefix and a zero-weight tail
    us = [0.0, 1 / 6, 0.49, 0.5, 0.75, one]
    assert CC.host_pick(exe, tmp, w, us).tolist() == [2, 3, 3, 5, 5, 5] == [want(w, u) for u in us]
    w = np.array([1, 0, 0, 2], np.float64)                                # the last element
    assert CC.host_pick(exe, tmp, w, [0.0, 0.3, 1 / 3, 0.9, one]).tolist() == [0, 0, 3, 3, 3]
    assert CC.host_pick(exe, tmp, [5.0], [0.0, 0.5, one]).tolist() == [0, 0, 0]
    # several tiles: a first tile of zeros only, a tile boundary inside the support, a zero tail over the last tile
    g = np.random.default_rng(3)
    w = g.integers(0, 4, 5000).astype(np.float64)
    w[:1500] = 0
    w[4000:] = 0
    w[1024 * 2 - 1:1024 * 2 + 1] = 1
    us = np.concatenate([g.random(200), [0.0, one], (np.cumsum(w)[[1499, 1500, 2047, 2048, 3999]] / w.sum())])
    assert CC.host_pick(exe, tmp, w, us).tolist() == [want(w, u) for u in us]


def _philox_numpy(key, ctr):
    c = [np.uint64(v) for v in ctr]
    k0, k1 = np.uint64(key & 0xffffffff), np.uint64(key >> 32)
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return [int(v) for v in c]


def _philox_rows(exe, tmp):
    rows = [(0, 0, 0, 0), (256, 9, 255, 6), (32, 3, 1, 2), (1, 0, 7, 0), (2 ** 31 - 1, 63, 0, 1)]
    for state in (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1):
        got = CC.host_philox(exe, tmp, state, rows)
        for (problem, restart, step, cand), u in zip(rows, got):
            r = _philox_numpy(state, (step, cand, problem, restart))
            assert u == (((r[0] >> 5) << 26) | (r[1] >> 6)) / 2.0 ** 53 and 0.0 <= u < 1.0
    # the Random123 known answer for Philox4x32-10, counter = key = 0
    assert _philox_numpy(0, (0, 0, 0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # different restarts, steps, candidates: different numbers
    many = CC.host_philox(exe, tmp, 0, [(4, r, s, c) for r in range(10) for s in range(4) for c in range(3)])
    assert len(set(many.tolist())) == len(many)


def test_host_core_reproduces_the_reference_percentile(host_exe, tmp_path):
    _percentile_fixture(host_exe, tmp_path)


def test_host_core_reproduces_sklearn_lloyd(host_exe, tmp_path):
    _lloyd_fixture(host_exe, tmp_path)


def test_hand_made_rows(host_exe, tmp_path):
    _hand_rows(host_exe, tmp_path)


def test_philox_stream_and_inverse_cdf_pick(host_exe, tmp_path):
    _philox_rows(host_exe, tmp_path)
    _pick_rows(host_exe, tmp_path)


def test_host_prefix_sums_against_cumsum(host_exe, tmp_path):
    g = np.random.default_rng(0)
    for n in (1, 15, 16, 17, 4095, 4096, 4097, 70001):
        x = np.sort(g.random(n).astype(np.float32))
        ps, ps2 = CC.host_prefix(host_exe, tmp_path, x)
        ref, ref2 = np.cumsum(x.astype(np.float64)), np.cumsum(x.astype(np.float64) ** 2)
        assert ps[0] == 0 and ps2[0] == 0
        assert (np.abs(ps[1:] - ref) <= n * 2.0 ** -52 * ref).all() and (np.abs(ps2[1:] - ref2) <= n * 2.0 ** -52 * ref2).all()


def test_host_build_under_address_and_undefined_sanitizers(san_exe, tmp_path):
    """the same cases with the stand-alone program as the ASan + UBSan build: every array is an exact-size
    std::vector or new[], so a read or write past one, signed overflow or a bad shift ends the run with a non-zero code"""
    _percentile_fixture(san_exe, tmp_path)
    _lloyd_fixture(san_exe, tmp_path)
    _hand_rows(san_exe, tmp_path)
    _philox_rows(san_exe, tmp_path)
    _pick_rows(san_exe, tmp_path)


def test_exports_refuse_bad_arguments():
    from layout_dm_amd import binding, build

    lib = C.CDLL(build.build(verbose=False))
    vp, i32, i64, sz, u64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_uint64, C.c_double
    lib.ldm_cluster_workspace_bytes.argtypes = [i32, i64, i32, i32, C.POINTER(sz)]
    lib.ldm_cluster_sort.argtypes = [vp, i32, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]
    lib.ldm_kmeans1d_fit.argtypes = [vp, vp, vp, i32, i64, vp, vp, i32, i32, i32, u64, i32, f64, vp, vp, vp, vp, vp, sz, vp]
    lib.ldm_nearest_centre.argtypes = [vp, i64, vp, i32, i32, vp, vp]
    need = sz()
    assert lib.ldm_cluster_workspace_bytes(4, 100000, 32, 10, C.byref(need)) == 0 and need.value > 0
    small = sz()
    assert lib.ldm_cluster_workspace_bytes(4, 100000, 0, 1, C.byref(small)) == 0 and 0 < small.value < need.value
    for bad in ((0, 10, 1, 1), (1, 0, 1, 1), (1, 2 ** 31, 1, 1), (1, 10, -1, 1), (1, 10, 1, 0), (1, 10, 1, 65), (1, 10, 4096, 64)):
        assert lib.ldm_cluster_workspace_bytes(*bad, C.byref(need)) == -1, bad
    assert lib.ldm_cluster_workspace_bytes(1, 10, 1, 1, None) == -1
    d = C.c_void_p(256)   # never dereferenced: every call below is refused before it touches memory or launches
    big = 1 << 40
    assert lib.ldm_cluster_sort(None, 1, 10, 0, 3, d, d, d, d, d, d, d, big, d, None) == -1
    assert lib.ldm_cluster_sort(d, 1, 10, 2, 3, d, d, d, d, d, d, d, big, d, None) == -1
    assert lib.ldm_cluster_sort(d, 1, 10, 0, 3, d, d, d, d, d, d, d, 16, d, None) == -1           # workspace too small
    assert lib.ldm_cluster_sort(d, 1, 10, 0, 3, d, d, d, d, d, d, C.c_void_p(264), big, d, None) == -1   # not 256-byte aligned
    assert lib.ldm_cluster_sort(d, 1, 0, 0, 3, d, d, d, d, d, d, d, big, d, None) == -1        # n = 0
    assert lib.ldm_cluster_sort(d, 1, 10, 0, 0, d, d, d, d, d, d, d, big, d, None) == -1 and lib.ldm_cluster_sort(d, 1, 10, 0, 4, d, d, d, d, d, d, d, big, d, None) == -1

    def fit(prob, n=100, A=1, n_init=10, max_iter=300, tol=1e-4):
        h = (C.c_int32 * (3 * len(prob)))(*[v for row in prob for v in row])
        return lib.ldm_kmeans1d_fit(d, d, d, A, n, h, d, len(prob), n_init, 0, 0, max_iter, tol, d, d, d, d, d, big, None)

    for prob in ([(0, 257, 0)], [(0, 0, 0)], [(1, 4, 0)], [(-1, 4, 0)], [(0, 101, 0)], [(0, 4, 0), (0, 8, 1)]):
        assert fit(prob) == -1, prob            # k > 256, k < 1, array out of range, k > n, k not sorted
    assert fit([(0, 4, 0)], max_iter=0) == -1 and fit([(0, 4, 0)], tol=-1.0) == -1 and fit([(0, 4, 0)], n_init=0) == -1
    assert fit([(0, 4, 0)], tol=float("nan")) == -1
    assert lib.ldm_nearest_centre(d, 10, d, 0, 2, d, None) == -1 and lib.ldm_nearest_centre(d, 10, d, 257, 2, d, None) == -1
    assert lib.ldm_nearest_centre(d, 10, d, 4, 0, d, None) == -1        # linear bins have no centres
    assert lib.ldm_nearest_centre(None, 0, None, 4, 2, None, None) == 0  # nothing to do, nothing touched
    assert set(NEW_EXPORTS) <= set(binding.EXPORTS)


def test_python_api_refusals_and_no_silent_cpu_path():
    from layout_dm_amd import clustering as cl

    x = np.linspace(0, 1, 50, dtype=np.float32)
    for k in (0, 257, -3):
        with pytest.raises(ValueError, match="n_clusters"):
            cl.KMeans1D(k).fit(x)
        with pytest.raises(ValueError, match="n_clusters"):
            cl.Percentile(k).fit(x)
    with pytest.raises(ValueError, match="n = 0"):
        cl.KMeans1D(2).fit(np.zeros((0, 1), np.float32))
    with pytest.raises(ValueError, match="n = 0"):
        cl.fit_coordinate_bins(np.zeros((0, 4), np.float32), "kmeans")
    with pytest.raises(ValueError, match=r"\(N, 4\)"):
        cl.fit_coordinate_bins(np.zeros((5, 3), np.float32), "kmeans")
    with pytest.raises(ValueError, match="algorithm"):
        cl.fit_coordinate_bins(np.zeros((5, 4), np.float32), "dbscan")
    with pytest.raises(ValueError, match="float32 or float64"):
        cl.KMeans1D(2).fit(np.arange(10))
    # a float64 that is no float32 is refused, and so is a NaN: by the product's own check, before a device is asked for
    ok64 = np.array([float(np.float32(0.1)), 0.5, 2.0 ** -149, -0.0, 1.0], np.float64)
    for bad in (0.1, 1e-50, 1 + 2.0 ** -24):
        for fit in (cl.KMeans1D(2).fit, cl.Percentile(2).fit, lambda X: cl.fit_coordinate_bins(np.stack([X] * 4, 1), "kmeans")):
            with pytest.raises(ValueError, match="exactly a float32"):
                fit(np.append(ok64, bad))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="NaN or an infinite"):
            cl.KMeans1D(2).fit(np.append(ok64, bad))
    assert cl._values(torch.from_numpy(ok64), "t").dtype == torch.float32 if torch.cuda.is_available() else True
    m = cl.ClusterModel("kmeans", np.array([0.1, 0.5], np.float32))
    assert m.n_clusters == 2 and m.cluster_centers_.shape == (2, 1)
    import pickle

    assert pickle.loads(pickle.dumps(m)) == m
    if not torch.cuda.is_available():
        for call in (lambda: cl.KMeans1D(2).fit(x), lambda: cl.Percentile(2).fit(x), lambda: m.predict(x.reshape(-1, 1)),
                     lambda: cl.fit_coordinate_bins(np.zeros((5, 4), np.float32), "percentile")):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()


def test_cluster_kernels_use_no_scratch_and_no_float_atomics():
    asm, out, _ = HB.kernel_asm("kernels_cluster.hip", resource_report=True)
    blocks = re.split(r"Function Name: ", out)[1:]
    assert len(blocks) >= 18
    for blk in blocks:
        get = lambda pat: int(re.search(pat, blk).group(1))   # noqa: E731
        assert get(r"ScratchSize \[bytes/lane\]: (\d+)") == 0, blk
        assert get(r"VGPRs? Spill: (\d+)") == 0 and get(r"SGPRs? Spill: (\d+)") == 0, blk
        assert get(r"LDS Size \[bytes/block\]: (\d+)") <= 65536, blk
    ins = [ln.split(";")[0].strip() for ln in asm.splitlines()]
    ops = {i.split()[0] for i in ins if i and not i.startswith((".", "_", "$")) and not i.endswith(":")}
    # determinism: no floating-point atomic of any memory space; the integer LDS add of the radix histogram is the only atomic
    assert not [o for o in ops if re.search(r"(atomic|ds)_(pk_)?(add|min|max)_(rtn_)?f(16|32|64)", o) or "atomic_pk" in o], ops
    assert not [o for o in ops if o.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "scratch_"))], ops
    assert any(o.startswith("ds_add") and "u32" in o for o in ops), ops
