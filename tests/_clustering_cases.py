"""Shared by test_clustering.py (CPU) and test_clustering_gpu.py: the fixture of tools/make_clustering_golden.py and the host
build of csrc/ldm_cluster_core.h (tests/cpu_cluster_check.cpp) with one runner per mode of that program."""
import os

import numpy as np

import _hostbuild as HB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clustering", "reference.npz")
PCT_N, PCT_K = (1, 5, 40, 257, 5000), (2, 32, 256)
LLOYD_M, LLOYD_NK = (1, 5, 300), ((257, 4), (1000, 32), (5000, 128), (20000, 256))
FULL_DATA, FULL_K = ("cont", "grid", "mix"), (4, 32, 128)

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def build_host(sanitize=False):
    """(the builder's -ffp-contract=off: every product and sum rounded, as the device build; the header's pragma covers clang only)"""
    return HB.host_program("cpu_cluster_check", sanitize=sanitize)


def _run(exe, tmp, mode, payload: bytes):
    return HB.run_host_io(exe, tmp, payload, mode)


def i32(*v):
    return np.array(v, np.int32).tobytes()


def host_percentile(exe, tmp, x, k):
    """-> (exit code, m, float32 centres (k))"""
    x = np.ascontiguousarray(x, np.float32)
    rc, raw = _run(exe, tmp, "percentile", i32(x.size, k) + x.tobytes())
    if rc != 0:
        return rc, None, None
    return rc, int(np.frombuffer(raw[:8], np.int64)[0]), np.frombuffer(raw[8:], np.float32)


def host_lloyd(exe, tmp, x, c0, max_iter, tol=0.0):
    """-> dict(rc, n_iter, inertia, centres (k), trace (n_iter, k)); rc 5: dict(rc, distinct)"""
    x, c0 = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(c0, np.float64)
    k = c0.size
    rc, raw = _run(exe, tmp, "lloyd", i32(x.size, k, max_iter) + np.float64(tol).tobytes() + x.tobytes() + c0.tobytes())
    if rc == 5:
        return {"rc": rc, "distinct": int(np.frombuffer(raw[:8], np.int64)[0])}
    if rc != 0:
        return {"rc": rc}
    n_iter = int(np.frombuffer(raw[:4], np.int32)[0])
    body = np.frombuffer(raw[4:], np.float64)
    return {"rc": 0, "n_iter": n_iter, "inertia": float(body[0]), "centres": body[1:1 + k], "trace": body[1 + k:].reshape(n_iter, k)}


def host_prefix(exe, tmp, x):
    x = np.ascontiguousarray(x, np.float32)
    rc, raw = _run(exe, tmp, "prefix", i32(x.size) + x.tobytes())
    assert rc == 0
    both = np.frombuffer(raw, np.float64)
    return both[:x.size + 1], both[x.size + 1:]


def host_pick(exe, tmp, w, u):
    w, u = np.ascontiguousarray(w, np.float64), np.ascontiguousarray(u, np.float64).reshape(-1)
    rc, raw = _run(exe, tmp, "pick", i32(w.size, u.size) + w.tobytes() + u.tobytes())
    assert rc == 0
    return np.frombuffer(raw, np.int64)


def host_philox(exe, tmp, random_state, rows):
    """rows: (m, 4) {problem, restart, step, candidate} -> m float64 uniforms"""
    rows = np.ascontiguousarray(rows, np.int32).reshape(-1, 4)
    rc, raw = _run(exe, tmp, "philox", np.uint64(random_state).tobytes() + i32(len(rows)) + rows.tobytes())
    assert rc == 0
    return np.frombuffer(raw, np.float64)


def ulp_distance(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def check_percentile(got, g, kind, n, k):
    """the bars of fixture (a): the -1 pattern equal, centres within the stored ulp distance + 1"""
    ref, slack = g[f"pct_{kind}_{n}_{k}_centres"], int(g[f"pct_{kind}_{n}_{k}_ulp"]) + 1
    got = np.asarray(got, np.float32).reshape(-1)
    assert got.shape == ref.shape
    assert np.array_equal(got == -1.0, ref == -1.0), (kind, n, k)
    live = ref != -1.0
    d = ulp_distance(got[live], ref[live])
    assert d.max(initial=0) <= slack, (kind, n, k, int(d.max()), slack)


def check_lloyd(centres, inertia, n_iter, g, n, k, M):
    """the bars of fixture (b): centres <= 1e-12, n_iter equal, direct-pass inertia <= 1e-9 relative"""
    ref, ref_j, ref_it = g[f"lloyd_{n}_{k}_{M}_centres"], float(g[f"lloyd_{n}_{k}_{M}_inertia"]), int(g[f"lloyd_{n}_{k}_{M}_n_iter"])
    err = float(np.abs(np.asarray(centres) - ref).max())
    rel = abs(float(inertia) - ref_j) / ref_j
    print(f"lloyd n={n} k={k} M={M}: centres err {err:.3g}, inertia rel {rel:.3g}, n_iter {n_iter} / {ref_it}")
    assert err <= 1e-12 and int(n_iter) == ref_it and rel <= 1e-9, (n, k, M, err, rel, n_iter, ref_it)
