"""The PRDC kernels (kernels_prdc.hip: prdc_pdist2_k, prdc_kth_k, prdc_rows_k, prdc_cols_k behind ldm_prdc) EXACTLY, stage by
stage, on inputs where every comparison has one right answer.

Inputs live on an integer lattice (every feature coordinate a small integer stored as float32): every squared distance is an integer
<= dim * (2 * amp + 1)^2 <= 100 * 25 < 2^24, so a float32 sum of the squares is exact in any order, distances land exactly ON radii
(the strict '<'), rows hold equal distances (the tie pop of the wave-wide k-th-smallest extraction) and duplicated points give zero
distances and zero radii.  The device therefore has to equal an integer reference WITH NO TOLERANCE: the real x fake
squared-distance matrix, both sets' squared radii and the four raw counts, read through the development hook ldm_dev_prdc_stages
(the same launch sequence as ldm_prdc: one static function behind both); the ratios are np.float32(count / denominator).

The CPU half (not marked gpu) pins the inputs so that the GPU half cannot go vacuous: per case the in-test integer reference,
oracle.fid.compute_prdc and the route the prdc package takes (sklearn pairwise_distances + np.partition) give identical counts, at
least one cross distance lies exactly on a radius and the four scores are not all in {0, 1}.

Argument edges: ldm_prdc refuses (-1 / -6) before it allocates or launches anything; only refused calls are made there."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import fid as OF


def _lattice(n_real, n_fake, dim, amp, seed):
    rng = np.random.default_rng(seed)
    real = rng.integers(-amp, amp + 1, (n_real, dim))
    fake = rng.integers(-amp, amp + 1, (n_fake, dim)) + (rng.random((n_fake, dim)) < 0.15)
    return real.astype(np.int64), fake.astype(np.int64)


def _duplicates():
    real, fake = _lattice(96, 80, 40, 2, 8)
    fake[:12] = real[:12]
    real[12:24] = real[0]
    return real, fake


def _lane_column():
    # rows 0, 64, .., 448 of `real` identical: in row 0 of the real x real matrix the eight smallest entries (all zero) sit in
    # columns 0, 64, .., 448, i.e. all in lane 0's sorted list; the radius^2 of those rows is 0
    real, fake = _lattice(520, 40, 16, 2, 10)
    real[64:512:64] = real[0]
    return real, fake


def _identical_sets():
    real, _ = _duplicates()
    return real, real.copy()


# id -> (builder, nearest_k, trivial).  A trivial case may have no distance on a radius and all scores in {0, 1}.
CASES = {
    "smallest_2x2": (lambda: _lattice(2, 2, 1, 4, 1), 1, True),
    "n_fake_is_k_plus_1": (lambda: _lattice(9, 8, 1, 4, 2), 7, False),          # radius = row maximum, dim << 32, sets < a wave
    "k1_tile_plus_1": (lambda: _lattice(33, 130, 7, 3, 3), 1, False),           # one row / column past a 32-tile, rows % 4 != 0
    "dim_slab_plus_1": (lambda: _lattice(70, 45, 33, 2, 4), 5, False),          # zero padding of the last K-slab, m < 64
    "two_slabs_k7": (lambda: _lattice(129, 65, 64, 2, 5), 7, False),            # one past a tile / a wave, largest k
    "cols_block_straddle": (lambda: _lattice(257, 255, 100, 2, 6), 3, False),   # the 256-thread block of prdc_cols_k
    "heavy_ties": (lambda: _lattice(64, 64, 5, 1, 7), 2, False),
    "duplicates": (_duplicates, 5, False),                                      # zero distances, zero radii, equal minima
    "evicting_lists": (lambda: _lattice(31, 600, 31, 2, 9), 7, False),          # > 8 entries per lane in the fake x fake rows
    "lane_column": (_lane_column, 7, False),
    "identical_sets": (_identical_sets, 5, False),
}


def _d2(a, b):
    """Squared distances in integers, difference form."""
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.int64)
    for d in range(a.shape[1]):
        diff = a[:, d][:, None] - b[:, d][None, :]
        acc += diff * diff
    return acc


@functools.lru_cache(maxsize=None)
def _case(name):
    """(real, fake, k, reference) of a case, computed once and shared (nobody writes to it)."""
    build, k, _ = CASES[name]
    real, fake = build()
    r2_real, r2_fake = np.sort(_d2(real, real), -1)[:, k], np.sort(_d2(fake, fake), -1)[:, k]
    drf = _d2(real, fake)
    inside = drf < r2_real[:, None]
    counts = (int(inside.any(0).sum()), int((drf < r2_fake[None, :]).any(1).sum()), int(inside.sum()),
              int((drf.min(1) < r2_real).sum()))
    ref = {"drf": drf, "r2_real": r2_real, "r2_fake": r2_fake, "counts": counts,
           "on_edge": int((drf == r2_real[:, None]).sum() + (drf == r2_fake[None, :]).sum())}
    for a in (real, fake, drf, r2_real, r2_fake):
        a.setflags(write=False)
    return real, fake, k, ref


def _denominators(n_real, n_fake, k):
    return (n_fake, n_real, k * n_fake, n_real)


def _counts_of_scores(scores, n_real, n_fake, k):
    den = _denominators(n_real, n_fake, k)
    c = [scores[key] * d for key, d in zip(("precision", "recall", "density", "coverage"), den)]
    assert all(abs(x - round(x)) < 1e-6 for x in c), c
    return tuple(int(round(x)) for x in c)


# ------------------------------------------------------------------------------------------------ CPU: the inputs are pinned
@pytest.mark.parametrize("name", list(CASES))
def test_lattice_case_is_exact_and_not_vacuous(name):
    from sklearn.metrics import pairwise_distances

    real, fake, k, ref = _case(name)
    n_real, n_fake, dim = real.shape[0], fake.shape[0], real.shape[1]
    assert n_real > k and n_fake > k and max(n_real, n_fake) <= 600 and dim <= 100
    assert ref["drf"].max() < 2 ** 24 and _d2(real, real).max() < 2 ** 24 and _d2(fake, fake).max() < 2 ** 24
    # route 2: the oracle restatement (float64 Euclidean distances, np.partition)
    o = OF.compute_prdc(real, fake, nearest_k=k)
    assert _counts_of_scores(o, n_real, n_fake, k) == ref["counts"]
    # route 3: what the prdc package does (sklearn pairwise_distances + np.partition)
    rf, ff = real.astype(np.float64), fake.astype(np.float64)
    kth = lambda d: np.partition(d, k, axis=-1)[:, :k + 1].max(axis=-1)
    rr, rk = kth(pairwise_distances(rf, rf, metric="euclidean")), kth(pairwise_distances(ff, ff, metric="euclidean"))
    d = pairwise_distances(rf, ff, metric="euclidean")
    sk = (int((d < rr[:, None]).any(0).sum()), int((d < rk[None, :]).any(1).sum()), int((d < rr[:, None]).sum()),
          int((d.min(1) < rr).sum()))
    assert sk == ref["counts"]
    print(f"[prdc lattice {name}] {n_real}x{n_fake} dim={dim} k={k}: counts {ref['counts']} of {_denominators(n_real, n_fake, k)}, "
          f"{ref['on_edge']} cross distances on a radius")
    if not CASES[name][2]:
        assert ref["on_edge"] >= 1
        ratios = [c / d for c, d in zip(ref["counts"], _denominators(n_real, n_fake, k))]
        assert not all(r in (0.0, 1.0) for r in ratios), ratios


def test_special_cases_hold_what_they_are_built_for():
    real, fake, k, ref = _case("duplicates")
    assert (ref["drf"] == 0).sum() >= 12 and (ref["r2_real"] == 0).sum() >= 12
    real, fake, k, ref = _case("lane_column")
    assert k == 7 and (ref["r2_real"][0:512:64] == 0).all() and (ref["r2_real"] > 0).sum() > 500
    real, fake, k, ref = _case("identical_sets")
    assert np.array_equal(real, fake) and (ref["r2_real"] == 0).any() and ref["counts"][3] < real.shape[0]   # not all ones
    real, fake, k, ref = _case("n_fake_is_k_plus_1")
    assert np.array_equal(ref["r2_fake"], _d2(fake, fake).max(-1))


# ------------------------------------------------------------------------------------------------ GPU
def _lib():
    import torch

    from layout_dm_amd import binding

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    lib = binding.load_library()
    vp, i32 = C.c_void_p, C.c_int
    lib.ldm_prdc.argtypes = [vp, i32, vp, i32, i32, i32, C.POINTER(C.c_float), vp]
    lib.ldm_prdc.restype = i32
    lib.ldm_dev_prdc_stages.argtypes = [vp, i32, vp, i32, i32, i32, C.POINTER(C.c_float), vp, vp, C.POINTER(C.c_ulonglong), vp, vp]
    lib.ldm_dev_prdc_stages.restype = i32
    return lib


def _stages(lib, real, fake, k, with_matrix=True):
    """ldm_dev_prdc_stages on float32 copies of (real, fake): (ratios float32[4], counts, r2_real, r2_fake, drf or None)."""
    import torch

    r = torch.from_numpy(np.ascontiguousarray(real, dtype=np.float32)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(fake, dtype=np.float32)).cuda()
    n_real, n_fake = r.shape[0], f.shape[0]
    # (sentinels: a stage the hook did not write cannot pass for a result)
    r2r = torch.full((n_real,), -1.0, dtype=torch.float32, device="cuda")
    r2f = torch.full((n_fake,), -1.0, dtype=torch.float32, device="cuda")
    drf = torch.full((n_real, n_fake), -1.0, dtype=torch.float32, device="cuda") if with_matrix else None
    out, cnt = (C.c_float * 4)(*[-1.0] * 4), (C.c_ulonglong * 4)(*[2 ** 63] * 4)
    torch.cuda.synchronize()
    rc = lib.ldm_dev_prdc_stages(r.data_ptr(), n_real, f.data_ptr(), n_fake, r.shape[1], k, out, r2r.data_ptr(), r2f.data_ptr(), cnt,
                                 drf.data_ptr() if with_matrix else None, int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return (np.array(list(out), dtype=np.float32), tuple(int(c) for c in cnt), r2r.cpu().numpy(), r2f.cpu().numpy(),
            drf.cpu().numpy() if with_matrix else None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_prdc_stages_equal_the_integer_reference(name):
    from layout_dm_amd.fid import compute_prdc

    lib = _lib()
    real, fake, k, ref = _case(name)
    n_real, n_fake = real.shape[0], fake.shape[0]
    ratios, counts, r2r, r2f, drf = _stages(lib, real, fake, k)
    print(f"[prdc lattice {name}] device counts {counts}  reference {ref['counts']}")
    assert drf.dtype == np.float32 and np.array_equal(drf, ref["drf"].astype(np.float32))
    assert np.array_equal(r2r, ref["r2_real"].astype(np.float32))
    assert np.array_equal(r2f, ref["r2_fake"].astype(np.float32))
    assert counts == ref["counts"]
    want = np.array([np.float32(c / d) for c, d in zip(ref["counts"], _denominators(n_real, n_fake, k))], dtype=np.float32)
    assert np.array_equal(ratios, want)
    # the entry point itself, and the hook without the optional matrix
    got = compute_prdc(real.astype(np.float32), fake.astype(np.float32), nearest_k=k)
    assert [np.float32(got[key]) for key in ("precision", "recall", "density", "coverage")] == list(want)
    ratios2, counts2, r2r2, r2f2, _ = _stages(lib, real, fake, k, with_matrix=False)
    assert np.array_equal(ratios2, want) and counts2 == counts and np.array_equal(r2r2, r2r) and np.array_equal(r2f2, r2f)


@pytest.mark.gpu
def test_hook_and_entry_point_cannot_drift_apart():
    """A continuous case of test_fid_parity.py::test_prdc_vs_oracle through the hook: the stages it returns reproduce ldm_prdc's
    four outputs bit for bit (counts recomputed on the host from the returned float32 matrix and radii == the returned counts;
    np.float32(count / denominator) == ldm_prdc's ratios)."""
    import torch

    lib = _lib()
    n_real, n_fake, dim, k = 64, 333, 48, 3
    rng = np.random.default_rng(n_real + dim)
    real = rng.standard_normal((n_real, dim)).astype(np.float32)
    fake = (rng.standard_normal((n_fake, dim)) * 1.15 + 0.08).astype(np.float32)
    ratios, counts, r2r, r2f, drf = _stages(lib, real, fake, k)
    r, f = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    out = (C.c_float * 4)()
    assert lib.ldm_prdc(r.data_ptr(), n_real, f.data_ptr(), n_fake, dim, k, out, int(torch.cuda.current_stream().cuda_stream)) == 0
    entry = np.array(list(out), dtype=np.float32)
    assert np.array_equal(ratios, entry)
    inside = drf < r2r[:, None]
    host = (int(inside.any(0).sum()), int((drf < r2f[None, :]).any(1).sum()), int(inside.sum()), int((drf.min(1) < r2r).sum()))
    assert host == counts
    assert np.array_equal(np.array([np.float32(c / d) for c, d in zip(counts, _denominators(n_real, n_fake, k))]), entry)
    assert 0 < counts[2] and 0 < counts[3] < n_real
    # the radii are the (k + 1)-th smallest entries of the float32 distance rows the device itself would build
    assert (r2r > 0).all() and (r2f > 0).all()


REFUSED = [  # (n_real, n_fake, dim, k, return code)
    (10, 10, 4, 0, -1), (10, 10, 4, 8, -1), (5, 10, 4, 5, -1), (10, 5, 4, 5, -1), (10, 10, 0, 3, -1),
    (65537, 10, 1, 5, -6), (10, 65537, 1, 5, -6),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n_real,n_fake,dim,k,code", REFUSED)
def test_prdc_refuses_bad_arguments(n_real, n_fake, dim, k, code):
    """-1 for k = 0, k = 8, n_real == k, n_fake == k, dim = 0; -6 for 65 537 samples (dim = 1: the input is tiny, and the refusal
    comes before the n^2 workspace is asked for).  The output is left alone; compute_prdc raises.  Every call here is refused."""
    import torch

    from layout_dm_amd.fid import compute_prdc

    lib = _lib()
    r = torch.zeros((n_real, max(dim, 1)), dtype=torch.float32, device="cuda")
    f = torch.zeros((n_fake, max(dim, 1)), dtype=torch.float32, device="cuda")
    out = (C.c_float * 4)(*[-7.0] * 4)
    assert lib.ldm_prdc(r.data_ptr(), n_real, f.data_ptr(), n_fake, dim, k, out, None) == code
    assert list(out) == [-7.0] * 4
    with pytest.raises(RuntimeError):
        compute_prdc(np.zeros((n_real, dim), np.float32), np.zeros((n_fake, dim), np.float32), nearest_k=k)


@pytest.mark.gpu
def test_prdc_refuses_null_pointers():
    import torch

    lib = _lib()
    r = torch.zeros((10, 4), dtype=torch.float32, device="cuda")
    out = (C.c_float * 4)(*[-7.0] * 4)
    assert lib.ldm_prdc(None, 10, r.data_ptr(), 10, 4, 3, out, None) == -1
    assert lib.ldm_prdc(r.data_ptr(), 10, None, 10, 4, 3, out, None) == -1
    assert lib.ldm_prdc(r.data_ptr(), 10, r.data_ptr(), 10, 4, 3, None, None) == -1
    assert list(out) == [-7.0] * 4
    # the hook needs its stage buffers (only the matrix is optional)
    cnt = (C.c_ulonglong * 4)()
    assert lib.ldm_dev_prdc_stages(r.data_ptr(), 10, r.data_ptr(), 10, 4, 3, out, None, r.data_ptr(), cnt, None, None) == -1
    assert lib.ldm_dev_prdc_stages(r.data_ptr(), 10, r.data_ptr(), 10, 4, 3, out, r.data_ptr(), r.data_ptr(), None, None, None) == -1
