"""GPU parity of the FID feature extractor (ldm_fid_features, kernels_fid.hip) — SURVEY §8f row 3:
features == the REAL reference's FIDNetV3.extract_features (golden) and == the oracle restatement on a full batch;
tolerance: fp32 accumulation-order noise (1e-4 absolute on features of magnitude ~3), stated here.

The extractor's edges: every slot count the C-ABI accepts at its ends (max_bbox = 31 with N = 31 — 32 rows, FID_MAXS exactly, the
only shape whose embedding GEMM reads the slack row behind the 32-row concat buffer — and N = 1), against the oracle restatement
evaluated in float64 at the same TOL; padded slots (whatever finite values they carry), the number of slots a layout is placed in,
and its place in the batch change NOTHING, bit for bit; a layout with every slot padded gives finite features equal to the oracle's.
ldm_prdc's end-to-end check on continuous clouds is here too; its kernels are pinned exactly in test_prdc_exact_gpu.py."""
import os

import numpy as np
import pytest
import torch

from oracle import fid as OF

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _model(num_label, max_bbox=25):
    from layout_dm_amd.fid import FIDNetV3

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    m = FIDNetV3(num_label=num_label, max_bbox=max_bbox)
    sd = OF.synth_fid_state_dict(num_label, seed=0, max_bbox=max_bbox)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.eval(), sd


def test_fid_features_vs_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "fid_v3.npz"))
    m, _ = _model(int(g["num_label"]))
    f = m.extract_features(torch.from_numpy(g["bbox"]), torch.from_numpy(g["label"]), torch.from_numpy(g["padding_mask"]))
    assert f.is_cuda and f.shape == (6, 256)
    err = np.abs(f.cpu().numpy() - g["features"]).max()
    print(f"[fid] max |feature - reference| = {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("num_label,N", [(25, 25), (5, 25), (25, 9)])
def test_fid_features_vs_oracle_full_batch(num_label, N):
    """B=512 layouts (the sampling batch), ragged element counts incl. empty layouts, fewer slots than max_bbox;
    then the FID of two feature sets through the same host formula."""
    from layout_dm_amd.fid import compute_fid

    m, sd = _model(num_label)
    bbox, label, pm = OF.synth_layouts(num_label, 512, N, seed=3)
    f = m.extract_features(torch.from_numpy(bbox), torch.from_numpy(label), torch.from_numpy(pm)).cpu().numpy()
    ref = OF.extract_features(sd, bbox, label, pm).numpy()
    assert np.abs(f - ref).max() <= TOL
    # batch-composition independence, bit for bit
    one = m.extract_features(torch.from_numpy(bbox[7:8]), torch.from_numpy(label[7:8]), torch.from_numpy(pm[7:8]))
    assert np.array_equal(one.cpu().numpy()[0], f[7])
    # FID of the device features == FID of the oracle's, and a perturbed set is further away than an identical one
    bbox2 = np.clip(bbox + 0.05, 0, 1).astype(np.float32)
    f2 = m.extract_features(torch.from_numpy(bbox2), torch.from_numpy(label), torch.from_numpy(pm)).cpu().numpy()
    ref2 = OF.extract_features(sd, bbox2, label, pm).numpy()
    fid_dev, fid_ref = compute_fid(f, f2), compute_fid(ref, ref2)
    assert abs(fid_dev - fid_ref) <= 1e-3 * max(1.0, abs(fid_ref))
    assert compute_fid(f, f) < 1e-6 < fid_dev
    assert m.extract_features(torch.zeros(0, N, 4), torch.zeros(0, N, dtype=torch.long),
                              torch.zeros(0, N, dtype=torch.bool)).shape == (0, 256)


def test_fid_rejects_bad_geometry():
    from layout_dm_amd.fid import FIDNetV3

    with pytest.raises(RuntimeError):
        FIDNetV3(num_label=25, max_bbox=40)          # one workgroup holds token + <= 31 elements
    m, _ = _model(25)
    with pytest.raises(RuntimeError):
        m.extract_features(torch.zeros(1, 26, 4), torch.zeros(1, 26, dtype=torch.long), torch.zeros(1, 26, dtype=torch.bool))
    for bad in (0, 32):                              # ldm_fid_create takes max_bbox in [1, 31]
        with pytest.raises(RuntimeError):
            FIDNetV3(num_label=25, max_bbox=bad)
    m31, _ = _model(25, max_bbox=31)
    with pytest.raises(RuntimeError):                # N > max_bbox, at the largest model
        m31.extract_features(torch.zeros(1, 32, 4), torch.zeros(1, 32, dtype=torch.long), torch.zeros(1, 32, dtype=torch.bool))
    assert m31.extract_features(torch.zeros(1, 31, 4), torch.zeros(1, 31, dtype=torch.long),
                                torch.zeros(1, 31, dtype=torch.bool)).shape == (1, 256)


def _features(m, bbox, label, pm):
    return m.extract_features(torch.from_numpy(bbox), torch.from_numpy(label), torch.from_numpy(pm)).cpu().numpy()


def _ref64(sd, bbox, label, pm):
    return OF.extract_features(sd, bbox, label, pm, dtype=torch.float64).numpy()


@pytest.mark.parametrize("num_label", [25, 1])
@pytest.mark.parametrize("max_bbox,N", [(31, 31), (31, 1), (25, 1)])
def test_fid_features_at_the_slot_count_edges_vs_float64(max_bbox, N, num_label):
    """B = 5 ragged layouts (element counts include 0 and N) against the oracle restatement in float64, at TOL.
    Measured max |device - float64| on an MI355X: 1.4e-6 (N = 31, 25 labels), 1.6e-6 (N = 1, 25 labels), 1.9e-6 (one label, N = 31
    and N = 1) on features of magnitude 3 — fp32 rounding, 50 x under TOL."""
    m, sd = _model(num_label, max_bbox)
    bbox, label, pm = OF.synth_layouts(num_label, 5, N, seed=11 + N)
    n = (~pm).sum(1)
    assert n[0] == 0 and n[-1] == N
    f = _features(m, bbox, label, pm)
    ref = _ref64(sd, bbox, label, pm)
    err = np.abs(f - ref).max()
    print(f"[fid edges max_bbox={max_bbox} N={N} num_label={num_label}] max |device - float64 oracle| = {err:.3e} "
          f"(features up to {np.abs(ref).max():.2f})")
    assert f.shape == (5, 256) and np.isfinite(f).all()
    assert err <= TOL
    if N == 31:
        # batch placement: first, last or alone, the same bits
        i = 3
        alone = _features(m, bbox[i:i + 1], label[i:i + 1], pm[i:i + 1])[0]
        order = [i, 0, 1, 2, 4]
        first = _features(m, bbox[order], label[order], pm[order])[0]
        order = [0, 1, 2, 4, i]
        last = _features(m, bbox[order], label[order], pm[order])[-1]
        assert np.array_equal(alone, f[i]) and np.array_equal(first, f[i]) and np.array_equal(last, f[i])


@pytest.mark.parametrize("max_bbox", [25, 31])
def test_fid_features_ignore_what_padded_slots_hold(max_bbox):
    """The kernel masks padded keys to -inf and weights their values by an exact 0: any finite content of a padded slot leaves the
    features bit-identical to the run with clean (zero box, label 0) padded slots."""
    num_label, N = 25, max_bbox
    m, _ = _model(num_label, max_bbox)
    bbox, label, pm = OF.synth_layouts(num_label, 5, N, seed=21)
    assert pm.any() and (~pm).any()
    clean_b, clean_l = np.where(pm[..., None], np.float32(0), bbox), np.where(pm, 0, label)
    want = _features(m, clean_b, clean_l, pm)
    assert np.isfinite(want).all()
    variants = {
        "boxes 1e30": (np.where(pm[..., None], np.float32(1e30), bbox), clean_l),
        "boxes -1e30": (np.where(pm[..., None], np.float32(-1e30), bbox), clean_l),
        "labels num_label - 1": (clean_b, np.where(pm, num_label - 1, label)),
        "another layout's slots": (np.where(pm[..., None], np.roll(bbox, 1, axis=0), bbox), np.where(pm, np.roll(label, 1, axis=0), label)),
        "random slots": (bbox, label),
    }
    for what, (b, l) in variants.items():
        got = _features(m, np.ascontiguousarray(b, dtype=np.float32), np.ascontiguousarray(l, dtype=np.int64), pm)
        assert np.array_equal(got, want), what


@pytest.mark.parametrize("n", [1, 4, 9])
def test_fid_features_do_not_depend_on_the_slot_count(n):
    """The same n elements in N = n, 9, 25 slots (max_bbox = 25 model) and 31 slots (max_bbox = 31 model), the rest padded:
    bit-identical features (the weights do not depend on max_bbox)."""
    num_label, B = 25, 3
    rng = np.random.default_rng(40 + n)
    eb, el = rng.random((B, n, 4)).astype(np.float32), rng.integers(0, num_label, (B, n)).astype(np.int64)

    def placed(N):
        bbox, label, pm = np.zeros((B, N, 4), np.float32), np.zeros((B, N), np.int64), np.ones((B, N), bool)
        bbox[:, :n], label[:, :n], pm[:, :n] = eb, el, False
        return bbox, label, pm

    m25, sd25 = _model(num_label, 25)
    m31, sd31 = _model(num_label, 31)
    assert all(np.array_equal(sd25[k], sd31[k]) for k in sd25)
    want = _features(m25, *placed(n))
    assert np.abs(want - _ref64(sd25, *placed(n))).max() <= TOL
    for m, N in ((m25, 9), (m25, 25), (m31, n), (m31, 25), (m31, 31)):
        assert np.array_equal(_features(m, *placed(N)), want), N


@pytest.mark.parametrize("max_bbox", [25, 31])
def test_fid_features_of_a_fully_padded_layout(max_bbox):
    """Only the [token] slot attends: finite features, equal to the oracle's (measured 1.4e-6 from float64), whatever N is and
    whatever the slots hold."""
    num_label = 25
    m, sd = _model(num_label, max_bbox)
    got = {}
    for N in (1, 9, max_bbox):
        bbox, label, _ = OF.synth_layouts(num_label, 2, N, seed=5)
        pm = np.ones((2, N), bool)
        f = _features(m, bbox, label, pm)
        assert np.isfinite(f).all()
        err = np.abs(f - _ref64(sd, bbox, label, pm)).max()
        print(f"[fid fully padded max_bbox={max_bbox} N={N}] max |device - float64 oracle| = {err:.3e}")
        assert err <= TOL
        got[N] = f
    assert all(np.array_equal(f, got[1]) and np.array_equal(f[0], f[1]) for f in got.values())


@pytest.mark.parametrize("n_real,n_fake,dim,k", [(700, 500, 256, 5), (64, 333, 48, 3), (257, 257, 256, 7)])
def test_prdc_vs_oracle(n_real, n_fake, dim, k):
    """ldm_prdc (kernels_prdc.hip) == the restatement of prdc.compute_prdc on random feature clouds that overlap only
    partly (so that none of the four numbers is trivially 0 or 1); identical sets give precision = recall = coverage = 1."""
    from layout_dm_amd.fid import compute_generative_model_scores, compute_prdc

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    rng = np.random.default_rng(n_real + dim)
    real = rng.standard_normal((n_real, dim)).astype(np.float32)
    fake = (rng.standard_normal((n_fake, dim)) * 1.15 + 0.08).astype(np.float32)
    got, ref = compute_prdc(real, fake, nearest_k=k), OF.compute_prdc(real, fake, nearest_k=k)
    print(f"[prdc n={n_real}x{n_fake} dim={dim} k={k}] device {got}  oracle {ref}")
    for key in ("precision", "recall", "density", "coverage"):
        assert 0.0 < ref[key] or key in ("precision", "recall")
        assert abs(got[key] - ref[key]) <= 2.0 / min(n_real, n_fake) + 1e-6, (key, got[key], ref[key])  # <= 2 samples on a '<' edge
    same = compute_prdc(real, real, nearest_k=k)
    assert same["precision"] == 1.0 and same["recall"] == 1.0 and same["coverage"] == 1.0
    if k == 5:
        full = compute_generative_model_scores([torch.from_numpy(real[:300]), torch.from_numpy(real[300:])], torch.from_numpy(fake))
        assert set(full) == {"precision", "recall", "density", "coverage", "fid"} and full["fid"] > 0
