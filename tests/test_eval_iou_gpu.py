"""Max-IoU, DocSim and average IoU on the MI355X (kernels_eval_iou.hip through the C-ABI and the drop-ins of
layout_dm_amd/metrics.py) against tests/golden/eval_iou/reference.npz, the reference's own results (tools/make_eval_iou_golden.py):
rtol 1e-5 for float32 inputs, 1e-10 for float64 and the mixed float32 x float64 call.  No reference import here."""
import os

import numpy as np
import pytest
import torch

import _hostbuild as HB

RTOL = {"f32": 1e-5, "f64": 1e-10, "mix": 1e-10}
PRECISIONS = ("f32", "f64", "mix")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_iou", "reference.npz"))


def _layouts(fx, name, prec, which):
    f64 = prec == "f64" or (prec == "mix" and which == 2)
    out, o = [], 0
    for k in fx[f"{name}_n"]:
        out.append((fx[f"{name}_box"][o:o + k].astype(np.float64 if f64 else np.float32), fx[f"{name}_label"][o:o + k].copy()))
        o += k
    return out


def _close(a, b, rtol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = ~(np.abs(a - b) <= rtol * np.abs(b) + 1e-300)
    assert not bad.any(), (what, np.flatnonzero(bad)[:4], a[bad][:4], b[bad][:4])


@pytest.mark.parametrize("prec", PRECISIONS)
def test_maximum_iou_vs_reference_fixture(cuda, fx, prec):
    from scipy.optimize import linear_sum_assignment

    from layout_dm_amd import metrics as M

    a, b = _layouts(fx, "mx_a", prec, 1), _layouts(fx, "mx_b", prec, 2)
    groups = M.max_iou_pair_scores(a, b)
    assert [(n1, n2) for _, n1, n2, _ in groups] == [tuple(s) for s in fx[f"maxiou_group_size_{prec}"]]
    pairs = np.concatenate([s for *_, s in groups])
    assert len(pairs) % 64 != 0          # the last block is partly empty
    _close(pairs, fx[f"maxiou_pairs_{prec}"], RTOL[prec], "pairs")
    means = []
    for _, n1, n2, s in groups:
        m = s.reshape(n1, n2)
        ii, jj = linear_sum_assignment(m, maximize=True)
        means.append(m[ii, jj].mean())
    _close(means, fx[f"maxiou_group_mean_{prec}"], RTOL[prec], "group means")
    r = M.compute_maximum_iou(a, b, disable_parallel=False, n_jobs=4)
    assert isinstance(r, float)
    _close(r, fx[f"maxiou_{prec}"], RTOL[prec], "public")
    assert M.compute_maximum_iou(_layouts(fx, "nk_a", prec, 1), _layouts(fx, "nk_b", prec, 2)) == 0.0


@pytest.mark.parametrize("prec", PRECISIONS)
def test_docsim_vs_reference_fixture(cuda, fx, prec):
    from layout_dm_amd import metrics as M

    g, h = _layouts(fx, "ds_gt", prec, 1), _layouts(fx, "ds_gen", prec, 2)
    r = M.compute_docsim(g, h + h[:3])           # zip truncates to the shorter list
    assert isinstance(r, np.floating)
    _close(r, fx[f"docsim_{prec}"], RTOL[prec], "public")
    # per pair through the tensor form (padded rows, elements at arbitrary slots)
    S = max(len(l) for _, l in g + h) + 3
    rng = np.random.default_rng(0)

    def pad(ls):
        box = np.zeros((len(ls), S, 4), ls[0][0].dtype)
        lab = np.full((len(ls), S), 99, np.int64)
        mask = np.zeros((len(ls), S), bool)
        for r_, (b, l) in enumerate(ls):
            slots = np.sort(rng.choice(S, len(l), replace=False))
            box[r_, slots], lab[r_, slots], mask[r_, slots] = b, l, True
        return [torch.from_numpy(x).to(cuda) for x in (box, lab, mask)]

    out = M.docsim(*pad(g), *pad(h))
    assert out.is_cuda and out.dtype == torch.float64
    _close(out.cpu().numpy(), fx[f"docsim_pairs_{prec}"], RTOL[prec], "pairs")


@pytest.mark.parametrize("prec", ("f32", "f64"))
def test_average_iou_vs_reference_fixture(cuda, fx, prec):
    from layout_dm_amd import metrics as M

    v = _layouts(fx, "avg", prec, 1)
    r = M.compute_average_iou(v)
    assert set(r) == {"average_iou-BLT", "average_iou-VTN"} and all(isinstance(x, float) for x in r.values())
    _close([r["average_iou-BLT"], r["average_iou-VTN"]], fx[f"avgiou_{prec}"], RTOL[prec], "public")
    S = max(len(l) for _, l in v)
    box = np.zeros((len(v), S, 4), v[0][0].dtype)
    mask = np.zeros((len(v), S), bool)
    for i, (b, l) in enumerate(v):
        box[i, S - len(l):], mask[i, S - len(l):] = b, True          # valid slots at the end: the mask decides
    out = M.average_iou(torch.from_numpy(box).to(cuda), torch.from_numpy(mask).to(cuda))
    assert out.is_cuda and out.shape == (len(v), 2) and len(v) % 64 != 0
    _close(out[:, 0].cpu().numpy(), fx[f"avgiou_blt_{prec}"], RTOL[prec], "BLT")
    _close(out[:, 1].cpu().numpy(), fx[f"avgiou_vtn_{prec}"], RTOL[prec], "VTN")


def test_nan_iou_raises_value_error(cuda):
    from layout_dm_amd import metrics as M

    z = (np.zeros((2, 4), np.float32), np.zeros(2, np.int64))     # two zero-area boxes: IoU 0 / 0 (scipy raises there)
    with pytest.raises(ValueError):
        M.compute_maximum_iou([z], [z])
    with pytest.raises(ValueError):
        M.compute_average_iou([(np.zeros((40, 4), np.float32), np.zeros(40, np.int64))])   # over the element limit


def test_tensor_forms_on_decoded_samples_equal_list_forms(cuda):
    """A real sampling call (synthetic weights, T = 10, random sampler) decoded with kmeans-like centres (float64 boxes) and
    with linear bins (float32): the tensor forms on decode's device output equal the list drop-ins on the same layouts."""
    from layout_dm_amd import metrics as M
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion
    from oracle import spec as SP
    from oracle import synth

    spec = SP.RICO25
    m = HipMaskAndReplaceDiffusion(n_category=spec.n_category, precision="fast", max_batch=64, device=0)
    m.load_state_dict(synth.synth_state_dict(spec, seed=1, perturb=True))
    torch.manual_seed(0)
    tokens = m.sample(batch_size=100, sampling_cfg={"name": "random", "num_timesteps": 10})
    rng = np.random.default_rng(0)
    centres = np.sort(rng.integers(1, 64, (4, m.engine.n_bin)) / 64.0, axis=1)
    for cen in (None, torch.from_numpy(centres)):
        dec = m.engine.decode(tokens.int().to(cuda), centres=cen)
        bbox, label, mask = dec["bbox"], dec["label"], dec["mask"]
        assert bbox.is_cuda and bbox.dtype == (torch.float32 if cen is None else torch.float64)
        bb, ll, mm = bbox.cpu().numpy(), label.cpu().numpy(), mask.cpu().numpy()
        layouts = [(bb[i][mm[i]], ll[i][mm[i]]) for i in range(len(bb))]
        assert any(len(l) > 1 for _, l in layouts)
        t = M.average_iou(bbox, mask).cpu().numpy()
        r = M.compute_average_iou(layouts)
        assert np.array_equal([t[:, 0].mean(), t[:, 1].mean()], [r["average_iou-BLT"], r["average_iou-VTN"]])
        half = len(layouts) // 2
        d = M.docsim(bbox[:half], label[:half], mask[:half], bbox[half:2 * half], label[half:2 * half], mask[half:2 * half])
        assert d.cpu().numpy().mean() == M.compute_docsim(layouts[:half], layouts[half:2 * half])
        assert M.compute_maximum_iou(layouts[:half], layouts[half:]) >= 0.0


def test_scale_group_of_256_by_256_layouts_s25_vs_host_build(cuda, tmp_path):
    """One label multiset of 25 elements (segments of 10, 8, 4, 2, 1) in 256 + 300 layouts: 76 800 pairs in one launch,
    every 7th against the host build of the same source (float32 x float64)."""
    from layout_dm_amd import metrics as M

    rng = np.random.default_rng(5)
    key = np.repeat(np.arange(5), [10, 8, 4, 2, 1]).astype(np.int64)

    def lay(dt):
        b = np.concatenate([rng.uniform(0.1, 0.9, (25, 2)), rng.uniform(0.05, 0.6, (25, 2))], 1).astype(dt)
        return b, rng.permutation(key)

    a = [lay(np.float32) for _ in range(256)]
    b = [lay(np.float64) for _ in range(300)]
    (_, n1, n2, s), = M.max_iou_pair_scores(a, b)
    assert (n1, n2) == (256, 300) and s.shape == (256 * 300,)
    idx = np.arange(0, len(s), 7)
    srt = lambda x: (x[0][np.argsort(x[1], kind="stable")], np.sort(x[1], kind="stable"))  # noqa: E731
    s1 = [srt(a[k % n1]) for k in idx]
    s2 = [srt(b[k // n1]) for k in idx]
    payload = np.array([2, 0, 1, len(idx), 25], np.int32).tobytes()
    for ls, dt in ((s1, np.float32), (s2, np.float64)):
        payload += np.stack([x for x, _ in ls]).astype(dt).tobytes()
        payload += np.stack([l for _, l in ls]).astype(np.int64).tobytes()
        payload += np.full(len(ls), 25, np.int32).tobytes()
    rc, raw = HB.run_host_io(HB.host_program("cpu_eval_iou_check"), tmp_path, payload)   # (the plain build: no sanitizer next to a GPU)
    assert rc == 0, rc
    _close(s[idx], np.frombuffer(raw, np.float64), 1e-12, "scale")
