"""Relation violation score on the MI355X (kernels_violation.hip through the C-ABI and layout_dm_amd/metrics.py) against
tests/golden/relation_violation/reference.npz, the reference's own results (tools/make_relation_violation_golden.py): the flattened
form, the dense form and the per-edge outputs BIT FOR BIT on every graph and every edge, float32 and float64, NaN compared
by position.  Then the dense form on ldm_decode_layouts' output, the error path, the reference's function on the same device
tensors and the cond=relation entry point with and without the swap (the last two where the reference is importable)."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from test_relation_violation import CASES, G, assert_same_scores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "relation_violation", "reference.npz"))


def graph(y, ei, ea, batch, dev=None):
    d = {"y": torch.from_numpy(y), "edge_index": torch.from_numpy(ei), "edge_attr": torch.from_numpy(ea),
         "batch": torch.from_numpy(batch)}
    return {k: v.to(dev) for k, v in d.items()} if dev is not None else d


def densify(box, batch, rng, spare=3):
    """(bbox (B,S,4), mask (B,S)) whose bbox_c[mask_c] is `box`: node 0 of every graph is the canvas row test.py prepends,
    the others go to random slots of their layout, in order, with unused slots (garbage boxes) between them"""
    n = np.bincount(batch)
    B, S = len(n), int(n.max()) - 1 + spare
    bbox = rng.uniform(0, 1, (B, S, 4)).astype(box.dtype)
    mask = np.zeros((B, S), bool)
    first = np.r_[0, np.cumsum(n)]
    for b in range(B):
        assert tuple(box[first[b]]) == G.CANVAS
        slots = np.sort(rng.choice(S, n[b] - 1, replace=False))
        mask[b, slots] = True
        bbox[b, slots] = box[first[b] + 1:first[b + 1]]
    return bbox, mask


@pytest.mark.parametrize("name,prec", CASES)
def test_three_forms_equal_the_reference_fixture_bit_for_bit(cuda, fx, name, prec):
    from layout_dm_amd import metrics as M

    box, y, ei, ea, batch = G.load_inputs(fx)[name][prec]
    want = fx[f"{name}_score_{prec}"]
    bx = torch.from_numpy(box).to(cuda)
    # flattened form: the reference's signature; device graph and host graph
    for dev in (None, cuda):
        got = M.compute_violation(bx, graph(y, ei, ea, batch, dev))
        assert got.dtype == torch.float32 and got.shape == (int(batch.max()) + 1,)
        assert got.device.type == ("cpu" if dev is None else "cuda")    # data.x.device; without x, where the graph lives
        assert_same_scores(got.cpu().numpy(), want, (name, prec, "flat"))
    # dense form
    bbox, mask = densify(box, batch, np.random.default_rng(3))
    tb, tm = torch.from_numpy(bbox).to(cuda), torch.from_numpy(mask).to(cuda)
    assert torch.equal(torch.cat([torch.tensor(G.CANVAS, dtype=tb.dtype, device=cuda).expand(len(tb), 1, 4), tb], 1)[
        torch.cat([torch.ones(len(tb), 1, dtype=torch.bool, device=cuda), tm], 1)], bx)
    got = M.relation_violation(tb, tm, graph(y, ei, ea, batch))
    assert got.is_cuda
    assert_same_scores(got.cpu().numpy(), want, (name, prec, "dense"))
    # per edge, in edge_index's order
    size, loc, fail = (t.cpu().numpy() for t in M.relation_detect(bx, graph(y, ei, ea, batch)))
    for got_e, key in ((size, "size"), (loc, "loc")):
        ref = fx[f"{name}_{key}_{prec}"]
        bad = np.flatnonzero(got_e != ref)
        assert got_e.shape == ref.shape and bad.size == 0, (name, prec, key, bad[:8], got_e[bad[:8]], ref[bad[:8]])
    assert np.array_equal(fail, fx[f"{name}_failure_{prec}"])


def test_edges_in_any_order_and_hundreds_per_layout(cuda, fx):
    """no cap on edges per layout: every edge of the hand-made set five times over, shuffled across graphs (more than 64 per
    layout: several strides of a wavefront) — failures and valid both scale by five, the quotient stays"""
    from layout_dm_amd import metrics as M

    box, y, ei, ea, batch = G.load_inputs(fx)["edge"]["f32"]
    perm = np.random.default_rng(0).permutation(5 * ea.size) % ea.size
    got = M.compute_violation(torch.from_numpy(box).to(cuda), graph(y, ei[:, perm].copy(), ea[perm].copy(), batch))
    assert np.bincount(batch[ei[0]]).max() * 5 > 640
    assert_same_scores(got.cpu().numpy(), fx["edge_score_f32"], "shuffled x5")
    size, loc, fail = (t.cpu().numpy() for t in M.relation_detect(torch.from_numpy(box).to(cuda),
                                                                   graph(y, ei[:, perm].copy(), ea[perm].copy(), batch)))
    assert np.array_equal(size, fx["edge_size_f32"][perm]) and np.array_equal(loc, fx["edge_loc_f32"][perm])
    assert np.array_equal(fail, fx["edge_failure_f32"][perm])


def random_graph_for(mask, label, rng):
    """a relation graph over decoded layouts: 1 + mask count nodes per layout (canvas first), random edges and bitmasks"""
    ys, batch, src, dst = [], [], [], []
    first = 0
    for b in range(len(mask)):
        n = 1 + int(mask[b].sum())
        ys += [0] + (label[b][mask[b]] + 1).tolist()
        batch += [b] * n
        for _ in range(int(rng.integers(0, 3 * n))):
            i, j = rng.integers(0, n, 2)
            if i != j:
                src.append(first + i)
                dst.append(first + j)
        first += n
    ea = rng.integers(0, 1 << 10, len(src))
    return np.asarray(ys, np.int64), np.asarray([src, dst], np.int64).reshape(2, -1), ea.astype(np.int64), np.asarray(batch, np.int64)


def flatten_like_test_py(bbox, mask):
    """test.py:232-250 with torch, on the tensors' device"""
    B = bbox.size(0)
    canvas = torch.tensor([0.5, 0.5, 1.0, 1.0], dtype=torch.float32, device=bbox.device)
    bbox_c = torch.cat([canvas.expand(B, 1, 4), bbox], dim=1)
    mask_c = torch.cat([torch.ones(B, 1, dtype=torch.bool, device=bbox.device), mask.bool()], dim=1)
    return bbox_c[mask_c]


@pytest.fixture(scope="module")
def decoded(cuda):
    """a real sampling call (synthetic weights, T = 10, random sampler) decoded with linear bins (float32 boxes) and with
    kmeans-like centres (float64): what ldm_decode_layouts leaves on the device"""
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion
    from oracle import spec as SP
    from oracle import synth

    spec = SP.RICO25
    m = HipMaskAndReplaceDiffusion(n_category=spec.n_category, precision="fast", max_batch=64, device=0)
    m.load_state_dict(synth.synth_state_dict(spec, seed=1, perturb=True))
    torch.manual_seed(0)
    tokens = m.sample(batch_size=100, sampling_cfg={"name": "random", "num_timesteps": 10})
    centres = np.sort(np.random.default_rng(0).integers(1, 64, (4, m.engine.n_bin)) / 64.0, axis=1)
    return [m.engine.decode(tokens.int().to(cuda), centres=cen) for cen in (None, torch.from_numpy(centres))]


def test_dense_form_on_decode_output_equals_flattened_form(cuda, decoded):
    from layout_dm_amd import metrics as M

    for dec, dt in zip(decoded, (torch.float32, torch.float64)):
        bbox, mask = dec["bbox"], dec["mask"]
        assert bbox.is_cuda and bbox.dtype == dt
        mm, ll = mask.cpu().numpy().astype(bool), dec["label"].cpu().numpy()
        y, ei, ea, batch = random_graph_for(mm, ll, np.random.default_rng(1))
        assert ea.size > 500 and mm.sum(1).min() < mm.sum(1).max()
        flat = flatten_like_test_py(bbox, mask)
        assert flat.dtype == dt and len(flat) == len(y)
        want = M.compute_violation(flat.cpu(), graph(y, ei, ea, batch))
        got = M.relation_violation(bbox, mask, graph(y, ei, ea, batch))
        assert_same_scores(got.cpu().numpy(), want.numpy(), "decode")
        f = want[~want.isnan()]
        assert len(f.unique()) > 10

        # generated masks that disagree with the graph: layout 3 loses an element, layout 4 gains one (rows shift; the
        # reference reads whatever row the global index names) — still the flattened form on bbox_c[mask_c]
        m2 = mm.copy()
        k = [b for b in range(len(mm) - 1) if mm[b].sum() >= 2 and not mm[b + 1].all()][0]
        m2[k, np.flatnonzero(mm[k])[0]] = False
        m2[k + 1, np.flatnonzero(~mm[k + 1])[0]] = True
        tm2 = torch.from_numpy(m2).to(cuda)
        flat2 = flatten_like_test_py(bbox, tm2)
        assert len(flat2) == len(flat) and not torch.equal(flat2, flat)
        want2 = M.compute_violation(flat2, graph(y, ei, ea, batch))
        got2 = M.relation_violation(bbox, tm2, graph(y, ei, ea, batch))
        assert_same_scores(got2.cpu().numpy(), want2.cpu().numpy(), "shifted rows")


def test_mask_that_drops_a_named_element_is_an_error(cuda, decoded):
    """the last layout's last element has an edge; without it in the mask the edge names a row beyond bbox_c[mask_c]: the
    reference raises an IndexError, the kernel sets the error bit and reads nothing, the call gives no result"""
    from layout_dm_amd import binding, metrics as M

    dec = decoded[0]
    bbox, mask = dec["bbox"], dec["mask"].bool().clone()
    mm = mask.cpu().numpy()
    if not mm[-1].any():
        mask[-1, 0] = True
        mm = mask.cpu().numpy()
    y, ei, ea, batch = random_graph_for(mm, dec["label"].cpu().numpy(), np.random.default_rng(2))
    last = len(y) - 1
    ei = np.concatenate([ei, [[last - 1], [last]]], 1)
    ea = np.concatenate([ea, [1 << 2 | 1 << 6]])
    assert torch.isfinite(M.relation_violation(bbox, mask, graph(y, ei, ea, batch))[-1])
    short = mask.clone()
    short[-1, int(np.flatnonzero(mm[-1])[-1])] = False
    with pytest.raises(IndexError):
        M.relation_violation(bbox, short, graph(y, ei, ea, batch))
    with pytest.raises(IndexError):
        M.compute_violation(flatten_like_test_py(bbox, short), graph(y, ei, ea, batch))
    # the error bit itself, through the C-ABI
    n_graph, E, n_nodes, canvas, off, src, dst, attr, first, _ = M._violation_graph(graph(y, ei, ea, batch), cuda)
    out = torch.full((n_graph,), 7.0, device=cuda)
    err = torch.full((1,), 99, dtype=torch.int32, device=cuda)
    rows = torch.empty(len(mask) + 1, dtype=torch.int32, device=cuda)
    m8 = short.to(torch.uint8).contiguous()
    rc = binding.load_library().ldm_relation_violation_dense(
        bbox.data_ptr(), 0, m8.data_ptr(), len(mask), mask.shape[1], rows.data_ptr(), canvas.data_ptr(), n_nodes, off.data_ptr(),
        src.data_ptr(), dst.data_ptr(), attr.data_ptr(), first.data_ptr(), n_graph, E, out.data_ptr(), None, err.data_ptr(),
        binding._stream_ptr(cuda))
    torch.cuda.synchronize()
    assert rc == 0 and int(err.item()) == 1 and bool(out[-1].isnan())
    assert rows.cpu().tolist() == np.r_[0, np.cumsum(1 + short.cpu().numpy().sum(1))].tolist()


def _reference_metric():
    from oracle import ref_harness as rh

    if not rh.reference_importable():
        pytest.skip("neither the reference tree nor oracle/_ref/ present")
    rh.install_stubs()
    from trainer.helpers import metric

    return rh, metric


def test_reference_function_on_the_same_device_tensors(cuda, fx):
    rh, metric = _reference_metric()
    from layout_dm_amd import metrics as M

    box, y, ei, ea, batch = G.load_inputs(fx)["big"]["f32"]
    keep = batch[ei[0]] < 48                      # (the reference's loop syncs per edge: 48 layouts are enough here)
    n = int((batch < 48).sum())
    g = graph(y[:n], ei[:, keep], ea[keep], batch[:n])
    data = rh.GraphBatch(g["y"], g["edge_index"], g["edge_attr"], g["batch"])     # as test.py:251 calls it: the batch on the
    data.x = torch.from_numpy(box[:n])                                            # host, bbox_flatten.to(device)
    bx = data.x.to(cuda)
    want = metric.compute_violation(bx, data)
    got = M.compute_violation(bx, data)
    assert got.device == want.device and got.dtype == want.dtype
    assert_same_scores(got.cpu().numpy(), want.cpu().numpy(), "reference on device")
    assert_same_scores(got.cpu().numpy(), fx["big_score_f32"][:48], "fixture")


def test_entry_point_scores_equal_with_and_without_the_swap(cuda, tmp_path, monkeypatch, capsys):
    """cond=relation through the reference's own main(), as tests/test_entry_reference_main_gpu.py runs it (same job, same
    arguments), once with compute_violation swapped for the drop-in (the drop-in class installs it when main() builds it:
    layout_dm_amd/reference_hooks.py) and once with the reference's function behind the same seam.
    test.py keeps `relation_scores` out of the pickle unless `relations` is non-empty (test.py:262-264), and nothing fills
    it, so next to the pickles the per-batch score tensors are compared as the two functions return them, and the printed
    violation_score-mean."""
    rh, metric = _reference_metric()
    import yaml

    from layout_dm_amd import metrics as M
    from layout_dm_amd import synthetic as SY
    from layout_dm_amd import test_entry as TE
    from test_entry_reference_main_gpu import TRAIN_CFG

    rh.install_entry_stubs()
    import trainer.datasets.rico as rico
    import trainer.models.layoutdm as ref_layoutdm
    import trainer.test as ref_test

    job_dir = tmp_path / "job"
    job_dir.mkdir()
    (job_dir / "config.yaml").write_text(yaml.safe_dump(TRAIN_CFG))
    sd = {k: torch.from_numpy(v) for k, v in SY.synth_state_dict(SY.RICO25, seed=1, perturb=True).items()}
    torch.save(sd, job_dir / "best_model.pt")
    synth_ds = type("Rico25Dataset", (rh.SynthLayoutDataset,), {"labels": rico.Rico25Dataset.labels})
    monkeypatch.setattr(rico, "Rico25Dataset", synth_ds)
    monkeypatch.setattr(ref_test, "save_image", lambda *a, **k: None)
    monkeypatch.setattr(ref_layoutdm, "LayoutDM", ref_layoutdm.LayoutDM)
    monkeypatch.setattr(ref_test, "compute_violation", ref_test.compute_violation)
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    monkeypatch.chdir(tmp_path)
    common = ["cond=relation", f"job_dir={job_dir}", "max_batch_size=4", "num_uncond_samples=6", "sampling=deterministic",
              "num_timesteps=25"]
    seen = {}

    def spy(which, fn):
        def run(bbox_flatten, data):
            v = fn(bbox_flatten, data)
            seen.setdefault(which, []).append(v.detach().cpu().numpy())
            return v
        return run

    dropin = M.compute_violation
    out = {}
    for which, fn in (("ours", dropin), ("ref", metric.compute_violation)):
        monkeypatch.setattr(M, "compute_violation", spy(which, fn))     # what trainer.test.compute_violation now hands on to
        TE.main(common + [f"result_dir={tmp_path / which}"])
        out[which] = capsys.readouterr().out.strip().splitlines()[-2:]
    assert ref_test.compute_violation.reference is metric.compute_violation     # installed once, the original kept
    assert len(seen["ours"]) == len(seen["ref"]) >= 2
    for a, b in zip(seen["ours"], seen["ref"]):
        assert_same_scores(a, b, "per-batch scores")
    assert any((~np.isnan(a)).any() for a in seen["ours"])

    def printed(lines):
        keys, values = lines[0].split(","), lines[1].split(",")
        return values[keys.index("violation_score-mean")]

    assert printed(out["ours"]) == printed(out["ref"]) and float(printed(out["ours"])) >= 0.0

    def load(which):
        d = os.listdir(tmp_path / which)
        assert len(d) == 1 and d[0].startswith("relation_")
        return pickle.load(open(tmp_path / which / d[0] / "seed_0.pkl", "rb"))

    ours, ref = load("ours"), load("ref")
    assert set(ours) == set(ref) and ours.get("relation_scores") == ref.get("relation_scores")
    for (b1, l1), (b2, l2) in zip(ours["results"], ref["results"]):
        assert np.array_equal(b1, b2) and np.array_equal(l1, l2)
