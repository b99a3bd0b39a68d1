"""GPU: cond= inputs built from raw layouts on the device (layout_dm_amd/task.py -> ldm_encode_cond / ldm_relation_graph).

  * the comparisons of tests/test_cond_builder.py through the C-ABI on the device: the reference's own get_cond results of
    tests/golden/rico25_getcond.npz bit for bit from raw x / y / batch, the linear-bin boundaries against torch, host-resident
    and device-resident inputs identical;
  * end to end: task.get_cond with the captured randomness == the fixture's cond, and LayoutDM's greedy tokens under it ==
    the reference's `*_greedy_tokens` in the exact and the split numerics modes (the bar tests/test_getcond_gpu.py holds for
    reference-produced dicts);
  * own draws at B = 512: counts, combinations order, noise moments within five standard errors, cut invariance, seeds;
  * sample_from_layouts == get_cond followed by sample; the relation cond feeds metrics.compute_violation unchanged."""
import os

import numpy as np
import pytest
import torch

from oracle import spec as SP
from oracle import synth

from _stub_tokenizer import StubTokenizer  # noqa: E402
from test_cond_builder import E, N_BIN, N_CATEGORY, PAD, boundary_boxes, dense_of, sub, torch_linear_encode  # noqa: E402
from test_getcond_gpu import BACKBONE_CFG, _sampling_cfg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def tok():
    return StubTokenizer(SP.RICO25)


@pytest.fixture(scope="module")
def getcond(golden_dir):
    return np.load(os.path.join(golden_dir, "rico25_getcond.npz"))


def layouts_of(s, ctype, dev=None):
    bbox, label, mask = dense_of(s["x"], s["y"], s["batch"], canvas=ctype == "relation")
    out = {"bbox": torch.from_numpy(bbox), "label": torch.from_numpy(label), "mask": torch.from_numpy(mask).bool()}
    return {k: v.to(dev) for k, v in out.items()} if dev is not None else out


def captured(s, ctype):
    """the randomness the reference used, as task.get_cond takes it"""
    from layout_dm_amd.task import selection_from_edges

    if ctype == "partial":
        return {"keep": torch.from_numpy(s["cond_mask"][:, ::5])}
    if ctype == "relation":
        return {"selection": selection_from_edges(s["edge_index"], s["edge_attr"], s["batch"], int(s["batch"].max()) + 1, E)}
    return {}


def assert_cond_is_the_fixtures(cond, s, ctype):
    assert sorted(cond) == list(s["cond_keys"])
    assert cond["seq"].dtype == torch.int64 and cond["mask"].dtype == torch.bool and cond["type"] == ctype
    assert np.array_equal(cond["seq"].cpu().numpy(), s["cond_seq"].astype(np.int64))
    assert np.array_equal(cond["mask"].cpu().numpy(), s["cond_mask"])
    if "num_element" in s:
        assert cond["num_element"].dtype == torch.int64 and np.array_equal(cond["num_element"].cpu().numpy(), s["num_element"])
    if ctype == "relation":
        g = cond["batch_w_canvas"]
        assert np.array_equal(g.edge_index.cpu().numpy(), s["edge_index"]) and g.edge_index.dtype == torch.int64
        assert np.array_equal(g.edge_attr.cpu().numpy(), s["edge_attr"]) and g.edge_attr.dtype == torch.int64
        assert np.array_equal(g.y.cpu().numpy(), s["y"]) and np.array_equal(g.batch.cpu().numpy(), s["batch"])
        assert g.x.dtype == torch.float32 and np.array_equal(g.x.cpu().numpy(), s["x"])
        assert bool(g.attr["has_canvas_element"].all())


@pytest.mark.parametrize("ctype", ["c", "cwh", "partial", "relation"])
def test_device_get_cond_reproduces_the_reference(cuda, tok, getcond, ctype):
    from layout_dm_amd import task

    s = sub(getcond, ctype + "_")
    host = task.get_cond(layouts_of(s, ctype), tok, ctype, **captured(s, ctype))
    assert_cond_is_the_fixtures(host, s, ctype)
    assert host["seq"].device.type == "cpu"
    dev = task.get_cond(layouts_of(s, ctype, cuda), tok, ctype, **captured(s, ctype))
    assert dev["seq"].is_cuda and dev["mask"].is_cuda
    assert_cond_is_the_fixtures(dev, s, ctype)
    for k in ("seq", "mask"):
        assert torch.equal(host[k], dev[k].cpu())
    # the plain encode: the kept tokens of the reference's cond are its tokens
    enc = task.encode(tok, **layouts_of(s, ctype))
    kept = torch.from_numpy(s["cond_mask"]) & enc["mask"]
    assert enc["seq"].dtype == torch.int64 and enc["mask"].dtype == torch.bool
    assert torch.equal(enc["seq"][kept], torch.from_numpy(s["cond_seq"].astype(np.int64))[kept])


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_device_linear_boundaries_follow_torch(cuda, tok, T):
    from layout_dm_amd import task

    boxes = boundary_boxes(T)
    M = len(boxes)
    B = (M + E - 1) // E
    bbox = np.zeros((B * E, 4), T)
    bbox[:M] = boxes
    mask = np.zeros(B * E, bool)
    mask[:M] = True
    bbox, mask = torch.from_numpy(bbox.reshape(B, E, 4)), torch.from_numpy(mask.reshape(B, E))
    label = (torch.arange(B * E) % N_CATEGORY).reshape(B, E)
    for dev in (None, cuda):
        mv = (lambda t: t) if dev is None else (lambda t: t.to(dev))
        out = task.encode(tok, mv(bbox), mv(label), mv(mask))
        got = out["seq"].cpu().reshape(B, E, 5)
        assert torch.equal(got[mask][:, 1:], torch_linear_encode(bbox)[mask]) and torch.equal(got[mask][:, 0], label[mask])
        assert bool((got[~mask] == PAD).all()) and torch.equal(out["mask"].cpu(), mask.repeat_interleave(5, dim=1))


def test_refinement_with_supplied_noise_follows_torch(cuda, tok, getcond):
    from layout_dm_amd import task

    s = sub(getcond, "refinement_")
    lay = layouts_of(s, "refinement")
    noise = torch.normal(0, 0.1, size=lay["bbox"].shape, generator=torch.Generator().manual_seed(3))
    for dt in (torch.float32, torch.float64):
        cur = dict(lay, bbox=lay["bbox"].to(dt))
        cond = task.get_cond(cur, tok, "refinement", noise=noise)
        assert sorted(cond) == list(s["cond_keys"])
        valid = lay["mask"]
        t = torch.cat([lay["label"][..., None], torch_linear_encode(cur["bbox"] + noise)], dim=-1)
        t[~valid] = PAD
        orig = t.reshape(len(valid), -1)
        v5 = valid.repeat_interleave(5, dim=1)
        m = v5 & (torch.arange(5 * E) % 5 == 0) | ~v5
        seq = torch.where(v5, torch.where(m, orig, torch.tensor(PAD + 1)), torch.tensor(PAD))
        assert torch.equal(cond["seq_orig"], orig) and torch.equal(cond["seq"], seq) and torch.equal(cond["mask"], m)
        assert np.array_equal(cond["num_element"].numpy(), s["num_element"])


@pytest.fixture(scope="module")
def models(cuda, tok):
    from layout_dm_amd.layoutdm import LayoutDM

    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(SP.RICO25, seed=1, perturb=True).items()}
    out = {}
    for prec in ("exact", "split"):
        m = LayoutDM(backbone_cfg=BACKBONE_CFG, tokenizer=tok, q_type="constrained", max_batch=8, precision=prec).to("cuda")
        m.load_state_dict(sd)
        out[prec] = m.eval()
    return out


@pytest.mark.parametrize("ctype", ["c", "cwh", "partial", "relation"])
def test_end_to_end_raw_layouts_to_the_reference_greedy_tokens(cuda, tok, getcond, models, ctype):
    from layout_dm_amd import task

    s = sub(getcond, ctype + "_")
    cond = task.get_cond(layouts_of(s, ctype), tok, ctype, **captured(s, ctype))
    assert_cond_is_the_fixtures(cond, s, ctype)
    want = torch.from_numpy(s["greedy_tokens"].astype(np.int64))
    B = want.shape[0]
    for prec in ("exact", "split"):
        got = models[prec].model.sample(batch_size=B, cond=cond, sampling_cfg=_sampling_cfg(ctype, "deterministic"))
        diff = int((got != want).sum())
        print(f"[cond builder {ctype}] {prec}: greedy tokens differing from the reference's sample(): {diff}/{want.numel()}")
        assert diff == 0


def synth_layouts(B, seed=0, dev=None):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(1, E + 1, (B,), generator=g)
    n[:E + 1] = torch.arange(0, E + 1)               # every size, the empty layout included
    mask = torch.arange(E)[None] < n[:, None]
    wh = 0.05 + 0.4 * torch.rand((B, E, 2), generator=g)
    xy = wh / 2 + (1 - wh) * torch.rand((B, E, 2), generator=g)
    out = {"bbox": torch.cat([xy, wh], dim=-1) * mask[..., None], "label": torch.randint(0, N_CATEGORY, (B, E), generator=g) * mask,
           "mask": mask}
    return ({k: v.to(dev) for k, v in out.items()} if dev is not None else out), n


def cut(layouts, lo, hi):
    return {k: v[lo:hi] for k, v in layouts.items()}


def test_own_draws_partial(cuda, tok):
    from layout_dm_amd import task

    lay, n = synth_layouts(512, dev=cuda)
    cond = task.get_cond(lay, tok, "partial", seed=7)
    keep = cond["mask"].cpu().reshape(512, E, 5)
    assert bool((keep == keep[:, :, :1]).all())
    keep = keep[:, :, 0]
    assert not bool((keep & ~lay["mask"].cpu()).any())
    cnt = keep.sum(1)
    hi = torch.tensor([max(1, int((int(k) - 1) * 0.3)) for k in n])
    ok = torch.where(n == 0, cnt == 0, (cnt >= 1) & (cnt <= hi))
    assert bool(ok.all()), (n[~ok], cnt[~ok])
    assert len(set(cnt[n == 25].tolist())) > 1                                  # k itself is drawn
    seq = cond["seq"].cpu().reshape(512, E, 5)
    assert bool((seq[~keep] == PAD + 1).all()) and bool((seq[keep] < PAD).all())
    halves = [task.get_cond(cut(lay, lo, lo + 256), tok, "partial", seed=7, first_layout=lo) for lo in (0, 256)]
    for k in ("seq", "mask"):
        assert torch.equal(torch.cat([h[k] for h in halves]), cond[k])
    other = task.get_cond(lay, tok, "partial", seed=8)
    assert not torch.equal(other["mask"], cond["mask"])


def test_own_draws_relation(cuda, tok):
    from layout_dm_amd import task

    lay, n = synth_layouts(512, dev=cuda)
    g = task.relation_graph(lay, tok, seed=7)
    ei, ea, batch = g.edge_index.cpu(), g.edge_attr.cpu(), g.batch.cpu()
    assert torch.equal(torch.bincount(batch, minlength=512), n + 1)
    known = torch.tensor([bin(int(a) & 0b1111101110).count("1") for a in ea])
    eg = batch[ei[0]]
    per = torch.zeros(512, dtype=torch.long).index_add_(0, eg, known)
    want = torch.tensor([int(2 * ((int(k) + 1) * int(k) // 2) * 0.1) for k in n])
    assert torch.equal(per, want)
    assert bool((ea & 1).ne(0).logical_and((ea & 16).ne(0)).logical_not().all())     # no both-unknown edge
    # combinations order inside every layout: (src, dst) strictly increasing lexicographically, src < dst
    first = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(batch, minlength=512).cumsum(0)])[:-1]
    key = eg * 10000 + (ei[0] - first[eg]) * 100 + (ei[1] - first[eg])
    assert bool((ei[0] < ei[1]).all()) and bool((key[1:] > key[:-1]).all())
    assert {"edge_off", "src", "dst", "attr", "first_node", "canvas"} <= set(g.csr) and g.csr["edge_off"].is_cuda
    halves = [task.relation_graph(cut(lay, lo, lo + 256), tok, seed=7, first_layout=lo) for lo in (0, 256)]
    assert torch.equal(torch.cat([h.edge_attr for h in halves]), g.edge_attr)
    assert torch.equal(torch.cat([halves[0].edge_index, halves[1].edge_index + halves[0].y.numel()], dim=1), g.edge_index)
    other = task.relation_graph(lay, tok, seed=8)
    assert not (other.edge_index.shape == g.edge_index.shape and torch.equal(other.edge_index, g.edge_index))
    # edge_ratio is honoured
    g3 = task.relation_graph(lay, tok, seed=7, edge_ratio=0.3)
    known3 = sum(bin(int(a) & 0b1111101110).count("1") for a in g3.edge_attr.cpu())
    assert known3 == sum(int(2 * ((int(k) + 1) * int(k) // 2) * 0.3) for k in n)


def test_own_draws_refinement_noise(cuda, tok):
    from layout_dm_amd import task

    lay, _ = synth_layouts(512, dev=cuda)
    geometry = task.tokenizer_geometry(tok)
    dense = task._dense(lay, E, cuda)
    r = task.encode_cond(geometry, *dense, "refinement", seed=7, want_noise=True)
    z = r["noise"].double().cpu().reshape(-1)
    n = z.numel()
    assert n == 512 * 25 * 4 == 51200
    mean, std = float(z.mean()), float(z.std())
    print(f"[cond builder refinement] own noise over {n} draws: mean {mean:.3e}, std {std:.6f}")
    assert abs(mean) <= 5 * 0.1 / np.sqrt(n)                 # five standard errors of the mean
    assert abs(std - 0.1) <= 5 * 0.1 / np.sqrt(2 * n)        # ... and of the standard deviation
    # what was added is what was reported: feeding it back reproduces the call
    again = task.encode_cond(geometry, *dense, "refinement", noise=r["noise"])
    assert torch.equal(again["seq_orig"], r["seq_orig"]) and torch.equal(again["seq"], r["seq"])
    cond = task.get_cond(lay, tok, "refinement", seed=7)
    assert torch.equal(cond["seq_orig"], r["seq_orig"].long())
    halves = [task.get_cond(cut(lay, lo, lo + 256), tok, "refinement", seed=7, first_layout=lo) for lo in (0, 256)]
    for k in ("seq", "mask", "seq_orig", "num_element"):
        assert torch.equal(torch.cat([h[k] for h in halves]), cond[k])
    other = task.get_cond(lay, tok, "refinement", seed=8)
    assert not torch.equal(other["seq_orig"], cond["seq_orig"])
    # seed=None draws the seed from torch's global generator
    torch.manual_seed(5)
    a = task.get_cond(lay, tok, "refinement")
    torch.manual_seed(5)
    b = task.get_cond(lay, tok, "refinement")
    assert torch.equal(a["seq_orig"], b["seq_orig"]) and not torch.equal(a["seq_orig"], cond["seq_orig"])


def test_error_bits_raise(cuda, tok):
    from layout_dm_amd import task

    lay, _ = synth_layouts(32)
    bad = dict(lay, mask=lay["mask"].clone())
    bad["mask"][20, 0] = False
    with pytest.raises(ValueError, match="prefix"):
        task.get_cond(bad, tok, "c")
    bad = dict(lay, bbox=lay["bbox"].clone())
    bad["bbox"][20, 1, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        task.encode(tok, **bad)
    bad = dict(lay, label=lay["label"].clone())
    bad["label"][20, 1] = N_CATEGORY
    with pytest.raises(ValueError, match="label"):
        task.relation_graph(bad, tok, seed=1)


@pytest.mark.parametrize("ctype", ["c", "partial", "refinement", "relation"])
def test_sample_from_layouts_equals_get_cond_then_sample(cuda, tok, models, ctype):
    from layout_dm_amd import task

    lay = cut(synth_layouts(32, seed=3)[0], 3, 11)      # sizes 3 .. 10
    m = models["exact"]
    cfg = _sampling_cfg(ctype, "random")
    cfg["num_timesteps"] = 10
    cond = task.get_cond(lay, tok, ctype, seed=21)
    want = m.sample(batch_size=8, cond=cond, sampling_cfg=cfg, seed=4)
    got = m.sample_from_layouts(lay, ctype, cfg, cond_seed=21, seed=4)
    for k in ("bbox", "label", "mask"):
        assert torch.equal(got[k], want[k]), (ctype, k)
    if ctype != "partial":
        assert torch.equal(got["mask"], lay["mask"]) and torch.equal(got["label"][got["mask"]], lay["label"][lay["mask"]])


def test_relation_cond_feeds_compute_violation(cuda, tok, getcond):
    from layout_dm_amd import metrics, task

    s = sub(getcond, "relation_")
    cond = task.get_cond(layouts_of(s, "relation"), tok, "relation", **captured(s, "relation"))
    g = cond["batch_w_canvas"]
    score = metrics.compute_violation(g.x, g)             # the layouts the relations were read from break none of them
    assert score.dtype == torch.float32 and score.shape == (2,) and bool((score == 0).all())
    moved = g.x.clone()
    moved[1:, :2] = 1 - moved[1:, :2]
    assert float(metrics.compute_violation(moved, g).nan_to_num(0).sum()) > 0
    # and the graph as a reference-style dict gives the same scores
    plain = {"y": g.y, "edge_index": g.edge_index, "edge_attr": g.edge_attr, "batch": g.batch}
    assert torch.equal(metrics.compute_violation(moved, plain), metrics.compute_violation(moved, g))


def test_relation_graph_to_device_and_single_read(cuda, tok, getcond):
    from layout_dm_amd import metrics, task

    s = sub(getcond, "relation_")
    cond = task.get_cond(layouts_of(s, "relation"), tok, "relation", **captured(s, "relation"))
    g = cond["batch_w_canvas"]
    gd = g.to("cuda")
    assert gd is not g and all(getattr(gd, k).is_cuda for k in ("x", "y", "batch", "edge_index", "edge_attr")) and not g.x.is_cuda
    assert torch.equal(gd.edge_index.cpu(), g.edge_index) and gd.csr is not None and gd.to(gd.x.device) is gd
    moved = g.x.clone()
    moved[1:, :2] = 1 - moved[1:, :2]
    assert torch.equal(metrics.compute_violation(moved, gd).cpu(), metrics.compute_violation(moved, g))
    # a bad input of the encode half still raises for cond=relation, where its error word travels with the edge total
    lay = layouts_of(s, "relation")
    lay["bbox"][0, 0, 0] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        task.get_cond(lay, tok, "relation", seed=1)
