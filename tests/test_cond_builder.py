"""cond= inputs from raw layouts (layout_dm_amd/task.py, csrc/ldm_cond_core.h) — CPU side.

The host build of the kernels' one source (csrc/ldm_cond_core.h through tests/cpu_cond_check.cpp) against
tests/golden/rico25_getcond.npz, the reference's OWN get_cond results (oracle/make_golden.py getcond_cases): from the raw
x / y / batch of each case, every `seq`, `mask`, `seq_orig`-free field, `num_element`, `edge_index` (order included) and
`edge_attr` BIT FOR BIT — c, cwh, partial (keep = the reference's returned mask) and relation (selection recovered from its
edge_attr: a sampled relation is never UNKNOWN).  Linear-bin boundaries (k/32 +- 1 ulp, products k + 0.5, values < 0, > 1,
exactly 0 / 1, w / h below d; float32 and float64) are held against torch executing the statements of bbox_tokenizer.py:84-115.
Also: the documented kmeans / percentile rules, every error bit on a hand-made bad input, and the C-ABI exports."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _hostbuild as HB

N_CATEGORY, N_BIN, E = 25, 32, 25
PAD, MASK = N_CATEGORY + 4 * N_BIN, N_CATEGORY + 4 * N_BIN + 1
RULES = {"gt": 0, "c": 1, "cwh": 2, "partial": 3, "refinement": 4, "relation": 5}


@pytest.fixture(scope="module")
def host_exe():
    return HB.host_program("cpu_cond_check")


@pytest.fixture(scope="module")
def getcond(golden_dir):
    return np.load(os.path.join(golden_dir, "rico25_getcond.npz"))


def _pad8(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 8)


def host_run(exe, tmp_path, mode, bbox, label, mask, *, n_category=N_CATEGORY, n_bin=N_BIN, quant=0, rule=0, centres=None,
             keep=None, noise=None, selection=None, edge_ratio=0.1, seed=0, first_layout=0):
    B, S = label.shape
    f64 = bbox.dtype == np.float64
    payload = np.array([mode, f64, B, S, n_category, n_bin, quant, rule, keep is not None, noise is not None,
                        selection is not None, 0], np.int32).tobytes()
    payload += np.array([edge_ratio], np.float64).tobytes() + np.array([seed, first_layout], np.uint64).tobytes()
    for a, dt in ((bbox, bbox.dtype), (label, np.int64), (mask, np.uint8), (centres, np.float64), (keep, np.uint8),
                  (noise, np.float32), (selection, np.uint8)):
        if a is not None:
            payload += _pad8(np.ascontiguousarray(a, dt).tobytes())
    rc, raw = HB.run_host_io(exe, tmp_path, payload)
    assert rc == 0
    raw = np.frombuffer(raw, np.uint8)
    at = [0]

    def take(dt, n):
        size = np.dtype(dt).itemsize * n
        v = raw[at[0]:at[0] + size].view(dt)
        at[0] += size
        return v

    if mode == 0:
        n = B * S * 5
        return {"err": int(take(np.int32, 1)[0]), "seq": take(np.int32, n).reshape(B, -1), "mask": take(np.uint8, n).reshape(B, -1),
                "seq_orig": take(np.int32, n).reshape(B, -1), "num_element": take(np.int32, B)}
    err, n_edge, n_nodes = take(np.int32, 3)
    out = {"err": int(err), "edge_off": take(np.int32, B + 1), "src": take(np.int32, n_edge), "dst": take(np.int32, n_edge),
           "attr": take(np.int32, n_edge), "first_node": take(np.int64, B), "y": take(np.int64, n_nodes),
           "batch": take(np.int64, n_nodes), "x": take(bbox.dtype, 4 * n_nodes).reshape(-1, 4)}
    g = np.repeat(np.arange(B), np.diff(out["edge_off"]))
    out["edge_index"] = np.stack([out["src"] + out["first_node"][g], out["dst"] + out["first_node"][g]]).astype(np.int64)
    return out


def dense_of(x, y, batch, canvas: bool):
    """to_dense_batch (+ sparse_to_dense's remove_canvas) of a collated batch: bbox (B,E,4), label (B,E), mask (B,E)"""
    B = int(batch.max()) + 1
    bbox, label, mask = np.zeros((B, E, 4), x.dtype), np.zeros((B, E), np.int64), np.zeros((B, E), np.uint8)
    for b in range(B):
        rows = np.flatnonzero(batch == b)
        if canvas:
            rows = rows[1:]
        n = len(rows)
        bbox[b, :n], label[b, :n], mask[b, :n] = x[rows], y[rows] - (1 if canvas else 0), 1
    return bbox, label, mask


def sub(g, prefix):
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


@pytest.mark.parametrize("ctype", ["c", "cwh", "partial", "relation"])
def test_host_build_reproduces_the_reference_get_cond(host_exe, tmp_path, getcond, ctype):
    s = sub(getcond, ctype + "_")
    bbox, label, mask = dense_of(s["x"], s["y"], s["batch"], canvas=ctype == "relation")
    keep = s["cond_mask"][:, ::5] if ctype == "partial" else None
    out = host_run(host_exe, tmp_path, 0, bbox, label, mask, rule=RULES[ctype], keep=keep)
    assert out["err"] == 0
    assert np.array_equal(out["seq"], s["cond_seq"].astype(np.int32))
    assert np.array_equal(out["mask"].astype(bool), s["cond_mask"])
    if "num_element" in s:
        assert np.array_equal(out["num_element"], s["num_element"])
    # the plain encode under it: where the reference kept a token it is the encode's token
    enc = host_run(host_exe, tmp_path, 0, bbox, label, mask, rule=RULES["gt"])
    kept = s["cond_mask"] & (np.repeat(mask, 5, axis=1) != 0)
    assert kept.any() and np.array_equal(enc["seq"][kept], s["cond_seq"].astype(np.int32)[kept])
    assert np.array_equal(enc["mask"], np.repeat(mask, 5, axis=1))


def test_host_build_reproduces_the_reference_relation_graph(host_exe, tmp_path, getcond):
    from layout_dm_amd.task import selection_from_edges

    s = sub(getcond, "relation_")
    bbox, label, mask = dense_of(s["x"], s["y"], s["batch"], canvas=True)
    B = len(bbox)
    sel = selection_from_edges(s["edge_index"], s["edge_attr"], s["batch"], B, E).numpy()
    assert sel.sum() == sum(bin(int(a) & 0b1111101110).count("1") for a in s["edge_attr"])
    out = host_run(host_exe, tmp_path, 1, bbox, label, mask, selection=sel)
    assert out["err"] == 0
    assert np.array_equal(out["edge_index"], s["edge_index"])        # order included
    assert np.array_equal(out["attr"].astype(np.int64), s["edge_attr"])
    assert np.array_equal(out["y"], s["y"]) and np.array_equal(out["batch"], s["batch"])
    assert out["x"].dtype == s["x"].dtype and np.array_equal(out["x"], s["x"])


def boundary_boxes(T):
    """(M,4) boxes in T whose four coordinates each sweep the linear bins' boundaries"""
    T = np.dtype(T).type
    d = T(1.0 / N_BIN)
    vals = []
    for k in range(N_BIN + 1):
        v = T(k / N_BIN)
        vals += [v, np.nextafter(v, T(2)), np.nextafter(v, T(-1))]
        h = T((k + 0.5) / N_BIN)                       # N * q = k + 0.5: round half to even
        vals += [h, np.nextafter(h, T(2)), np.nextafter(h, T(-1)), T(h + d)]
    vals += [T(-0.5), T(-1e-9), T(0.0), T(1.0), T(1.5), T(1e9), T(d / 2), T(d / 3), np.nextafter(d, T(-1)), T(1 - d), T(1e-30)]
    v = np.asarray(vals, T)
    return np.stack([v, v[::-1], np.roll(v, 7), np.roll(v[::-1], 3)], axis=1)


def torch_linear_encode(bbox):
    """bbox_tokenizer.py:84-115 for linear bins + the stacked x-y-w-h offsets, statement for statement, run by torch"""
    d = 1 / N_BIN
    q = torch.zeros_like(bbox)
    q[..., :2] = torch.clamp(bbox[..., :2], 0.0, 1.0 - d)
    q[..., 2:] = torch.clamp(bbox[..., 2:], d, 1.0) - d
    idx = (N_BIN * q).round().long()
    for k in range(4):
        idx[..., k] += N_BIN * k
    return idx + N_CATEGORY


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_linear_bin_boundaries_follow_torch(host_exe, tmp_path, T):
    boxes = boundary_boxes(T)
    M = len(boxes)
    B = (M + E - 1) // E
    bbox = np.zeros((B * E, 4), T)
    bbox[:M] = boxes
    bbox = bbox.reshape(B, E, 4)
    mask = np.zeros(B * E, np.uint8)
    mask[:M] = 1
    mask = mask.reshape(B, E)
    label = (np.arange(B * E) % N_CATEGORY).reshape(B, E)
    out = host_run(host_exe, tmp_path, 0, bbox, label, mask)
    want = torch_linear_encode(torch.from_numpy(bbox)).numpy()
    got = out["seq"].reshape(B, E, 5)
    valid = mask != 0
    assert out["err"] == 0 and np.array_equal(got[valid][:, 1:], want[valid])
    assert np.array_equal(got[valid][:, 0], label[valid]) and (got[~valid] == PAD).all()
    bins = got[valid][:, 1:] - N_CATEGORY - N_BIN * np.arange(4)
    assert bins.min() == 0 and bins.max() == N_BIN - 1 and len(np.unique(bins)) == N_BIN
    # the half-way products are there, and half goes to even: x = 2.5 / 32 -> bin 2, 3.5 / 32 -> bin 4
    x = bbox[valid][:, 0]
    for k, b in ((2, 2), (3, 4)):
        hit = x == T((k + 0.5) / N_BIN)
        assert hit.any() and (bins[hit, 0] == b).all()


def test_refinement_rule_and_noise_sum(host_exe, tmp_path, getcond):
    """seq_orig = encode(bbox + noise) in the boxes' dtype; mask = valid & (attr == 0) | ~valid; seq = where(mask, seq_orig,
    mask_id), pad on padding (task.py:126-138) — against torch running those statements on the fixture's refinement layouts."""
    s = sub(getcond, "refinement_")
    bbox, label, mask = dense_of(s["x"], s["y"], s["batch"], canvas=False)
    noise = torch.normal(0, 0.1, size=bbox.shape, generator=torch.Generator().manual_seed(3)).numpy()
    for T in (np.float32, np.float64):
        b = bbox.astype(T)
        out = host_run(host_exe, tmp_path, 0, b, label, mask, rule=RULES["refinement"], noise=noise)
        new = torch.from_numpy(b) + torch.from_numpy(noise)
        assert new.dtype == torch.from_numpy(b).dtype
        valid = torch.from_numpy(mask != 0)
        tok = torch.cat([torch.from_numpy(label)[..., None], torch_linear_encode(new)], dim=-1)
        tok[~valid] = PAD
        orig = tok.reshape(len(b), -1)
        v5 = valid.repeat_interleave(5, dim=1)
        m = v5 & (torch.arange(5 * E) % 5 == 0) | ~v5
        seq = torch.where(m, orig, torch.tensor(MASK))
        seq = torch.where(v5, seq, torch.tensor(PAD))
        assert out["err"] == 0 and np.array_equal(out["seq_orig"], orig.numpy()) and np.array_equal(out["seq"], seq.numpy())
        assert np.array_equal(out["mask"].astype(bool), m.numpy()) and np.array_equal(out["num_element"], s["num_element"])
    # with zero noise the kept category tokens are the reference's own
    out = host_run(host_exe, tmp_path, 0, bbox, label, mask, rule=RULES["refinement"], noise=np.zeros_like(noise))
    assert np.array_equal(out["mask"].astype(bool), s["cond_mask"])
    assert np.array_equal(out["seq"][:, ::5], s["cond_seq"].astype(np.int32)[:, ::5])


def test_kmeans_and_percentile_rules(host_exe, tmp_path):
    rng = np.random.default_rng(5)
    centres = np.sort(rng.random((4, N_BIN)), axis=1)
    centres32 = centres.astype(np.float32).astype(np.float64)
    M = 40 * E
    x = rng.random((M, 4)).astype(np.float32)
    mid = ((centres32[:, :-1] + centres32[:, 1:]) / 2).astype(np.float32)          # set B: midpoints +- {0, 1, 2} ulp
    for k in range(4):
        m = np.tile(mid[k], 5)[:M // 2]
        for u in range(5):
            step = u - 2
            v = m[u::5].copy()
            for _ in range(abs(step)):
                v = np.nextafter(v, np.float32(2 if step > 0 else -1))
            m[u::5] = v
        x[:len(m), k] = m
    x[-1] = [-0.25, 1.25, 0.0, 1.0]
    bbox = x.reshape(-1, E, 4)
    B = len(bbox)
    label, mask = np.zeros((B, E), np.int64), np.ones((B, E), np.uint8)
    for quant, cs in ((2, centres32), (1, centres32)):
        for T in (np.float32, np.float64):
            out = host_run(host_exe, tmp_path, 0, bbox.astype(T), label, mask, quant=quant, centres=cs)
            got = out["seq"].reshape(-1, 5)[:, 1:] - N_CATEGORY - N_BIN * np.arange(4)
            for k in range(4):
                v = x[:, k]
                if quant == 2:     # |float32(x) - c| in float64, lowest index on a tie
                    want = np.argmin(np.abs(v.astype(np.float64)[:, None] - cs[k][None]), axis=1)
                else:              # clustering.py:43-55: clip, float32 distances, first minimum
                    want = np.argmin(np.fabs(cs[k].astype(np.float32)[:, None] - v.clip(0.0, 1.0)[None]), axis=0)
                assert np.array_equal(got[:, k], want), (quant, T, k)
                near = np.abs(got[:, k] - np.searchsorted(cs[k], v.astype(np.float64))).max()
                assert near <= 1      # one of the two neighbouring centres
            assert out["err"] == 0


def test_percentile_sentinel_centres_are_part_of_the_search(host_exe, tmp_path):
    cs = np.tile(np.r_[np.full(4, -1.0), np.linspace(0.1, 0.9, N_BIN - 4)], (4, 1))    # sorted, -1 = "will not be queried"
    bbox = np.zeros((1, E, 4), np.float32)
    bbox[0, 0] = [0.0, 0.01, 0.1, 1.0]
    out = host_run(host_exe, tmp_path, 0, bbox, np.zeros((1, E), np.int64), np.ones((1, E), np.uint8), quant=1, centres=cs)
    got = out["seq"].reshape(-1, 5)[0, 1:] - N_CATEGORY - N_BIN * np.arange(4)
    assert got.tolist() == [4, 4, 4, N_BIN - 1]      # |-1 - 0| = 1 loses against |0.1 - 0|


def test_every_error_bit_fires(host_exe, tmp_path):
    bbox = np.full((2, E, 4), 0.5, np.float32)
    label = np.zeros((2, E), np.int64)
    mask = np.zeros((2, E), np.uint8)
    mask[:, :3] = 1
    run = lambda mode, b=bbox, l=label, m=mask: host_run(host_exe, tmp_path, mode, b, l, m,
                                                        selection=np.ones((2, 2, E + 1, E + 1), np.uint8) if mode else None)["err"]
    hole = mask.copy()
    hole[1, 1] = 0
    nan, inf = bbox.copy(), bbox.copy()
    nan[0, 2, 1], inf[1, 0, 3] = np.nan, np.inf
    lab_hi, lab_lo = label.copy(), label.copy()
    lab_hi[0, 1], lab_lo[1, 2] = N_CATEGORY, -1
    pad_junk = bbox.copy()
    pad_junk[0, 5] = np.nan        # padding slots are not looked at
    lab_pad = label.copy()
    lab_pad[0, 7] = 99
    for mode in (0, 1):
        assert run(mode) == 0
        assert run(mode, m=hole) == 1
        assert run(mode, b=nan) == 2 and run(mode, b=inf) == 2
        assert run(mode, l=lab_hi) == 4 and run(mode, l=lab_lo) == 4
        assert run(mode, b=nan, l=lab_hi, m=hole) == 7
        assert run(mode, b=pad_junk, l=lab_pad) == 0


def test_zero_element_layout(host_exe, tmp_path):
    bbox, label, mask = np.zeros((1, E, 4), np.float32), np.zeros((1, E), np.int64), np.zeros((1, E), np.uint8)
    for rule in ("gt", "c", "cwh", "refinement", "relation"):
        out = host_run(host_exe, tmp_path, 0, bbox, label, mask, rule=RULES[rule], noise=np.zeros((1, E, 4), np.float32))
        assert out["err"] == 0 and (out["seq"] == PAD).all() and out["num_element"].tolist() == [0]
        assert (out["mask"] == (0 if rule == "gt" else 1)).all()
    g = host_run(host_exe, tmp_path, 1, bbox, label, mask)
    assert g["edge_off"].tolist() == [0, 0] and g["y"].tolist() == [0] and g["x"].tolist() == [[0.5, 0.5, 1.0, 1.0]]


def test_host_own_draws_have_the_reference_counts(host_exe, tmp_path):
    """exact counts of the own draws (the statistics and the cut-invariance are GPU tests)"""
    rng = np.random.default_rng(1)
    B = 64
    n = np.r_[np.arange(0, 26), rng.integers(1, 26, B - 26)]
    mask = (np.arange(E)[None] < n[:, None]).astype(np.uint8)
    bbox = rng.random((B, E, 4)).astype(np.float32)
    label = rng.integers(0, N_CATEGORY, (B, E))
    out = host_run(host_exe, tmp_path, 0, bbox, label, mask, rule=RULES["partial"], seed=11)
    keep = out["mask"].reshape(B, E, 5)
    assert (keep == keep[:, :, :1]).all() and not (keep[:, :, 0] & (mask == 0)).any()
    cnt = keep[:, :, 0].sum(1)
    for b in range(B):
        hi = max(1, int((n[b] - 1) * 0.3))
        assert (cnt[b] == 0) if n[b] == 0 else (1 <= cnt[b] <= hi), (b, n[b], cnt[b])
    g = host_run(host_exe, tmp_path, 1, bbox, label, mask, seed=11)
    known = np.array([bin(int(a) & 0b1111101110).count("1") for a in g["attr"]])
    per = np.add.reduceat(np.r_[known, 0], g["edge_off"][:-1]) * (np.diff(g["edge_off"]) > 0)
    for b in range(B):
        N = n[b] + 1
        assert per[b] == int(2 * (N * (N - 1) // 2) * 0.1), (b, n[b], per[b])
    other = host_run(host_exe, tmp_path, 1, bbox, label, mask, seed=12)
    assert not np.array_equal(other["edge_index"], g["edge_index"])


def test_host_build_under_address_and_undefined_sanitizers(tmp_path, getcond):
    """every host-build case above on the ASan + UBSan build: the program reads its arrays from one exact-size buffer, and the
    graph builder fills per-layout arrays of n_pairs entries by pair_of's index arithmetic"""
    exe = HB.host_program("cpu_cond_check", sanitize=True)
    for ctype in ("c", "cwh", "partial", "relation"):
        test_host_build_reproduces_the_reference_get_cond(exe, tmp_path, getcond, ctype)
    test_host_build_reproduces_the_reference_relation_graph(exe, tmp_path, getcond)
    for T in (np.float32, np.float64):
        test_linear_bin_boundaries_follow_torch(exe, tmp_path, T)
    test_refinement_rule_and_noise_sum(exe, tmp_path, getcond)
    test_kmeans_and_percentile_rules(exe, tmp_path)
    test_percentile_sentinel_centres_are_part_of_the_search(exe, tmp_path)
    test_every_error_bit_fires(exe, tmp_path)
    test_zero_element_layout(exe, tmp_path)
    test_host_own_draws_have_the_reference_counts(exe, tmp_path)


def test_exports_and_bad_arguments():
    from layout_dm_amd import binding, build

    for name in ("ldm_encode_cond", "ldm_relation_graph"):
        assert name in binding.EXPORTS
    assert binding.ABI_VERSION == 5
    assert "kernels_cond.hip" in build.SOURCES
    lib = C.CDLL(build.build(verbose=False))
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    lib.ldm_encode_cond.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]
    lib.ldm_relation_graph.argtypes = [vp, i32, vp, vp, i32, i32, i32, vp, C.c_double, u64, u64] + [vp] * 13
    d = C.c_void_p(64)   # never dereferenced: every call below is refused before it touches memory or launches

    def enc(bbox=d, f64=0, label=d, mask=d, B=2, E=25, ncat=25, nbin=32, quant=0, centres=None, rule=1, keep=None, noise=None,
            seq=d, cm=d, orig=None, num=None, nz=None, err=d):
        return lib.ldm_encode_cond(bbox, f64, label, mask, B, E, ncat, nbin, quant, centres, rule, keep, noise, 0, 0, seq, cm, orig,
                                   num, nz, err, None)

    for bad in ({"bbox": None}, {"label": None}, {"mask": None}, {"seq": None}, {"cm": None}, {"err": None}, {"f64": 2}, {"B": -1},
                {"E": 0}, {"E": 33}, {"ncat": 0}, {"nbin": 0}, {"nbin": 129}, {"quant": 3}, {"quant": 1}, {"centres": d},
                {"rule": 6}, {"rule": -1}, {"rule": 4}, {"bbox": C.c_void_p(8)}, {"noise": C.c_void_p(4)}):
        assert enc(**bad) == -1, bad

    def graph(bbox=d, f64=0, label=d, mask=d, B=2, E=25, ncat=25, ratio=0.1, err=d, **null):
        out = [None if null.get(k) else d for k in ("work", "off", "src", "dst", "attr", "first", "x", "y", "batch", "canvas", "totals")]
        return lib.ldm_relation_graph(bbox, f64, label, mask, B, E, ncat, None, ratio, 0, 0, *out, err, None)

    for bad in ({"bbox": None}, {"label": None}, {"mask": None}, {"err": None}, {"f64": -1}, {"B": 0}, {"E": 40}, {"ncat": 0},
                {"ratio": -0.1}, {"ratio": 1.5}, {"ratio": float("nan")}, {"work": 1}, {"off": 1}, {"src": 1}, {"dst": 1},
                {"attr": 1}, {"first": 1}, {"x": 1}, {"y": 1}, {"batch": 1}, {"canvas": 1}, {"totals": 1}):
        assert graph(**bad) == -1, bad


def test_python_api_and_no_silent_cpu_path():
    from _stub_tokenizer import StubTokenizer
    from oracle import spec as SP

    from layout_dm_amd import task
    from layout_dm_amd.layoutdm import LayoutDM

    assert callable(task.encode) and callable(task.get_cond) and callable(LayoutDM.sample_from_layouts) and callable(LayoutDM.encode)
    tok = StubTokenizer(SP.RICO25)
    assert task.tokenizer_geometry(tok) == (25, 32, 25, "linear", None)
    layouts = {"bbox": torch.rand(2, 25, 4), "label": torch.zeros(2, 25, dtype=torch.long), "mask": torch.ones(2, 25, dtype=torch.bool)}
    with pytest.raises(NotImplementedError, match="random"):
        task.get_cond(layouts, tok, "random")
    with pytest.raises(ValueError):
        task.get_cond(layouts, tok, "nonsense")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            task.get_cond(layouts, tok, "c")
        with pytest.raises(RuntimeError, match="no CPU path"):
            task.encode(tok, layouts["bbox"], layouts["label"], layouts["mask"])


def test_relation_graph_object_is_read_only_and_moves():
    from layout_dm_amd.task import RelationGraph

    csr = {"edge_off": torch.tensor([0, 1], dtype=torch.int32), "src": torch.tensor([0], dtype=torch.int32)}
    g = RelationGraph(torch.rand(2, 4), torch.tensor([0, 3]), torch.tensor([0, 0]), torch.tensor([[0], [1]]), torch.tensor([4 | 1 << 2]),
                      1, csr)
    assert g.num_graphs == 1 and bool(g.attr["has_canvas_element"].all()) and g.csr["edge_off"].tolist() == [0, 1]
    for name in ("x", "y", "batch", "edge_index", "edge_attr", "csr", "attr"):
        with pytest.raises(AttributeError):
            setattr(g, name, None)
    assert g.to("cpu") is g and g.to(torch.device("cpu")) is g
    moved = g.to("meta")
    assert moved is not g and all(getattr(moved, k).device.type == "meta" for k in ("x", "y", "batch", "edge_index", "edge_attr"))
    assert moved.csr["edge_off"].device.type == "cpu" and g.x.device.type == "cpu"
