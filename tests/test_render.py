"""Layouts as pictures (convert_layout_to_image / save_image, trainer/helpers/visualization.py:17-115) — CPU side.

The host build of the kernel's one source (csrc/ldm_render_core.h, through tests/cpu_render_check.cpp) against
tests/golden/render/reference.npz, which tools/make_render_golden.py writes from the reference's own convert_layout_to_image
(Pillow's ImageDraw on 0-dim torch scalars): every pixel of every layout BYTE FOR BYTE, float32 and float64, every hand-made
row.  No tolerance: the drawing is integer arithmetic on truncated coordinates.  Also: the mosaic the host path assembles
against a numpy assembly of the fixture's images under make_grid's documented rule, the error word, the hand-made inputs
reproducible without the reference and hitting what they aim at, the fixture regenerating bit for bit where the reference
is importable, the C-ABI exports refusing bad arguments, the kernel's resource report (no scratch), and the Python module
raising without a GPU."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _hostbuild as HB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("make_render_golden", os.path.join(ROOT, "tools", "make_render_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()
SETS = list(G.SETS)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "render", "reference.npz"))


@pytest.fixture(scope="module")
def host_exe():
    return HB.host_program("cpu_render_check")


def host_run(exe, tmp_path, bbox, label, mask, colors, canvas, cols=1, pad=0):
    """-> (exit code, error word, (GH,GW,3) uint8)"""
    B, S = mask.shape
    H, W = (int(v) for v in canvas)
    payload = np.array([bbox.dtype == np.float64, B, S, len(colors), H, W, cols, pad], np.int32).tobytes()
    for a, dt in ((bbox, bbox.dtype), (label, np.int64), (mask, np.uint8), (colors, np.uint8)):
        payload += np.ascontiguousarray(a, dt).tobytes()
    rc, raw = HB.run_host_io(exe, tmp_path, payload)
    if rc != 0:
        return rc, None, None
    raw = np.frombuffer(raw, np.uint8)
    GH, GW = mosaic_shape(B, H, W, cols, pad)
    return rc, int(raw[:4].view(np.int32)[0]), raw[4:].reshape(GH, GW, 3)


def mosaic_shape(B, H, W, cols, pad):
    """torchvision.utils.make_grid as documented: xmaps = min(nrow, B) columns, ceil(B / xmaps) rows of (H + pad, W + pad)
    cells plus one more pad at the bottom and the right"""
    rows = -(-B // cols)
    return rows * (H + pad) + pad, cols * (W + pad) + pad


def numpy_mosaic(images, nrow, pad):
    """make_grid(images, nrow, padding=pad, pad_value=0) in numpy, channels last"""
    B, H, W, _ = images.shape
    cols = min(nrow, B)
    GH, GW = mosaic_shape(B, H, W, cols, pad)
    grid = np.zeros((GH, GW, 3), np.uint8)
    for k in range(B):
        y, x = (k // cols) * (H + pad) + pad, (k % cols) * (W + pad) + pad
        grid[y:y + H, x:x + W] = images[k]
    return grid, cols


def first_difference(got, want, names=None):
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    k, y, x, c = bad[0]
    return {"layouts": np.unique(bad[:, 0])[:8].tolist(), "first": (int(k), int(y), int(x), int(c)),
            "got": int(got[k, y, x, c]), "want": int(want[k, y, x, c]), "row": names[k] if names is not None else None}


@pytest.mark.parametrize("name", SETS)
def test_host_build_equals_the_reference_byte_for_byte(host_exe, tmp_path, fx, name):
    bbox, label, mask = G.load_inputs(fx)[name]
    p, canvas = G.SETS[name]
    assert bbox.dtype == G.DTYPE[p] and tuple(fx[f"{name}_canvas"]) == canvas
    want = fx[f"{name}_image"]
    rc, err, got = host_run(host_exe, tmp_path, bbox, label, mask, fx["colors"], canvas)
    assert rc == 0 and err == 0
    got = got.reshape(want.shape)
    names = list(fx["hand_rows"]) if name.startswith("hand") else None
    assert first_difference(got, want, names) is None, (name, first_difference(got, want, names))


def test_host_mosaic_equals_numpy_assembly_of_the_fixture_images(host_exe, tmp_path, fx):
    bbox, label, mask = G.load_inputs(fx)["rand_f32"]
    images = fx["rand_f32_image"]
    for B, nrow, pad in ((1, 1, 2), (3, 2, 2), (70, 9, 2), (70, 9, 0), (5, 8, 3), (7, 1, 1)):
        want, cols = numpy_mosaic(images[:B], nrow, pad)
        rc, err, got = host_run(host_exe, tmp_path, bbox[:B], label[:B], mask[:B], fx["colors"], (60, 40), cols, pad)
        assert rc == 0 and err == 0 and got.shape == want.shape, (B, nrow, pad)
        assert np.array_equal(got, want), (B, nrow, pad)
    want, _ = numpy_mosaic(images[:70], 9, 2)
    assert want.shape == (8 * 62 + 2, 9 * 42 + 2, 3) and not want[7 * 62 + 2:, 7 * 42 + 2:].any()   # 2 empty tiles stay black


def bad_batch(fx, dtype=np.float32):
    """six layouts of the fixture; layout 1 gets a NaN box, layout 3 a negative width, layout 4 a label without a colour"""
    bbox, label, mask = (a[:6].copy() for a in G.load_inputs(fx)["rand_f32"])
    bbox = bbox.astype(dtype)
    for b in (1, 3, 4):
        assert mask[b, 0] and mask[b].sum() >= 2
    return bbox, label, mask


def drop_first(images_of, bbox, label, mask, b):
    """what the picture of layout b is without its element 0"""
    m = mask.copy()
    m[b, 0] = False
    return images_of(bbox[b:b + 1], label[b:b + 1], m[b:b + 1])[0]   # (rubbish under the mask is not read)


def test_host_error_word_and_what_is_still_drawn(host_exe, tmp_path, fx):
    colors = fx["colors"]
    images = fx["rand_f32_image"]

    def images_of(bbox, label, mask):
        rc, err, got = host_run(host_exe, tmp_path, bbox, label, mask, colors, (60, 40))
        assert rc == 0
        return got.reshape(len(mask), 60, 40, 3)

    for what, word in (("nan", 1), ("inf", 1), ("negative_w", 1), ("negative_h", 1), ("label_high", 2), ("label_negative", 2)):
        bbox, label, mask = bad_batch(fx)
        b = {"nan": 1, "inf": 1, "negative_w": 3, "negative_h": 3, "label_high": 4, "label_negative": 4}[what]
        if what == "nan":
            bbox[b, 0, 1] = np.nan
        elif what == "inf":
            bbox[b, 0, 2] = np.inf
        elif what == "negative_w":
            bbox[b, 0, 2] = -0.25
        elif what == "negative_h":
            bbox[b, 0, 3] = -np.float32(1e-30)
        elif what == "label_high":
            label[b, 0] = len(colors)
        else:
            label[b, 0] = -1
        rc, err, got = host_run(host_exe, tmp_path, bbox, label, mask, colors, (60, 40))
        assert rc == 0 and err == word, (what, rc, err)
        got = got.reshape(6, 60, 40, 3)
        good = [k for k in range(6) if k != b]
        assert np.array_equal(got[good], images[good]), what                      # the other layouts are untouched
        assert np.array_equal(got[b], drop_first(images_of, bbox, label, mask, b)), what   # the bad element alone is missing
    # -0.0 is not negative, and rubbish under the mask is never an error (the fixture's masked rows hold NaN and label 999)
    bbox, label, mask = bad_batch(fx)
    bbox[0, 0, 2] = -0.0
    assert host_run(host_exe, tmp_path, bbox, label, mask, colors, (60, 40))[1] == 0
    # beyond the limits: refused
    z = np.zeros
    assert host_run(host_exe, tmp_path, z((1, 257, 4), np.float32), z((1, 257), np.int64), z((1, 257), bool), colors, (60, 40))[0] == 2
    assert host_run(host_exe, tmp_path, z((1, 2, 4), np.float32), z((1, 2), np.int64), z((1, 2), bool), colors, (0, 40))[0] == 2


def test_host_build_under_address_and_undefined_sanitizers(tmp_path, fx):
    """every host-build case above on the ASan + UBSan build: rank_of places each drawn element in exact-size arrays of S slots,
    and every pixel is written through tile_origin's index into an exact-size mosaic"""
    exe = HB.host_program("cpu_render_check", sanitize=True)
    for name in SETS:
        test_host_build_equals_the_reference_byte_for_byte(exe, tmp_path, fx, name)
    test_host_mosaic_equals_numpy_assembly_of_the_fixture_images(exe, tmp_path, fx)
    test_host_error_word_and_what_is_still_drawn(exe, tmp_path, fx)


def test_handmade_inputs_are_reproducible_and_hit_what_they_aim_at(fx):
    inp = G.inputs()
    loaded = G.load_inputs(fx)
    for name in SETS:
        for a, b in zip(inp[name], loaded[name]):
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name
    assert np.array_equal(G.colors(), fx["colors"]) and list(fx["hand_rows"]) == G.HAND_ROWS
    rows = {n: i for i, n in enumerate(G.HAND_ROWS)}
    white = np.full(3, 255, np.uint8)
    for p in ("f32", "f64"):
        img, (bbox, label, mask) = fx[f"hand_{p}_image"], loaded[f"hand_{p}"]
        T = G.DTYPE[p]
        colors = fx["colors"]
        # a zero-height box paints row Y1 and, at its two columns only, row Y1 + 1 (Pillow's outline range)
        im = img[rows["zero_height_inside"]]
        c = colors[2]
        y = int(T(0.5) * T(59))
        x1, x2 = int((T(0.5) - T(0.3) / T(2)) * T(39)), int((T(0.5) + T(0.3) / T(2)) * T(39))
        assert (im[y, x1:x2 + 1] == c).all() and (im[y + 1, [x1, x2]] == c).all() and (im[y + 1, x1 + 1:x2] == white).all()
        assert (im[y - 1] == white).all() and (im[y + 2] == white).all()
        # at the bottom edge that extra row falls off the canvas; a point box in a corner is one pixel (plus the one below)
        im = img[rows["zero_height_bottom_edge"]]
        assert (im[59] != white).any() and (im[:59] == white).all()
        im = img[rows["zero_both_corners"]]
        assert (im[0, 0] == colors[8]).all() and (im[1, 0] == colors[8]).all() and (im[59, 39] == colors[9]).all()
        assert int((im != white).any(-1).sum()) == 6   # two corners at the top paint two rows, the two at the bottom one
        # equal areas: the six orders give more than one picture (element order decides), and each is the stable order
        eq = [img[rows[f"equal_area_order_{i}"]] for i in range(6)]
        assert len({e.tobytes() for e in eq}) > 1
        b = bbox[rows["equal_area_order_0"]]
        assert len({(T(r[2]) * T(r[3])) for r in b[:3]}) == 1
        # the canvas-sized box listed third is drawn first: its outline survives only on the canvas border
        im = img[rows["canvas_box_under_smaller"]]
        assert (im[0] == colors[17]).all() and (im[:, 0] == colors[17]).all() and (im[59] == colors[17]).all()
        # the all-masked layout is white, and the masked rubbish of the holes row is not drawn
        assert (img[rows["all_masked"]] == 255).all() and np.isnan(bbox[rows["all_masked"]]).all()
        assert np.isnan(bbox[rows["mask_with_holes"]][~mask[rows["mask_with_holes"]]]).all()
        assert {0, G.N_COLORS - 1} <= set(label[mask].tolist())
        # pixel boundaries: the picture changes between the value below the whole number and the value at it
        for axis, ks in (("x", (7, 20, 39)), ("y", (11, 30, 59))):
            for k in ks:
                trio = [img[rows[f"boundary_{axis}{k}_{t}"]] for t in ("dn", "at", "up")]
                assert not np.array_equal(trio[0], trio[1]), (p, axis, k)
    for name in SETS:
        assert (fx[f"{name}_image"] != 255).any()
    n50 = loaded["s50_f32"][2].sum(1)
    assert n50.min() >= 10 and n50.max() > 32 and loaded["s50_f32"][2].shape[1] == 50


def test_fixture_regenerates_from_reference(fx):
    import PIL

    from oracle import ref_harness as rh

    if not rh.reference_importable():
        pytest.skip("neither the reference tree nor oracle/_ref/ present")
    if PIL.__version__ != str(fx["pillow_version"]):
        pytest.skip(f"the fixture was drawn by Pillow {fx['pillow_version']}, this is {PIL.__version__}")
    out = G.compute(G.inputs())
    assert set(out) == set(fx.files)
    for k, v in out.items():
        v = np.asarray(v)
        assert v.dtype == fx[k].dtype and np.array_equal(v, fx[k], equal_nan=v.dtype.kind == "f"), k


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "render", "reference.npz")) < 1 << 20


def test_cabi_exports_and_refuses_bad_arguments():
    from layout_dm_amd import binding, build

    for name in ("ldm_render_layouts", "ldm_render_grid_shape"):
        assert name in binding.EXPORTS
    assert binding.ABI_VERSION == 5
    lib = C.CDLL(build.build(verbose=False))
    vp, i32 = C.c_void_p, C.c_int
    lib.ldm_render_layouts.argtypes = [vp, i32, vp, vp, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ldm_render_grid_shape.argtypes = [i32, i32, i32, i32, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    d = C.c_void_p(16)   # never dereferenced: every call below is refused before it touches memory or launches

    def call(bbox=d, f64=0, label=d, mask=d, B=4, S=25, colors=d, n_colors=25, H=60, W=40, cols=2, pad=2, out=d, err=d):
        return lib.ldm_render_layouts(bbox, f64, label, mask, B, S, colors, n_colors, H, W, cols, pad, out, err, None)

    for bad in ({"bbox": None}, {"label": None}, {"mask": None}, {"colors": None}, {"out": None}, {"err": None}, {"f64": 2},
                {"B": 0}, {"B": -1}, {"S": 0}, {"S": 257}, {"n_colors": 0}, {"H": 0}, {"W": 0}, {"H": (1 << 14) + 1},
                {"W": (1 << 14) + 1}, {"cols": 0}, {"pad": -1}, {"pad": (1 << 14) + 1}):
        assert call(**bad) == -1, bad
    gh, gw = C.c_int64(), C.c_int64()
    for (B, H, W, cols, pad), want in (((70, 60, 40, 9, 2), (8 * 62 + 2, 9 * 42 + 2)), ((3, 60, 40, 2, 2), (126, 86)),
                                       ((5, 60, 40, 1, 0), (300, 40)), ((1, 1, 1, 1, 0), (1, 1)), ((4, 7, 5, 4, 3), (13, 35))):
        assert lib.ldm_render_grid_shape(B, H, W, cols, pad, C.byref(gh), C.byref(gw)) == 0
        assert (gh.value, gw.value) == want == mosaic_shape(B, H, W, cols, pad)
    assert lib.ldm_render_grid_shape(0, 60, 40, 1, 0, C.byref(gh), C.byref(gw)) == -1
    assert lib.ldm_render_grid_shape(1, 60, 40, 1, 0, None, C.byref(gw)) == -1


def test_render_kernels_use_no_scratch():
    """from the compiler's resource report (what tools/kernel_resources.py prints): both instances of render_layouts_k, no
    scratch, no spills, and the LDS of the ranked list only"""
    _, out, _ = HB.kernel_asm("kernels_render.hip", resource_report=True)
    blocks = re.split(r"Function Name: ", out)[1:]
    seen = 0
    for blk in blocks:
        if "render_layouts_k" not in blk.split()[0]:
            continue
        seen += 1
        get = lambda pat: int(re.search(pat, blk).group(1))   # noqa: E731
        assert get(r"ScratchSize \[bytes/lane\]: (\d+)") == 0, blk
        assert get(r"VGPRs? Spill: (\d+)") == 0 and get(r"SGPRs? Spill: (\d+)") == 0, blk
        assert get(r"LDS Size \[bytes/block\]: (\d+)") <= 8192, blk   # 256 slots x (area 8 + flag 1 + rectangle 16 + colour 4) + alignment
    assert seen == 2


def test_python_api_and_no_silent_cpu_path(fx, monkeypatch):
    from layout_dm_amd import visualization as V

    for name in ("render_layouts", "render_grid", "save_image", "render_trajectory", "save_gif", "default_colors", "grid_shape"):
        assert callable(getattr(V, name))
    pal = V.default_colors(25)
    assert pal == V.default_colors(25) and len(set(pal)) == 25 and all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in pal)
    assert V.default_colors(5) == pal[:5] and "NOT the reference's" in V.default_colors.__doc__
    assert V.grid_shape(70, (60, 40), 9) == (8 * 62 + 2, 9 * 42 + 2, 9) and V.grid_shape(3) == (126, 86, 2)
    assert V.grid_shape(2, (60, 40), 8) == (64, 86, 2)          # make_grid: no more columns than tiles
    bbox, label, mask = (torch.from_numpy(a) for a in G.load_inputs(fx)["hand_f32"])
    # what is not drawn on the device says so before anything else happens
    with pytest.raises(NotImplementedError, match="draw_label"):
        V.save_image(bbox, label, mask, fx["colors"], draw_label=True, names=["a"])
    with pytest.raises(NotImplementedError, match="batch_resources"):
        V.save_image(bbox, label, mask, fx["colors"], batch_resources={"img_bg": [None]})
    if torch.cuda.is_available():
        got = V.render_layouts(bbox, label, mask, fx["colors"])
        assert np.array_equal(got.cpu().numpy(), fx["hand_f32_image"])
    else:
        for call in (lambda: V.render_layouts(bbox, label, mask, fx["colors"]),
                     lambda: V.render_grid(bbox, label, mask, fx["colors"]),
                     lambda: V.save_image(bbox, label, mask, fx["colors"], names=["dropped"]),
                     lambda: V.save_image(bbox, label, mask, fx["colors"], use_grid=True)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
    # the runners' switch: off by default, "1" -> <result_dir>/test_generated.png, anything else is the path
    monkeypatch.delenv(V.VIS_ENV, raising=False)
    assert V.vis_path("/r/x") is None and V.save_first_batch(None, "/r/x", 25) is None
    monkeypatch.setenv(V.VIS_ENV, "")
    assert V.vis_path("/r/x") is None
    monkeypatch.setenv(V.VIS_ENV, "1")
    assert V.vis_path("/r/x") == os.path.join("/r/x", "test_generated.png")
    monkeypatch.setenv(V.VIS_ENV, "/elsewhere/pic.png")
    assert V.vis_path("/r/x") == "/elsewhere/pic.png"


def test_save_gif_writes_the_frames_with_the_reference_parameters(tmp_path):
    from PIL import Image

    from layout_dm_amd import visualization as V

    rng = np.random.default_rng(0)
    frames = np.zeros((4, 12, 10, 3), np.uint8)
    for t in range(4):
        frames[t, t:t + 4] = rng.integers(0, 256, 3)       # flat colour bands: GIF's palette holds them exactly
    path = tmp_path / "traj.gif"
    V.save_gif(torch.from_numpy(frames), path)
    with Image.open(path) as im:
        assert im.n_frames == 4 and im.info["duration"] == 200 and im.info["loop"] == 0
        for t in range(4):
            im.seek(t)
            assert np.array_equal(np.asarray(im.convert("RGB")), frames[t])
    V.save_gif(list(frames), tmp_path / "b.gif", duration=50, loop=1)
    with Image.open(tmp_path / "b.gif") as im:
        assert im.n_frames == 4 and im.info["duration"] == 50 and im.info["loop"] == 1
