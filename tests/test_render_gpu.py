"""Layouts as pictures on the MI355X (kernels_render.hip through the C-ABI and layout_dm_amd/visualization.py) against
tests/golden/render/reference.npz, the reference's own pictures (tools/make_render_golden.py): every pixel of every fixture
row BYTE FOR BYTE, float32 and float64; mosaics at the documented offsets at the batch sizes that can go wrong (B = 1, a
last row that is not full, more layouts than a few compute units hold at once); save_image's three return forms; the
trajectory frames of a real sampling call; the error word; and the built-in runner's LDM_SAVE_VIS switch."""
import os

import numpy as np
import pytest
import torch
import yaml

from test_render import G, SETS, first_difference, numpy_mosaic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "render", "reference.npz"))


def tensors(fx, name, dev=None, n=None):
    out = [torch.from_numpy(a[:n]) for a in G.load_inputs(fx)[name]]
    return [t.to(dev) for t in out] if dev is not None else out


@pytest.mark.parametrize("name", SETS)
def test_render_layouts_equals_the_reference_byte_for_byte(cuda, fx, name):
    from layout_dm_amd import visualization as V

    p, canvas = G.SETS[name]
    want = fx[f"{name}_image"]
    names = list(fx["hand_rows"]) if name.startswith("hand") else None
    for dev in (cuda, None):                     # device tensors stay where they are; host tensors are copied over
        bbox, label, mask = tensors(fx, name, dev)
        got = V.render_layouts(bbox, label, mask, fx["colors"], canvas)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        diff = first_difference(got.cpu().numpy(), want, names)
        assert diff is None, (name, dev, diff)
    B = len(want)
    one = V.render_layouts(bbox[B - 1:], label[B - 1:], mask[B - 1:], torch.from_numpy(fx["colors"]), canvas)   # B = 1
    assert np.array_equal(one.cpu().numpy(), want[B - 1:])


@pytest.mark.parametrize("name,B,nrow,pad", [("rand_f32", 1, None, 2), ("rand_f64", 3, None, 2), ("rand_f32", 70, 9, 2),
                                             ("rand_f64", 70, 9, 0), ("rand_f32", 3, None, 0), ("s50_f32", 12, 5, 2),
                                             ("s50_f64", 7, 3, 1), ("big_f64", 5, 4, 2)])
def test_render_grid_tiles_are_the_images_at_the_documented_offsets(cuda, fx, name, B, nrow, pad):
    from layout_dm_amd import visualization as V

    canvas = G.SETS[name][1]
    bbox, label, mask = tensors(fx, name, cuda, B)
    grid = V.render_grid(bbox, label, mask, fx["colors"], canvas, nrow=nrow, padding=pad)
    images = V.render_layouts(bbox, label, mask, fx["colors"], canvas).cpu().numpy()
    assert np.array_equal(images, fx[f"{name}_image"][:B])
    want, cols = numpy_mosaic(images, nrow if nrow is not None else int(np.ceil(np.sqrt(B))), pad)
    assert grid.is_cuda and tuple(grid.shape) == want.shape == V.grid_shape(B, canvas, nrow, pad)[:2] + (3,)
    assert np.array_equal(grid.cpu().numpy(), want)      # tiles at their offsets; padding and empty tiles black


def test_save_image_three_forms_agree(cuda, fx, tmp_path):
    from PIL import Image

    from layout_dm_amd import visualization as V

    colors = [tuple(int(v) for v in c) for c in fx["colors"]]          # the dataset's form: a list of tuples
    for name, B in (("rand_f32", 10), ("rand_f64", 3), ("hand_f32", 1)):
        want = fx[f"{name}_image"][:B]
        for dev in (cuda, None):
            bbox, label, mask = tensors(fx, name, dev, B)
            batch = V.save_image(bbox, label, mask, colors, names=["dropped"])
            assert batch.dtype == torch.float32 and tuple(batch.shape) == (B, 3, 60, 40) and batch.device == bbox.device
            unit = (torch.from_numpy(want).permute(0, 3, 1, 2).float() / 255)         # ToTensor on the host
            assert torch.equal(batch.cpu(), unit)
            grid = V.save_image(bbox, label, mask, colors, use_grid=True)
            assert isinstance(grid, np.ndarray) and grid.dtype == np.uint8
            mosaic, _ = numpy_mosaic(want, int(np.ceil(np.sqrt(B))), 0 if B == 1 else 2)
            assert np.array_equal(grid, mosaic)
            path = tmp_path / f"{name}_{B}_{dev is None}.png"
            assert V.save_image(bbox, label, mask, colors, path) is None
            with Image.open(path) as im:
                assert im.mode == "RGB" and np.array_equal(np.asarray(im), mosaic)
            # back from the float form, as vutils.save_image rounds it: the same bytes
            back = batch.cpu().mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8).numpy()
            assert np.array_equal(back, want)
    bbox, label, mask = tensors(fx, "rand_f32", cuda, 6)
    wide = V.save_image(bbox, label, mask, colors, use_grid=True, nrow=4, canvas_size=(120, 80))
    assert wide.shape == (2 * 122 + 2, 4 * 82 + 2, 3)


@pytest.fixture(scope="module")
def sampler(cuda):
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion
    from oracle import spec as SP
    from oracle import synth

    spec = SP.RICO25
    m = HipMaskAndReplaceDiffusion(n_category=spec.n_category, precision="fast", max_batch=8, device=0)
    m.load_state_dict(synth.synth_state_dict(spec, seed=1, perturb=True))
    return m


def test_render_trajectory_frames_are_the_decoded_steps(cuda, sampler):
    from layout_dm_amd import visualization as V

    colors = V.default_colors(25)
    cfg = {"name": "random", "num_timesteps": 4}         # T = 100 model, 4 strided steps
    steps = sampler.sample(batch_size=5, sampling_cfg=cfg, get_intermediate_results=True, seed=7)
    final = sampler.sample(batch_size=5, sampling_cfg=cfg, seed=7, return_device_tensor=True)
    assert len(steps) == 4 and torch.equal(steps[-1], final.long().cpu())
    eng = sampler.engine
    centres = torch.from_numpy(np.sort(np.random.default_rng(0).integers(1, 64, (4, eng.n_bin)) / 64.0, axis=1))
    for cen, nrow in ((None, None), (centres, 2)):
        frames = V.render_trajectory(eng, steps, colors, centres=cen, nrow=nrow)
        GH, GW, _ = V.grid_shape(5, (60, 40), nrow)
        assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (4, GH, GW, 3)
        drawn = []
        for t, ids in enumerate(steps):
            dec = eng.decode(ids, cen)
            assert dec["bbox"].dtype == (torch.float32 if cen is None else torch.float64)
            assert torch.equal(frames[t], V.render_grid(dec["bbox"], dec["label"], dec["mask"], colors, nrow=nrow)), (t, nrow)
            drawn.append(int(dec["mask"].sum()))
        dec = eng.decode(final, cen)
        assert torch.equal(frames[-1], V.render_grid(dec["bbox"], dec["label"], dec["mask"], colors, nrow=nrow))
        assert drawn[-1] > 0 and (frames[-1] != frames[0]).any()
        # the (T,B,S) tensor form, on the device
        again = V.render_trajectory(eng, torch.stack(steps).to(cuda), colors, centres=cen, nrow=nrow)
        assert torch.equal(again, frames)
    # an element whose tokens are still [MASK] is absent: a frame of nothing but [MASK] is blank tiles
    blank = V.render_trajectory(eng, [torch.full((5, eng.S), eng.mask_id)], colors)
    tiles = V.render_grid(torch.zeros(5, 1, 4), torch.zeros(5, 1, dtype=torch.long), torch.zeros(5, 1, dtype=torch.bool), colors)
    assert torch.equal(blank[0], tiles) and int((tiles == 255).sum()) == 5 * 60 * 40 * 3


def test_one_bad_layout_raises_and_the_others_are_still_drawn(cuda, fx):
    from layout_dm_amd import visualization as V

    want = fx["rand_f32_image"]
    for what, exc in (("nan", ValueError), ("negative_w", ValueError), ("label", IndexError)):
        for dt in (torch.float32, torch.float64):
            bbox, label, mask = tensors(fx, "rand_f32", cuda, 6)
            bbox = bbox.to(dt)
            ref = fx["rand_f32_image"][:6] if dt == torch.float32 else V.render_layouts(bbox, label, mask, fx["colors"]).cpu().numpy()
            assert bool(mask[3, 0]) and int(mask[3].sum()) >= 2
            if what == "nan":
                bbox[3, 0, 0] = float("nan")
            elif what == "negative_w":
                bbox[3, 0, 2] = -0.125
            else:
                label[3, 0] = 25
            with pytest.raises(exc) as info:
                V.render_layouts(bbox, label, mask, fx["colors"])
            got = info.value.rendered.cpu().numpy()
            good = [0, 1, 2, 4, 5]
            assert np.array_equal(got[good], ref[good]), (what, dt)
            mask[3, 0] = False                     # the bad element alone is missing from its layout
            assert np.array_equal(got[3], V.render_layouts(bbox, label, mask, fx["colors"]).cpu().numpy()[3])
            with pytest.raises(exc):
                mask[3, 0] = True
                V.render_grid(bbox, label, mask, fx["colors"])
    assert want.shape[0] == 70
    # more slots than the kernel takes, more colours than labels, rubbish under the mask: refused / fine / ignored
    with pytest.raises(ValueError, match="at most 256"):
        V.render_layouts(torch.zeros(1, 257, 4), torch.zeros(1, 257, dtype=torch.long), torch.zeros(1, 257, dtype=torch.bool), fx["colors"])
    bbox, label, mask = tensors(fx, "hand_f64", cuda)
    assert torch.isnan(bbox[~mask]).any() and int(label[~mask].max()) == 999
    assert np.array_equal(V.render_layouts(bbox, label, mask, fx["colors"]).cpu().numpy(), fx["hand_f64_image"])


def test_builtin_runner_writes_the_picture_only_when_asked(cuda, tmp_path, monkeypatch):
    from PIL import Image

    from layout_dm_amd import cond_entry as CE
    from layout_dm_amd import synthetic as SY
    from layout_dm_amd import test_entry as TE
    from layout_dm_amd import visualization as V
    from layout_dm_amd.layoutdm import LayoutDM
    from test_entry_point import TRAIN_CFG

    job = tmp_path / "job"
    job.mkdir()
    (job / "config.yaml").write_text(yaml.safe_dump(TRAIN_CFG))
    torch.save({k: torch.from_numpy(v) for k, v in SY.synth_state_dict(SY.RICO25, seed=1, perturb=True).items()}, job / "best_model.pt")
    args = [f"job_dir={job}", "num_uncond_samples=7", "max_batch_size=5", "num_timesteps=4", "sampling=random"]
    monkeypatch.delenv(V.VIS_ENV, raising=False)
    out = CE.run_builtin_unconditional(TE.parse_cli(args + [f"result_dir={tmp_path / 'off'}"]))
    assert "images" not in out and [f for f in os.listdir(out["result_dir"])] == ["seed_0.pkl"]
    monkeypatch.setenv(V.VIS_ENV, "1")
    out = CE.main(args + [f"result_dir={tmp_path / 'on'}"]) if not CE._reference_importable() else \
        CE.run_builtin_unconditional(TE.parse_cli(args + [f"result_dir={tmp_path / 'on'}"]))
    png = os.path.join(out["result_dir"], "test_generated.png")
    assert out["images"] == [png] and sorted(os.listdir(out["result_dir"])) == ["seed_0.pkl", "test_generated.png"]
    with Image.open(png) as im:
        arr = np.asarray(im)
    GH, GW, _ = V.grid_shape(5)              # batch 0 holds max_batch_size = 5 layouts: 3 columns, 2 rows
    assert im.mode == "RGB" and arr.shape == (GH, GW, 3) == (126, 128, 3)
    assert not arr[:2].any() and (arr[2:62, 2:42] == 255).any() and not arr[64:, 86:].any()   # padding, a tile, the empty tile
    # the file is the mosaic of batch 0 drawn under its mask: the same seed through the model class, like test.py
    tok = TE.GeometryTokenizer(TE.to_attr(TRAIN_CFG["data"]), TE.to_attr(TRAIN_CFG["dataset"]))
    m = LayoutDM(backbone_cfg=TE.to_attr(TRAIN_CFG["backbone"]), tokenizer=tok, q_type="constrained", max_batch=5)
    m.load_state_dict(torch.load(job / "best_model.pt"))
    torch.manual_seed(0)
    lay = m.sample(batch_size=5, cond=None, sampling_cfg=TE.AttrDict(name="random", temperature=1.0, num_timesteps=4))
    want = V.save_image(lay["bbox"], lay["label"], lay["mask"], V.default_colors(25), use_grid=True)
    assert np.array_equal(arr, want) and int(lay["mask"].sum()) > 0
    monkeypatch.setenv(V.VIS_ENV, str(tmp_path / "elsewhere" / "pic.png"))
    out = CE.run_builtin_unconditional(TE.parse_cli(args + [f"result_dir={tmp_path / 'path'}"]))
    assert out["images"] == [str(tmp_path / "elsewhere" / "pic.png")] and os.listdir(out["result_dir"]) == ["seed_0.pkl"]
    with Image.open(out["images"][0]) as im:
        assert im.size == (128, 126)
