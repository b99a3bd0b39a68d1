"""Generated layouts as pictures on the MI355X — drop-in for `save_image` of the reference's visualisation helpers
(trainer/helpers/visualization.py:17-115; test.py:205-214 calls it on the first batch of every run, render.py builds on it),
plus what a diffusion sampler invites: the denoising trajectory as animation frames.

    from layout_dm_amd.visualization import save_image          # the reference's signature and return forms
    from layout_dm_amd.visualization import render_layouts, render_grid, render_trajectory, save_gif, default_colors

Inputs are what `LayoutDM.sample` / `Engine.decode` return: `bbox` (B,S,4) (xc, yc, w, h) float32 or float64, `label` (B,S),
`mask` (B,S) bool; `colors` is a list of RGB triples indexed by label (the dataset's `colors`) or an (n,3) uint8 array.
Tensors already on the device stay there (the decode kernel's output feeds the render kernel directly); CPU tensors are
copied over.  One launch of `render_layouts_k` (kernels_render.hip: one workgroup per layout, pixels owned by threads)
draws every layout exactly as Pillow's ImageDraw.rectangle does for the reference — white canvas, larger areas first,
fill blended with alpha 100, opaque outline — pixel for pixel, for float32 and float64 boxes.  PNG / GIF encoding stays with
PIL, on the uint8 frames the kernel produced.  No CPU fallback: without the extension or a GPU this raises.

Not drawn here (NotImplementedError): text labels (`draw_label`) and background / patch compositing (`batch_resources`).

The mosaic is torchvision's make_grid(nrow, padding=2, pad_value=0) as documented — tile k of min(nrow, B) columns at row
(k // cols) * (H + padding) + padding, column (k % cols) * (W + padding) + padding of a (GH, GW, 3) image, GH = ceil(B / cols)
* (H + padding) + padding, GW = cols * (W + padding) + padding.  torchvision is not a dependency and was not available to
check against, so this geometry is not pinned by the reference's own output.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .binding import _stream_ptr, load_library

MAX_ELEMENTS = 256     # element slots per layout (ldm_render::kMaxSlots)
MAX_CANVAS = 1 << 14   # H, W, padding
VIS_ENV = "LDM_SAVE_VIS"


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("layout_dm_amd.visualization needs a ROCm GPU (MI355X); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def default_colors(n: int):
    """n distinct RGB triples for callers without a dataset: hues a golden-ratio step apart at two alternating lightness
    levels, deterministic.  NOT the reference's palette — its datasets take seaborn's `husl` (datasets/base.py), and seaborn
    is not a dependency — so pictures drawn with these colours differ from the reference's in colour, not in geometry."""
    import colorsys

    out = []
    for i in range(int(n)):
        r, g, b = colorsys.hls_to_rgb((i * 0.6180339887498949) % 1.0, 0.45 if i % 2 == 0 else 0.6, 0.75)
        out.append((int(round(r * 255)), int(round(g * 255)), int(round(b * 255))))
    return out


def grid_shape(B: int, canvas_size: Tuple[int, int] = (60, 40), nrow: Optional[int] = None, padding: int = 2):
    """(GH, GW, cols) of the mosaic of B tiles (ldm_render_grid_shape); nrow defaults to ceil(sqrt(B))."""
    H, W = (int(v) for v in canvas_size)
    if nrow is None:
        nrow = int(math.ceil(math.sqrt(B)))
    cols = max(1, min(int(nrow), int(B)))
    gh, gw = C.c_int64(), C.c_int64()
    if load_library().ldm_render_grid_shape(int(B), H, W, cols, int(padding), C.byref(gh), C.byref(gw)) != 0:
        raise ValueError(f"render: B >= 1, 1 <= H, W <= {MAX_CANVAS}, 0 <= padding <= {MAX_CANVAS}, nrow >= 1; got B={B}, "
                         f"canvas_size={tuple(canvas_size)}, nrow={nrow}, padding={padding}")
    return int(gh.value), int(gw.value), cols


def _palette(colors, dev) -> torch.Tensor:
    c = np.asarray(colors.cpu() if isinstance(colors, torch.Tensor) else colors)
    if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 1:
        raise ValueError(f"colors must be n >= 1 RGB triples; got shape {c.shape}")
    if (c < 0).any() or (c > 255).any() or not np.array_equal(c, np.floor(c)):
        raise ValueError("colors must be integers in 0..255")
    return torch.from_numpy(np.ascontiguousarray(c, np.uint8)).to(dev)


def _launch(bbox, label, mask, palette, canvas_size, cols: int, pad: int, out: torch.Tensor, err: torch.Tensor):
    """one ldm_render_layouts call on tensors already in the kernel's form; out (GH,GW,3) uint8, err (1,) int32"""
    B, S = mask.shape
    H, W = (int(v) for v in canvas_size)
    dev = bbox.device
    with torch.cuda.device(dev):
        rc = load_library().ldm_render_layouts(bbox.data_ptr(), int(bbox.dtype == torch.float64), label.data_ptr(),
                                               mask.data_ptr(), B, S, palette.data_ptr(), palette.shape[0], H, W, cols, pad,
                                               out.data_ptr(), err.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        raise RuntimeError(f"ldm_render_layouts failed ({rc}): 1 <= S <= {MAX_ELEMENTS} elements per layout, "
                           f"1 <= H, W <= {MAX_CANVAS}" if rc == -1 else f"ldm_render_layouts failed ({rc})")


def _raise_for(word: int, rendered: torch.Tensor):
    """the error word as the exception Pillow / the colour list would raise; the exception carries the picture as `.rendered`
    (the offending elements are missing from it, everything else is drawn)"""
    if word & 1:
        e = ValueError("render: a box that is not finite or has a negative width or height (Pillow: x1 must be greater "
                       "than or equal to x0)")
    elif word & 2:
        e = IndexError("render: a label outside the colour list")
    else:
        return
    e.rendered = rendered
    raise e


def _prepare(bbox, label, mask, colors):
    bbox, label, mask = torch.as_tensor(bbox), torch.as_tensor(label), torch.as_tensor(mask)
    dev = bbox.device if bbox.is_cuda else _device()
    if bbox.dim() != 3 or bbox.shape[-1] != 4 or tuple(mask.shape) != tuple(bbox.shape[:2]) or label.shape != mask.shape \
            or 0 in mask.shape:
        raise ValueError(f"bbox must be (B,S,4), label and mask (B,S), B, S >= 1; got {tuple(bbox.shape)}, "
                         f"{tuple(label.shape)}, {tuple(mask.shape)}")
    if mask.shape[1] > MAX_ELEMENTS:
        raise ValueError(f"at most {MAX_ELEMENTS} elements per layout (got {mask.shape[1]})")
    dt = torch.float64 if bbox.dtype == torch.float64 else torch.float32
    return (bbox.to(device=dev, dtype=dt).contiguous(), label.to(device=dev, dtype=torch.int64).contiguous(),
            mask.to(device=dev, dtype=torch.uint8).contiguous(), _palette(colors, dev))


def _render(bbox, label, mask, colors, canvas_size, nrow, padding, batch_form: bool) -> torch.Tensor:
    b, l, m, pal = _prepare(bbox, label, mask, colors)
    B = m.shape[0]
    if batch_form:
        GH, GW, cols = grid_shape(B, canvas_size, 1, 0)
    else:
        GH, GW, cols = grid_shape(B, canvas_size, nrow, padding)
    out = torch.empty((GH, GW, 3), dtype=torch.uint8, device=b.device)
    err = torch.zeros(1, dtype=torch.int32, device=b.device)
    _launch(b, l, m, pal, canvas_size, cols, 0 if batch_form else int(padding), out, err)
    if batch_form:
        out = out.view(B, GH // B, GW, 3)
    _raise_for(int(err.item()), out)   # (synchronises: the temporaries above are done with)
    return out


def render_layouts(bbox, label, mask, colors, canvas_size: Tuple[int, int] = (60, 40)) -> torch.Tensor:
    """uint8 (B, H, W, 3) on the device: convert_layout_to_image (visualization.py:17-63) of every layout."""
    return _render(bbox, label, mask, colors, canvas_size, 1, 0, True)


def render_grid(bbox, label, mask, colors, canvas_size: Tuple[int, int] = (60, 40), nrow: Optional[int] = None,
                padding: int = 2) -> torch.Tensor:
    """uint8 (GH, GW, 3) on the device: the pictures of render_layouts as one make_grid mosaic (grid_shape), black
    padding; nrow defaults to ceil(sqrt(B))."""
    return _render(bbox, label, mask, colors, canvas_size, nrow, padding, False)


_UNIT = None


def _to_unit(img: torch.Tensor) -> torch.Tensor:
    """uint8 -> float32 uint8 / 255 exactly as torchvision's ToTensor divides on the host: a 256-entry table computed on the CPU"""
    global _UNIT
    if _UNIT is None:
        _UNIT = torch.arange(256, dtype=torch.float32) / 255
    return _UNIT.to(img.device)[img.long()]


def save_image(batch_boxes, batch_labels, batch_mask, colors, out_path=None, canvas_size: Optional[Tuple[int, int]] = (60, 40),
               nrow: Optional[int] = None, batch_resources=None, use_grid: bool = False, draw_label: bool = False, **kwargs):
    """visualization.py:66-115 with the drawing on the device.  With out_path: writes the mosaic (PIL encodes the uint8
    grid; the format follows the file name) and returns None.  With use_grid: the (GH, GW, 3) uint8 numpy mosaic.  Otherwise
    float32 (B, 3, H, W), every value uint8 / 255, on the inputs' device.  A single layout comes back without padding, as
    make_grid returns a batch of one image unchanged."""
    if draw_label:
        raise NotImplementedError("draw_label=True: text labels are not drawn on the device (use the reference's PIL path)")
    if batch_resources:
        raise NotImplementedError("batch_resources: background / patch compositing is not done on the device")
    kwargs.pop("names", None)   # (the reference drops it when draw_label is false)
    if out_path or use_grid:
        B = torch.as_tensor(batch_mask).shape[0]
        grid = render_grid(batch_boxes, batch_labels, batch_mask, colors, canvas_size, nrow, 0 if B == 1 else 2)
        arr = grid.cpu().numpy()
        if not out_path:
            return arr
        from PIL import Image

        Image.fromarray(arr).save(os.fspath(out_path))
        return None
    img = render_layouts(batch_boxes, batch_labels, batch_mask, colors, canvas_size)
    return _to_unit(img.permute(0, 3, 1, 2)).contiguous().to(torch.as_tensor(batch_boxes).device)


def render_trajectory(engine, tokens_per_step, colors, centres=None, canvas_size: Tuple[int, int] = (60, 40),
                      nrow: Optional[int] = None, padding: int = 2) -> torch.Tensor:
    """uint8 (T, GH, GW, 3) on the device: one mosaic per sampling step.  tokens_per_step is what
    `sample(..., get_intermediate_results=True)` returns — a list of T (B,S) id tensors — or a (T,B,S) tensor (the device
    intermediates of Engine.sample_loop).  Every step is decoded with Engine.decode (centres as there: None = linear bins)
    and drawn by the render kernel; an element decode marks invalid — a still-masked one included — is absent."""
    steps = list(tokens_per_step) if not isinstance(tokens_per_step, torch.Tensor) else list(tokens_per_step.unbind(0))
    if not steps:
        raise ValueError("render_trajectory: no steps")
    dev = engine.device
    pal = _palette(colors, dev)
    B = steps[0].shape[0]
    GH, GW, cols = grid_shape(B, canvas_size, nrow, padding)
    frames = torch.empty((len(steps), GH, GW, 3), dtype=torch.uint8, device=dev)
    err = torch.zeros((len(steps), 1), dtype=torch.int32, device=dev)
    for t, ids in enumerate(steps):
        if tuple(ids.shape) != (B, engine.S):
            raise ValueError(f"step {t}: ids must be ({B},{engine.S}); got {tuple(ids.shape)}")
        dec = engine.decode(ids, centres)
        if dec["mask"].shape[1] > MAX_ELEMENTS:
            raise ValueError(f"at most {MAX_ELEMENTS} elements per layout (got {dec['mask'].shape[1]})")
        _launch(dec["bbox"], dec["label"], dec["mask"].to(torch.uint8), pal, canvas_size, cols, int(padding), frames[t], err[t])
    word = 0
    for w in err.flatten().tolist():   # (synchronises once, after the last step)
        word |= w
    _raise_for(word, frames)
    return frames


def save_gif(frames, out_path, duration: int = 200, loop: int = 0):
    """An animation of (T, GH, GW, 3) uint8 frames (render_trajectory's, or a list of such images), written with PIL with
    the parameters of the reference's save_gif (visualization.py:354-371): save_all, optimize=False, duration=200, loop=0."""
    from PIL import Image

    if isinstance(frames, torch.Tensor):
        frames = frames.cpu().numpy()
    imgs = [Image.fromarray(np.ascontiguousarray(np.asarray(f.cpu() if isinstance(f, torch.Tensor) else f), dtype=np.uint8))
            for f in frames]
    if not imgs:
        raise ValueError("save_gif: no frames")
    imgs[0].save(os.fspath(out_path), save_all=True, append_images=imgs[1:], optimize=False, duration=duration, loop=loop)


def vis_path(result_dir: str) -> Optional[str]:
    """Where the hydra-less runners write the picture of batch 0: None unless LDM_SAVE_VIS is set; "1" ->
    <result_dir>/test_generated.png (the reference writes tmp/test_generated.png); any other value is the path itself."""
    v = os.environ.get(VIS_ENV, "")
    if not v:
        return None
    return os.path.join(result_dir, "test_generated.png") if v == "1" else v


def save_first_batch(layouts, result_dir: str, n_colors: int, colors: Optional[Sequence] = None) -> Optional[str]:
    """test.py:205-214 for the hydra-less runners: with LDM_SAVE_VIS set, the mosaic of `layouts` ({"bbox", "label", "mask"})
    as a PNG at vis_path(result_dir).  Returns the path written, or None."""
    path = vis_path(result_dir)
    if path is None:
        return None
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    save_image(layouts["bbox"], layouts["label"], layouts["mask"], colors if colors is not None else default_colors(n_colors), path)
    return path
