"""Writes tests/golden/render/reference.npz: the reference's own pictures of layouts — convert_layout_to_image
(trainer/helpers/visualization.py:17-63), called per layout with boxes[mask] / labels[mask] as save_image (l.66-115) calls it,
so Pillow gets 0-dim torch scalars — with their inputs, for tests/test_render.py and tests/test_render_gpu.py.

    python tools/make_render_golden.py     # needs the reference tree (oracle.ref_harness.install_stubs()) and Pillow

Sets (`SETS`: name -> dtype, canvas (H, W)); each holds bbox (B,S,4), label (B,S), mask (B,S) and image (B,H,W,3) uint8:
  * rand_f32 / rand_f64        70 seeded layouts of 0 - 25 elements (S = 25) on the default canvas (60, 40): float32 boxes of
                               32 linear bins (xc, yc = id / 32, w, h = (id + 1) / 32, bbox_tokenizer.py:141-146), float64
                               boxes looked up in sorted float64 centres (kmeans decode); every fifth mask has holes.
  * big_f32 / big_f64          32 such layouts on render.py's canvas (120, 80).
  * s50_f32 / s50_f64          12 layouts of 26 - 50 elements (S = 50, FIDNetV3's max_bbox).
  * hand_f32 / hand_f64        hand-made rows (`handmade`, names in HAND_ROWS): zero width / height / both, inside, on the
                               canvas edge and in its corners; three boxes of equal area in all six element orders; a box
                               covering the canvas listed after smaller ones; boxes over each edge and corner, beyond the
                               canvas, larger than it; coordinates whose pixel product is a whole number, one ulp either
                               side; an all-masked layout; a mask with holes whose masked slots hold NaN boxes and labels
                               without a colour; labels 0 and n_colors - 1.
  * px1_f32 / px1_f64, c75_f32 / c75_f64   free coordinates on a 1 x 1 and a 7 x 5 canvas.
The colours are seeded random RGB triples.  The file also names the Pillow version that drew it.  Only data: no program text.
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "render", "reference.npz")
SEED = 20261018
N_COLORS = 25
DTYPE = {"f32": np.float32, "f64": np.float64}
SETS = {f"{s}_{p}": (p, canvas) for s, canvas in (("rand", (60, 40)), ("big", (120, 80)), ("s50", (60, 40)), ("hand", (60, 40)),
                                                   ("px1", (1, 1)), ("c75", (7, 5))) for p in ("f32", "f64")}
HAND_S = 8


def colors():
    return np.random.default_rng(SEED).integers(0, 256, (N_COLORS, 3)).astype(np.uint8)


def _binned(rng, p, B, S, n_lo, n_hi):
    T = DTYPE[p]
    ids = rng.integers(0, 32, (B, S, 4))
    if p == "f32":
        d = 1 / 32
        box = np.concatenate([ids[..., :2].astype(np.float32) * np.float32(d), (ids[..., 2:] + 1).astype(np.float32) * np.float32(d)], -1)
    else:
        centres = np.sort(rng.random((4, 32)), axis=1)
        box = np.stack([centres[a][ids[..., a]] for a in range(4)], -1)
    n = rng.integers(n_lo, n_hi + 1, B)
    mask = np.arange(S)[None, :] < n[:, None]
    for b in range(0, B, 5):   # holes: the kernel takes any mask, not only the prefix decode leaves
        mask[b] &= rng.random(S) < 0.7
    label = rng.integers(0, N_COLORS, (B, S))
    return np.ascontiguousarray(box, T), label.astype(np.int64), mask


def _free(rng, p, B, S):
    T = DTYPE[p]
    box = rng.random((B, S, 4)) * np.array([1.4, 1.4, 1.2, 1.2]) - np.array([0.2, 0.2, 0.0, 0.0])
    mask = rng.random((B, S)) < 0.8
    return np.ascontiguousarray(box.astype(T)), rng.integers(0, N_COLORS, (B, S)).astype(np.int64), mask


def handmade(p, canvas=(60, 40)):
    """-> (names, bbox (B,HAND_S,4), label, mask): the rows of HAND_ROWS, arithmetic in DTYPE[p]"""
    T = DTYPE[p]
    H, W = canvas
    up, dn = (lambda v: np.nextafter(T(v), T(4))), (lambda v: np.nextafter(T(v), T(-4)))
    rows = []   # (name, [(xc, yc, w, h, label)] or (boxes, mask))

    def add(name, *elems):
        rows.append((name, list(elems)))

    add("zero_width_inside", (0.5, 0.5, 0.0, 0.3, 1))
    add("zero_height_inside", (0.5, 0.5, 0.3, 0.0, 2))
    add("zero_both_inside", (0.5, 0.5, 0.0, 0.0, 3))
    add("zero_width_left_edge", (0.0, 0.5, 0.0, 0.4, 4))
    add("zero_width_right_edge", (1.0, 0.5, 0.0, 0.4, 5))
    add("zero_height_top_edge", (0.5, 0.0, 0.4, 0.0, 6))
    add("zero_height_bottom_edge", (0.5, 1.0, 0.4, 0.0, 7))
    add("zero_both_corners", (0.0, 0.0, 0.0, 0.0, 8), (1.0, 1.0, 0.0, 0.0, 9), (1.0, 0.0, 0.0, 0.0, 10), (0.0, 1.0, 0.0, 0.0, 11))
    add("zero_over_filled", (0.5, 0.5, 0.6, 0.6, 1), (0.5, 0.5, 0.0, 0.3, 2), (0.4, 0.4, 0.3, 0.0, 3), (0.6, 0.6, 0.0, 0.0, 4))
    same = [(0.4, 0.4, 0.4, 0.2, 12), (0.5, 0.5, 0.2, 0.4, 13), (0.6, 0.45, 0.4, 0.2, 14)]
    for i, perm in enumerate(itertools.permutations(range(3))):
        add(f"equal_area_order_{i}", *[same[j] for j in perm])
    add("canvas_box_under_smaller", (0.3, 0.3, 0.2, 0.2, 15), (0.6, 0.6, 0.4, 0.3, 16), (0.5, 0.5, 1.0, 1.0, 17), (0.5, 0.5, 0.1, 0.1, 18))
    add("over_edges", (0.0, 0.5, 0.3, 0.3, 19), (1.0, 0.5, 0.3, 0.3, 20), (0.5, 0.0, 0.3, 0.3, 21), (0.5, 1.0, 0.3, 0.3, 22))
    add("over_corners", (0.0, 0.0, 0.3, 0.3, 19), (1.0, 0.0, 0.3, 0.3, 20), (0.0, 1.0, 0.3, 0.3, 21), (1.0, 1.0, 0.3, 0.3, 22))
    add("beyond_and_larger", (1.5, 0.5, 0.2, 0.2, 1), (0.5, 0.5, 1.5, 1.5, 2), (-0.2, 0.3, 0.6, 0.2, 3), (0.5, -0.01, 0.2, 0.01, 4),
        (0.5, 1.2, 3.0, 0.39, 5))
    add("labels_first_and_last", (0.3, 0.5, 0.4, 0.6, 0), (0.7, 0.5, 0.4, 0.6, N_COLORS - 1))
    # pixel boundaries: v * (W - 1) (v * (H - 1)) is the whole number k at v, and v's neighbours lie either side
    for axis, scale, ks in (("x", W - 1, (7, 20, 39)), ("y", H - 1, (11, 30, 59))):
        for k in ks:
            v = T(k) / T(scale)
            for tag, u in (("dn", dn(v)), ("at", v), ("up", up(v))):
                half = T(0.125)
                if axis == "x":
                    add(f"boundary_x{k}_{tag}", (u, 0.3, 0.0, 0.2, 6), (T(u - half), 0.7, 0.25, 0.2, 7))
                else:
                    add(f"boundary_y{k}_{tag}", (0.3, u, 0.2, 0.0, 8), (0.7, T(u - half), 0.2, 0.25, 9))
    add("all_masked")
    names = [n for n, _ in rows] + ["mask_with_holes"]
    B = len(names)
    box = np.zeros((B, HAND_S, 4), T)
    label = np.zeros((B, HAND_S), np.int64)
    mask = np.zeros((B, HAND_S), bool)
    for b, (_, elems) in enumerate(rows):
        for s, e in enumerate(elems):
            box[b, s] = [T(v) for v in e[:4]]
            label[b, s] = e[4]
            mask[b, s] = True
    # the all-masked row and the holes keep rubbish under the mask: it must not be read as an element
    b = names.index("all_masked")
    box[b], label[b] = np.nan, 999
    b = names.index("mask_with_holes")
    box[b], label[b] = np.nan, -7
    for s, e in ((0, (0.5, 0.5, 0.5, 0.5, 1)), (2, (0.4, 0.4, 0.3, 0.5, 2)), (5, (0.6, 0.6, 0.5, 0.3, 3)), (7, (0.5, 0.5, 0.1, 0.1, 4))):
        box[b, s], label[b, s], mask[b, s] = [T(v) for v in e[:4]], e[4], True
    return names, box, label, mask


HAND_ROWS = handmade("f32")[0]


def inputs():
    """{set: (bbox, label, mask)} — reproducible without the reference"""
    out = {}
    for i, (name, (p, canvas)) in enumerate(SETS.items()):
        rng = np.random.default_rng([SEED, i])
        kind = name.rsplit("_", 1)[0]
        if kind == "rand":
            out[name] = _binned(rng, p, 70, 25, 0, 25)
        elif kind == "big":
            out[name] = _binned(rng, p, 32, 25, 0, 25)
        elif kind == "s50":
            out[name] = _binned(rng, p, 12, 50, 26, 50)
        elif kind == "hand":
            out[name] = handmade(p, canvas)[1:]
        else:
            out[name] = _free(rng, p, 12, 6)
    return out


def load_inputs(fx):
    """the same structure from the committed file"""
    return {name: (fx[f"{name}_bbox"], fx[f"{name}_label"].astype(np.int64), fx[f"{name}_mask"]) for name in SETS}


def reference_images(bbox, label, mask, palette, canvas):
    """the reference's convert_layout_to_image, layout by layout as save_image drives it -> (B,H,W,3) uint8"""
    import torch

    from oracle import ref_harness as rh

    rh.install_stubs()
    from trainer.helpers.visualization import convert_layout_to_image

    cols = [tuple(int(v) for v in c) for c in palette]
    bb, ll, mm = torch.from_numpy(bbox), torch.from_numpy(label), torch.from_numpy(mask)
    H, W = canvas
    out = np.zeros((len(bbox), H, W, 3), np.uint8)
    for i in range(len(bbox)):
        img = convert_layout_to_image(bb[i][mm[i]], ll[i][mm[i]], cols, canvas)
        out[i] = np.asarray(img)
    return out


def compute(inp):
    import PIL

    palette = colors()
    out = {"seed": np.int64(SEED), "colors": palette, "pillow_version": np.str_(PIL.__version__),
           "hand_rows": np.array(HAND_ROWS)}
    for name, (p, canvas) in SETS.items():
        bbox, label, mask = inp[name]
        assert bbox.dtype == DTYPE[p]
        out[f"{name}_bbox"], out[f"{name}_label"], out[f"{name}_mask"] = bbox, label.astype(np.int16), mask
        out[f"{name}_canvas"] = np.asarray(canvas, np.int32)
        out[f"{name}_image"] = reference_images(bbox, label, mask, palette, canvas)
    return out


def main():
    out = compute(inputs())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes; Pillow", out["pillow_version"])
    for name in SETS:
        img = out[f"{name}_image"]
        print(name, img.shape, "elements", int(out[f"{name}_mask"].sum()), "non-white pixels", int((img != 255).any(-1).sum()))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
