// Rasterisation of generated layouts — convert_layout_to_image / save_image (trainer/helpers/visualization.py:17-115) as
// Pillow's ImageDraw.rectangle(outline=colour, fill=colour + (100,)) on an "RGBA" draw of a white RGB canvas paints them —
// ONE source of the arithmetic, compiled for the device (kernels_render.hip: one workgroup per layout, pixels owned by
// threads) and for the host (tests/cpu_render_check.cpp).
//
// Per layout, over the elements its mask keeps, templated on the box type TB (float, double):
//   * order: larger area first, a = w * h rounded in TB, `sorted(..., key=a, reverse=True)`: descending and stable, so equal
//     areas keep element order (rank_of);
//   * pixel rectangle: (xc -/+ w / 2) * (W - 1), (yc -/+ h / 2) * (H - 1) in TB, every product rounded (no FMA contraction:
//     see the pragma below), then truncated toward zero — Pillow's (int) cast of the double it gets, -0.6 -> 0 (rect_of).
//     Values beyond +-2^30 stop there: the canvas is smaller, so the pixels painted are the same and nothing overflows;
//   * fill: every pixel with X1 <= x <= X2 and Y1 <= y <= Y2, blended with alpha 100 in Pillow's integer arithmetic (blend);
//   * outline, after the fill and opaque: rows Y1 and Y2 over X1..X2, columns X1 and X2 over rows min(Y1+1, Y2) ..
//     max(Y1+1, Y2) — Pillow's range: a zero-height box also paints row Y1 + 1 at its two columns (classify);
//   * everything is clipped to the canvas per pixel.
// An element whose box is not finite or whose w or h is negative (Pillow: ValueError, x1 < x0), or whose label has no
// colour (IndexError), is an error: box_ok / the callers' label check; such an element is not drawn.
//
// The mosaic of torchvision's make_grid(nrow, padding, pad_value=0) is an addressing rule on top: tile k of `cols` columns
// starts at ((k / cols) * (H + pad) + pad, (k % cols) * (W + pad) + pad) of a (GH, GW, 3) image (grid_shape, tile_origin).
// torchvision is not a dependency and was not available to check against: this geometry follows its documented make_grid.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LDM_RN_HD __host__ __device__ __forceinline__
#else
#define LDM_RN_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)  // torch rounds w * h and every product of the rectangle: no fused multiply-adds
#endif

namespace ldm_render {

constexpr int kMaxSlots = 256;        // element slots per layout (S); the reference's datasets have <= 25, FIDNetV3 50
constexpr int kMaxCanvas = 1 << 14;   // H, W and the padding
constexpr int kFillAlpha = 100;       // c_fill = colors[label] + (100,)
constexpr int32_t kCoordLimit = 1 << 30;

enum : int { kErrBox = 1, kErrLabel = 2 };            // bits of the error word
enum : int { kNone = 0, kFill = 1, kOutline = 2 };  // what an element does to a pixel

struct Rect {
  int32_t x1, y1, x2, y2;
};

template <typename TB>
LDM_RN_HD bool box_ok(const TB* b) {
  for (int i = 0; i < 4; ++i)
    if (!(b[i] - b[i] == TB(0))) return false;  // NaN, +-inf
  return !(b[2] < TB(0)) && !(b[3] < TB(0));
}

template <typename TB>
LDM_RN_HD int32_t to_pixel(TB v) {
  const double d = (double)v;
  if (!(d > -(double)kCoordLimit)) return -kCoordLimit;
  if (d >= (double)kCoordLimit) return kCoordLimit;
  return (int32_t)d;  // toward zero
}

// b = {xc, yc, w, h}; canvas H x W
template <typename TB>
LDM_RN_HD Rect rect_of(const TB* b, int H, int W) {
  const TB hw = b[2] / TB(2), hh = b[3] / TB(2);
  const TB sx = TB(W - 1), sy = TB(H - 1);
  const TB x1 = (b[0] - hw) * sx, x2 = (b[0] + hw) * sx;
  const TB y1 = (b[1] - hh) * sy, y2 = (b[1] + hh) * sy;
  return Rect{to_pixel(x1), to_pixel(y1), to_pixel(x2), to_pixel(y2)};
}

template <typename TB>
LDM_RN_HD TB area_of(const TB* b) {
  return b[2] * b[3];
}

// position of element i among the drawn ones: descending area, equal areas in element order.  area / drawn: n entries
template <typename TB>
LDM_RN_HD int rank_of(const TB* area, const uint8_t* drawn, int n, int i) {
  const TB a = area[i];
  int r = 0;
  for (int j = 0; j < n; ++j) r += (drawn[j] != 0) & ((area[j] > a) | ((area[j] == a) & (j < i)));
  return r;
}

LDM_RN_HD int classify(int x, int y, const Rect& r) {
  if (x < r.x1 || x > r.x2) return kNone;
  if (y == r.y1 || y == r.y2) return kOutline;
  if (x == r.x1 || x == r.x2) {
    const int32_t a = r.y1 + 1, lo = a < r.y2 ? a : r.y2, hi = a < r.y2 ? r.y2 : a;
    if (y >= lo && y <= hi) return kOutline;
  }
  return (y >= r.y1 && y <= r.y2) ? kFill : kNone;
}

// Pillow's BLEND(mask, old, colour) with mask = 100: DIV255(old * 155 + colour * 100)
LDM_RN_HD uint32_t blend(uint32_t old, uint32_t colour) {
  const uint32_t t = old * (255 - kFillAlpha) + colour * kFillAlpha + 128;
  return ((t >> 8) + t) >> 8;
}

LDM_RN_HD uint32_t pack_colour(const uint8_t* c) { return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16; }

// one element on one pixel; rgb holds the three channels
LDM_RN_HD void paint(uint32_t* rgb, int kind, uint32_t colour) {
  const uint32_t c0 = colour & 255, c1 = (colour >> 8) & 255, c2 = (colour >> 16) & 255;
  if (kind == kOutline) {
    rgb[0] = c0, rgb[1] = c1, rgb[2] = c2;
  } else if (kind == kFill) {
    rgb[0] = blend(rgb[0], c0), rgb[1] = blend(rgb[1], c1), rgb[2] = blend(rgb[2], c2);
  }
}

// make_grid: B tiles in `cols` columns -> (GH, GW); false when an argument is out of range
LDM_RN_HD bool grid_shape(int B, int H, int W, int cols, int pad, int64_t* GH, int64_t* GW) {
  if (B < 1 || H < 1 || W < 1 || cols < 1 || pad < 0 || H > kMaxCanvas || W > kMaxCanvas || pad > kMaxCanvas) return false;
  const int64_t rows = ((int64_t)B + cols - 1) / cols;
  *GH = rows * (H + pad) + pad;
  *GW = (int64_t)cols * (W + pad) + pad;
  return true;
}

LDM_RN_HD void tile_origin(int k, int H, int W, int cols, int pad, int64_t* oy, int64_t* ox) {
  *oy = (int64_t)(k / cols) * (H + pad) + pad;
  *ox = (int64_t)(k % cols) * (W + pad) + pad;
}

}  // namespace ldm_render
