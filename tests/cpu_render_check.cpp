// Host build of layout_dm_amd/csrc/ldm_render_core.h (the arithmetic of kernels_render.hip), laid out like the kernel: rank
// the drawn elements, then walk them in order on every pixel of the layout's tile.
// tests/test_render.py runs it against the reference-produced fixture tests/golden/render/reference.npz.
//
// in:  int32 {f64, B, S, n_colors, H, W, cols, pad}, box [B][S][4] (float64 if f64 else float32), label int64 [B][S],
//      mask uint8 [B][S], colors uint8 [n_colors][3]
// out: int32 error word (bit 0 = bad box, bit 1 = label without a colour), then uint8 [GH][GW][3], zero outside the tiles
// exit 2: malformed input or an argument beyond the limits
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_render_core.h"
#include "cpu_check_io.h"

namespace {

using check_io::read_vec;

template <typename TB>
int render(const std::vector<TB>& box, const std::vector<int64_t>& label, const std::vector<uint8_t>& mask,
           const std::vector<uint8_t>& colors, int B, int S, int n_colors, int H, int W, int cols, int pad, int64_t GW,
           std::vector<uint8_t>& out) {
  namespace R = ldm_render;
  int err = 0;
  std::vector<TB> area(S);
  std::vector<uint8_t> drawn(S);
  std::vector<R::Rect> rect(S), ranked(S);
  std::vector<uint32_t> colour(S), ranked_colour(S);
  for (int k = 0; k < B; ++k) {
    int n = 0;
    for (int t = 0; t < S; ++t) {
      const size_t row = (size_t)k * S + t;
      area[t] = TB(0), drawn[t] = 0;
      if (!mask[row]) continue;
      const TB* b = &box[4 * row];
      int bad = 0;
      if (!R::box_ok(b)) bad |= R::kErrBox;
      if (label[row] < 0 || label[row] >= n_colors) bad |= R::kErrLabel;
      err |= bad;
      if (bad) continue;
      drawn[t] = 1, ++n;
      rect[t] = R::rect_of(b, H, W);
      area[t] = R::area_of(b);
      colour[t] = R::pack_colour(&colors[3 * label[row]]);
    }
    for (int t = 0; t < S; ++t) {
      if (!drawn[t]) continue;
      const int at = R::rank_of(area.data(), drawn.data(), S, t);
      ranked[at] = rect[t], ranked_colour[at] = colour[t];
    }
    int64_t oy, ox;
    R::tile_origin(k, H, W, cols, pad, &oy, &ox);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        uint32_t rgb[3] = {255, 255, 255};
        for (int e = 0; e < n; ++e) R::paint(rgb, R::classify(x, y, ranked[e]), ranked_colour[e]);
        uint8_t* o = &out[(size_t)(((oy + y) * GW + ox + x) * 3)];
        o[0] = (uint8_t)rgb[0], o[1] = (uint8_t)rgb[1], o[2] = (uint8_t)rgb[2];
      }
  }
  return err;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* f = check_io::open_or_exit(argv[1], "rb", 1);
  int32_t hdr[8];
  if (fread(hdr, 4, 8, f) != 8) return 2;
  const int f64 = hdr[0], B = hdr[1], S = hdr[2], n_colors = hdr[3], H = hdr[4], W = hdr[5], cols = hdr[6], pad = hdr[7];
  int64_t GH = 0, GW = 0;
  if ((f64 != 0 && f64 != 1) || S < 1 || S > ldm_render::kMaxSlots || n_colors < 1) return 2;
  if (!ldm_render::grid_shape(B, H, W, cols, pad, &GH, &GW)) return 2;
  std::vector<float> b32;
  std::vector<double> b64;
  std::vector<int64_t> label;
  std::vector<uint8_t> mask, colors;
  const size_t n = (size_t)B * S;
  if (!(f64 ? read_vec(f, b64, n * 4) : read_vec(f, b32, n * 4))) return 2;
  if (!read_vec(f, label, n) || !read_vec(f, mask, n) || !read_vec(f, colors, (size_t)n_colors * 3)) return 2;
  fclose(f);
  std::vector<uint8_t> out((size_t)GH * (size_t)GW * 3, 0);
  const int32_t err = f64 ? render(b64, label, mask, colors, B, S, n_colors, H, W, cols, pad, GW, out)
                          : render(b32, label, mask, colors, B, S, n_colors, H, W, cols, pad, GW, out);
  f = check_io::open_or_exit(argv[2], "wb", 1);
  check_io::write_vec(f, &err, 1);
  check_io::write_vec(f, out);
  fclose(f);
  return 0;
}
