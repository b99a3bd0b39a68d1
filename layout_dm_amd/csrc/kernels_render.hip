// Generated layouts as pictures on the device (convert_layout_to_image / save_image, trainer/helpers/visualization.py:17-115,
// called at trainer/test.py:205-214).  The arithmetic is the one source of ldm_render_core.h (also compiled for the host:
// tests/cpu_render_check.cpp).
//
// One workgroup per layout.  Thread t takes element slot t: mask, box and label are checked (a box that is not finite or
// has a negative w or h, a label without a colour: *err, and the element is not drawn — nothing is read from `colors`
// outside its n_colors rows), its pixel rectangle, area and colour go to registers, the areas to LDS.  Every drawn element
// then finds its place in the drawing order by counting (descending area, stable) and writes rectangle and colour to that
// place of the LDS list.  After that each thread OWNS pixels: it starts from white, walks the list in order with the pixel's
// three channels in registers (all lanes read the same LDS entry: a broadcast), and stores the pixel once.  Ownership makes
// the order of blends exact without atomics.
//
// The destination is a tile of a mosaic: layout k goes to rows oy .. oy + H - 1, columns ox .. ox + W - 1 of a (GH, GW, 3)
// uint8 image with (oy, ox) = ldm_render::tile_origin.  cols = 1, pad = 0 is the batch form (B, H, W, 3).  Only tile pixels
// are written: the caller clears the padding.
#include "ldm_kernels.h"
#include "ldm_render_core.h"

namespace ldm {

namespace {

constexpr int kRenderBlock = ldm_render::kMaxSlots;  // one thread per element slot in the ranking phase

template <typename TB>
__global__ __launch_bounds__(kRenderBlock) void render_layouts_k(const TB* __restrict__ bbox, const int64_t* __restrict__ label,
                                                                 const uint8_t* __restrict__ mask, int S,
                                                                 const uint8_t* __restrict__ colors, int n_colors, int H, int W,
                                                                 int cols, int pad, int64_t GW, uint8_t* __restrict__ out,
                                                                 int32_t* __restrict__ err) {
  __shared__ TB s_area[kRenderBlock];
  __shared__ uint8_t s_drawn[kRenderBlock];
  __shared__ ldm_render::Rect s_rect[kRenderBlock];
  __shared__ uint32_t s_colour[kRenderBlock];
  const int k = blockIdx.x, t = threadIdx.x;
  const size_t row = (size_t)k * S + t;
  bool drawn = false;
  int bad = 0;
  TB area = TB(0);
  ldm_render::Rect r{0, 0, 0, 0};
  uint32_t colour = 0;
  if (t < S && mask[row] != 0) {
    const TB* p = bbox + 4 * row;
    const TB b[4] = {p[0], p[1], p[2], p[3]};
    const int64_t lab = label[row];
    if (!ldm_render::box_ok(b)) bad |= ldm_render::kErrBox;
    if (lab < 0 || lab >= n_colors) bad |= ldm_render::kErrLabel;
    if (!bad) {
      drawn = true;
      r = ldm_render::rect_of(b, H, W);
      area = ldm_render::area_of(b);
      colour = ldm_render::pack_colour(colors + 3 * lab);
    }
  }
  s_area[t] = area;
  s_drawn[t] = drawn ? 1 : 0;
  if (bad) atomicOr(err, bad);
  const int n = __syncthreads_count(drawn ? 1 : 0);
  if (drawn) {
    const int at = ldm_render::rank_of(s_area, s_drawn, S, t);
    s_rect[at] = r;
    s_colour[at] = colour;
  }
  __syncthreads();

  int64_t oy, ox;
  ldm_render::tile_origin(k, H, W, cols, pad, &oy, &ox);
  const int n_pix = H * W;
  for (int px = t; px < n_pix; px += kRenderBlock) {
    const int y = px / W, x = px - y * W;
    uint32_t rgb[3] = {255, 255, 255};
    for (int e = 0; e < n; ++e) ldm_render::paint(rgb, ldm_render::classify(x, y, s_rect[e]), s_colour[e]);
    uint8_t* o = out + ((oy + y) * GW + ox + x) * 3;
    o[0] = (uint8_t)rgb[0], o[1] = (uint8_t)rgb[1], o[2] = (uint8_t)rgb[2];
  }
}

}  // namespace

void launch_render_layouts(const void* bbox, int box_f64, const int64_t* label, const uint8_t* mask, int B, int S,
                           const uint8_t* colors, int n_colors, int H, int W, int cols, int pad, int64_t GW, uint8_t* out,
                           int32_t* err, hipStream_t st) {
  if (box_f64)
    hipLaunchKernelGGL(render_layouts_k<double>, dim3((unsigned)B), dim3(kRenderBlock), 0, st, static_cast<const double*>(bbox),
                       label, mask, S, colors, n_colors, H, W, cols, pad, GW, out, err);
  else
    hipLaunchKernelGGL(render_layouts_k<float>, dim3((unsigned)B), dim3(kRenderBlock), 0, st, static_cast<const float*>(bbox),
                       label, mask, S, colors, n_colors, H, W, cols, pad, GW, out, err);
}

}  // namespace ldm
