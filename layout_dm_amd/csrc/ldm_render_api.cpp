// C-ABI of the layout renderer (include/ldm_hip.h, section "generated layouts as pictures"): ldm_render_layouts and
// ldm_render_grid_shape.  Handle-free like the metrics entry points: device pointers, sizes, a stream; every argument is
// checked before anything is launched.
#include "../../include/ldm_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldm_kernels.h"

#include "ldm_render_core.h"

using namespace ldm;

extern "C" int ldm_render_grid_shape(int B, int H, int W, int cols, int pad, int64_t* GH, int64_t* GW) {
  int64_t gh = 0, gw = 0;
  if (!GH || !GW || !ldm_render::grid_shape(B, H, W, cols, pad, &gh, &gw)) return -1;
  *GH = gh, *GW = gw;
  return 0;
}

extern "C" int ldm_render_layouts(const void* d_bbox, int box_f64, const int64_t* d_label, const uint8_t* d_mask, int B, int S,
                                  const uint8_t* d_colors, int n_colors, int H, int W, int cols, int pad, uint8_t* d_out,
                                  int32_t* d_err, void* stream) {
  int64_t GH = 0, GW = 0;
  if ((box_f64 != 0 && box_f64 != 1) || S < 1 || S > ldm_render::kMaxSlots || n_colors < 1) return -1;
  if (!ldm_render::grid_shape(B, H, W, cols, pad, &GH, &GW)) return -1;
  if (!d_bbox || !d_label || !d_mask || !d_colors || !d_out || !d_err) return -1;
  (void)hipGetLastError();
  if (hipMemsetAsync(d_err, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return -2;
  // the kernel writes tile pixels only: the padding and the empty tiles of a last row that is not full are cleared here
  if ((pad > 0 || B % cols != 0) && hipMemsetAsync(d_out, 0, (size_t)GH * (size_t)GW * 3, (hipStream_t)stream) != hipSuccess) return -2;
  launch_render_layouts(d_bbox, box_f64, d_label, d_mask, B, S, d_colors, n_colors, H, W, cols, pad, GW, d_out, d_err,
                        (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
