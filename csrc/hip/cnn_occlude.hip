// Occlusion sensitivity of a fitted Genetic-CNN (models/cnn_fitted.py, models/cnn_ensemble.py): the occluded
// copies of a group of raw input images, written straight into the predictor's staging tensor.
//
// The predictor uploads m raw images [m][Hp][Wp][Cp] once (the staging tensor's layout and element type: nhwc8
// bf16 / nhwc8f fp32; zero outside the real extent and in the channel padding). The unit of work is the item
// w = r * Cc + cell: image r with cell (gi, gj) = (cell / Gw, cell % Gw) of the occlusion grid replaced by the
// fill value. Items are packed densely into launches: launch row j holds item w0 + j, whatever the ratio of
// Cc to the launch's rows, so an image's cells may straddle launches and a launch may hold cells of several
// images. The forward launches then run over all rows and gt_head_occlusion (cnn_dense.hip) turns each row
// into one element of the map.
//
//   out[j][i, k, c] = fill[c]        for (i, k) in rows [gi*stride, min(gi*stride + patch, Hr)) x the same in k
//                   = raw[r][i, k, c] elsewhere inside the real extent Hr x Wr
//                   = 0              outside the real extent (raw is never loaded there)
// (tests/occlusion_ref.py is the oracle). With base = 1 launch row j < m is the plain copy of image j. Rows
// whose item does not exist (w >= m * Cc; j >= m in base mode) become zero images; exactly `rows` rows are
// written. `fill` holds Cp elements of the staging type, zero in the channel padding.
//
// Pure data movement, shaped like tta_views_kernel: one 8-channel chunk (16 B bf16, 32 B fp32) per thread,
// consecutive threads on consecutive chunks of an output row, one workgroup column (blockIdx.x) per output
// row, so the image, the cell and its rectangle are wave-uniform and stay on the scalar unit.

#include <hip/hip_runtime.h>

#include "common.h"

#define OCC_BLOCK 256
#define OCC_MAX_CELLS 4096

struct OccludeArgs {
  const void* raw;           // [m][Hp][Wp][Cp], bf16 (prec 0) or fp32 (prec 1)
  void* out;                 // staging tensor [cap][Hp][Wp][Cp], same type; rows [0, rows) are written
  const void* fill;          // [Cp], same type
  int m;                     // images in the raw buffer
  int w0;                    // first item of this launch (ignored in base mode)
  int Cc, Gw;                // cells per image, cells per grid row
  int patch, stride;
  int rows, cap;             // rows this launch writes, rows the staging tensor holds
  int Hp, Wp, Hr, Wr, Cp;
  int prec, base;
};

template <int PREC>
__global__ __launch_bounds__(OCC_BLOCK) void occlude_views_kernel(const OccludeArgs a) {
  typedef typename ActT<PREC>::T AT;
  const uint32_t j = blockIdx.x;                   // launch row
  // wave-uniform: the item, its image and its rectangle [y0, y1) x [x0, x1) (empty in base mode)
  const uint32_t w = a.base ? j : (uint32_t)a.w0 + j;
  const uint32_t items = a.base ? (uint32_t)a.m : (uint32_t)a.m * (uint32_t)a.Cc;
  const bool live = w < items;
  uint32_t r = w;
  int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  if (live && !a.base) {
    r = w / (uint32_t)a.Cc;
    const uint32_t cell = w - r * (uint32_t)a.Cc;
    const uint32_t gi = cell / (uint32_t)a.Gw, gj = cell - gi * (uint32_t)a.Gw;
    y0 = (int)gi * a.stride;
    x0 = (int)gj * a.stride;
    y1 = min(y0 + a.patch, a.Hr);
    x1 = min(x0 + a.patch, a.Wr);
  }

  const uint32_t CB = (uint32_t)a.Cp >> 3;
  const uint32_t chunks = (uint32_t)a.Hp * a.Wp * CB;
  const uint32_t c = blockIdx.y * OCC_BLOCK + threadIdx.x;
  if (c >= chunks) return;
  const FastDiv dcb(CB), dw((uint32_t)a.Wp);
  uint32_t px, cb, ui, uk;
  dcb.divmod(c, px, cb);
  dw.divmod(px, ui, uk);
  const int i = (int)ui, k = (int)uk;
  const bool real = live && i < a.Hr && k < a.Wr;
  const bool cover = real && i >= y0 && i < y1 && k >= x0 && k < x1;
  // dereferenced only where `real`: a pixel outside the real extent, or of an image past m, is never loaded
  const AT* src = cover ? static_cast<const AT*>(a.fill) + (int64_t)cb * 8
                        : static_cast<const AT*>(a.raw) + ((int64_t)r * chunks + c) * 8;
  AT* dst = static_cast<AT*>(a.out) + ((int64_t)j * chunks + c) * 8;
  if (PREC) {
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (real) {
      const float4* p = reinterpret_cast<const float4*>(src);
      v0 = p[0];
      v1 = p[1];
    }
    reinterpret_cast<float4*>(dst)[0] = v0;
    reinterpret_cast<float4*>(dst)[1] = v1;
  } else {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (real) v = *reinterpret_cast<const uint4*>(src);
    *reinterpret_cast<uint4*>(dst) = v;
  }
}

extern "C" {

size_t gt_sizeof_occlude_args() { return sizeof(OccludeArgs); }
int gt_occlude_max_cells() { return OCC_MAX_CELLS; }

// Returns non-zero (nothing launched) on arguments the kernel cannot run.
int gt_occlude_views(const void* ap, hipStream_t s) {
  if (!ap) return -1;
  const OccludeArgs& a = *static_cast<const OccludeArgs*>(ap);
  if (!a.raw || !a.out || !a.fill) return -2;
  if (a.m <= 0 || a.rows <= 0 || a.Hp <= 0 || a.Wp <= 0 || a.Cp <= 0 || a.Cp % 8) return -3;
  if (a.Hr <= 0 || a.Wr <= 0 || a.Hr > a.Hp || a.Wr > a.Wp) return -4;
  if (a.patch < 1 || a.patch > (a.Hr < a.Wr ? a.Hr : a.Wr) || a.stride < 1 || a.stride > a.patch) return -5;
  const long Gh = (a.Hr - a.patch + a.stride - 1) / a.stride + 1;
  const long Gw = (a.Wr - a.patch + a.stride - 1) / a.stride + 1;
  if (Gh * Gw > OCC_MAX_CELLS || a.Gw != Gw || a.Cc != Gh * Gw) return -5;
  if (a.prec != 0 && a.prec != 1) return -6;
  if (a.base != 0 && a.base != 1) return -6;
  if (a.w0 < 0 || a.rows > a.cap) return -8;
  // the items of the launch and of the raw buffer as 32-bit numbers
  if ((long)a.m * a.Cc > 0x7fffffffL || (long)a.w0 + a.rows > 0x7fffffffL) return -7;
  const long chunks = (long)a.Hp * a.Wp * (a.Cp / 8);
  const long dmax = a.Wp > a.Cp / 8 ? a.Wp : a.Cp / 8;
  if (chunks * dmax >= (1L << 32)) return -7;                              // FastDiv's range
  const long gy = (chunks + OCC_BLOCK - 1) / OCC_BLOCK;
  if (gy > 65535) return -7;
  const dim3 grid((unsigned)a.rows, (unsigned)gy);
  if (a.prec) hipLaunchKernelGGL(occlude_views_kernel<1>, grid, dim3(OCC_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(occlude_views_kernel<0>, grid, dim3(OCC_BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
