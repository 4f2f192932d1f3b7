// Test-time augmentation of a fitted Genetic-CNN (models/cnn_fitted.py, models/cnn_ensemble.py): the views of
// a chunk of raw input images, written straight into the predictor's staging tensor.
//
// The predictor uploads R raw images [R][Hp][Wp][Cp] (the staging tensor's layout and element type: nhwc8
// bf16 / nhwc8f fp32; a short tail holds zero images). This kernel writes row v * R + r = T_v(raw[r]) of the
// staging tensor for every view v < V; the forward launches then run once over all V * R rows and
// gt_head_tta (cnn_dense.hip) averages each raw row's views.
//
// The transform is training's (cnn_augment.hip; tests/augment_ref.transform is the oracle) with the draw
// replaced by a fixed table of up to 16 views that travels by value in the arguments:
//   out[i, j, c] = raw[i - dy, f(j - dx), c] inside the real extent Hr x Wr, else 0;  f(u) = flip ? Wr-1-u : u
// Everything outside the real extent is written as zeros; channel padding is copied from the raw chunk, where
// it is zero. Rows >= V * R of the staging tensor are not touched.
//
// Pure data movement, shaped like augment_kernel: one 8-channel chunk (16 B bf16, 32 B fp32) per thread,
// consecutive threads on consecutive chunks of an output row, one workgroup column (blockIdx.x) per output
// row, so the view and its (dy, dx, flip) are wave-uniform and stay on the scalar unit.

#include <hip/hip_runtime.h>

#include "common.h"

#define TTA_BLOCK 256
#define TTA_MAXV 16

struct TtaViewArgs {
  const void* raw;           // [R][Hp][Wp][Cp], bf16 (prec 0) or fp32 (prec 1)
  void* out;                 // staging tensor [rows][Hp][Wp][Cp], same type; rows [0, V * R) are written
  int R, V, rows;
  int Hp, Wp, Hr, Wr, Cp;
  int prec;
  int dy[TTA_MAXV], dx[TTA_MAXV], flip[TTA_MAXV];
};

template <int PREC>
__global__ __launch_bounds__(TTA_BLOCK) void tta_views_kernel(const TtaViewArgs a) {
  typedef typename ActT<PREC>::T AT;
  const int vr = blockIdx.x;                       // output row v * R + r
  const int v = vr / a.R, r = vr - v * a.R;
  const int dy = a.dy[v], dx = a.dx[v];
  const bool flip = a.flip[v] != 0;

  const uint32_t CB = (uint32_t)a.Cp >> 3;
  const uint32_t chunks = (uint32_t)a.Hp * a.Wp * CB;
  const uint32_t c = blockIdx.y * TTA_BLOCK + threadIdx.x;
  if (c >= chunks) return;
  const FastDiv dcb(CB), dw((uint32_t)a.Wp);
  uint32_t px, cb, ui, uj;
  dcb.divmod(c, px, cb);
  dw.divmod(px, ui, uj);
  const int i = (int)ui, j = (int)uj;
  const int si = i - dy, u = j - dx;
  const bool ok = i < a.Hr && j < a.Wr && si >= 0 && si < a.Hr && u >= 0 && u < a.Wr;
  const int sj = flip ? a.Wr - 1 - u : u;
  AT* dst = static_cast<AT*>(a.out) + ((int64_t)vr * chunks + c) * 8;
  // dereferenced only where `ok`: the offset of a pixel outside the real extent is never formed into a load
  const int64_t so = ((((int64_t)r * a.Hp + si) * a.Wp + sj) * (int64_t)CB + cb) * 8;
  if (PREC) {
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (ok) {
      const float4* p = reinterpret_cast<const float4*>(static_cast<const AT*>(a.raw) + so);
      v0 = p[0];
      v1 = p[1];
    }
    reinterpret_cast<float4*>(dst)[0] = v0;
    reinterpret_cast<float4*>(dst)[1] = v1;
  } else {
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (ok) w = *reinterpret_cast<const uint4*>(static_cast<const AT*>(a.raw) + so);
    *reinterpret_cast<uint4*>(dst) = w;
  }
}

extern "C" {

size_t gt_sizeof_tta_view_args() { return sizeof(TtaViewArgs); }

// Returns non-zero (nothing launched) on arguments the kernel cannot run.
int gt_tta_views(const void* ap, hipStream_t s) {
  if (!ap) return -1;
  const TtaViewArgs& a = *static_cast<const TtaViewArgs*>(ap);
  if (!a.raw || !a.out) return -2;
  if (a.R <= 0 || a.rows <= 0 || a.Hp <= 0 || a.Wp <= 0 || a.Cp <= 0 || a.Cp % 8) return -3;
  if (a.Hr <= 0 || a.Wr <= 0 || a.Hr > a.Hp || a.Wr > a.Wp) return -4;
  if (a.V < 1 || a.V > TTA_MAXV) return -5;
  for (int v = 0; v < a.V; ++v) {
    // as unsigned magnitudes: |INT_MIN| does not overflow
    const long ady = a.dy[v] < 0 ? -(long)a.dy[v] : (long)a.dy[v];
    const long adx = a.dx[v] < 0 ? -(long)a.dx[v] : (long)a.dx[v];
    if (ady >= a.Hr || adx >= a.Wr) return -5;
  }
  if (a.prec != 0 && a.prec != 1) return -6;
  const long rows = (long)a.V * a.R;
  if (rows > a.rows) return -8;
  const long chunks = (long)a.Hp * a.Wp * (a.Cp / 8);
  const long dmax = a.Wp > a.Cp / 8 ? a.Wp : a.Cp / 8;
  if (chunks * dmax >= (1L << 32) || rows > 0x7fffffffL) return -7;      // FastDiv's range, grid.x
  const long gy = (chunks + TTA_BLOCK - 1) / TTA_BLOCK;
  if (gy > 65535) return -7;
  const dim3 grid((unsigned)rows, (unsigned)gy);
  if (a.prec) hipLaunchKernelGGL(tta_views_kernel<1>, grid, dim3(TTA_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(tta_views_kernel<0>, grid, dim3(TTA_BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
