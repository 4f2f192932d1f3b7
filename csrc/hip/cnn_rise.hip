// RISE saliency (Petsiuk et al. 2018, randomized input sampling) of a fitted Genetic-CNN (models/cnn_fitted.py,
// models/cnn_ensemble.py): map[r] = inv * sum_i s_{r,i} M_i, the masks M_i weighted by the score s_{r,i} the
// model gives the target class of image r blended with M_i. Three kernels here; the scoring head gt_head_rise
// sits in cnn_dense.hip next to the heads it shares its helpers with.
//
// The masks are shared by all images: M_i is a function of (seed, i, cells, p, Hr, Wr) only (rise_masks in
// models/cnn_fitted.py is the numpy twin, tests/rise_ref.py the loop oracle). With s = cells, ch = ceil(Hr / s),
// cw = ceil(Wr / s), key = hash4(seed, i, RISE_KEY, 0):
//   grid bit g(a, b) = hash4(key, a, b, 1) < thr ? 1 : 0   for a, b in 0 .. s + 1
//   oy = hash4(key, 0, 0, 2) mod ch,  ox = hash4(key, 0, 0, 3) mod cw
//   Y = y + oy, a = Y / ch, ty = fp32(Y - a * ch) / fp32(ch); X, b, tx likewise
//   M_i[y, x] = top + ty * (bot - top), top = g(a, b) + tx * (g(a, b + 1) - g(a, b)), bot the same in row a + 1
// every product and every sum rounded separately (fp contraction off). Y <= Hr - 1 + ch - 1 < (s + 1) * ch, so
// a + 1 <= s + 1: the (s + 2)^2 bits cover every pixel.
//
//   gt_rise_views       raw fp32 images -> the launch's items in the predictor's staging tensor
//   gt_rise_masks       once per setting: the three exact bf16 planes of every mask, [3][Pp][Kp]
//   gt_rise_accumulate  D[pixel][image] = sum_k M[pixel][k] * S[image][k] on the matrix cores, times inv

#include <hip/hip_runtime.h>

#include "common.h"

#define RISE_BLOCK 256
#define RISE_KEY 0x52495345u          // "RISE": hash4 counter of the mask key
#define RISE_MAX_MASKS 8192
#define RISE_MAX_CELLS 16
#define RISE_MAXG (RISE_MAX_CELLS + 2)

__device__ __forceinline__ float rise_blend(float g00, float g01, float g10, float g11, float tx, float ty) {
#pragma clang fp contract(off)
  const float dt = g01 - g00;
  const float top = g00 + tx * dt;
  const float db = g11 - g10;
  const float bot = g10 + tx * db;
  const float d = bot - top;
  return top + ty * d;
}

// fp32(rem) / fp32(c): correctly rounded, as numpy divides
__device__ __forceinline__ float rise_frac(uint32_t rem, uint32_t c) { return (float)rem / (float)c; }

// ---------------------------------------------------------------------------------------------------------
// gt_rise_views: V_i(img)[y, x, c] = fill[c] + M_i[y, x] * (img[y, x, c] - fill[c]), converted once to the staging
// element type; zero outside the real extent and in the channel padding.
//
// The unit of work is the item w = r * masks + i; launch row j holds item w0 + j, so an image's masks may
// straddle launches and a launch may hold items of several images. With base = 1 launch row j < m is image j
// as it is. Rows whose item does not exist become zero images; exactly `rows` rows are written.
//
// Shaped like occlude_views_kernel: one workgroup column (blockIdx.x) per launch row, so the item, its image and
// its mask are wave-uniform; one 8-channel chunk per thread. The (s + 2)^2 grid bits and the two offsets of the
// row's mask are hashed once per workgroup, spread over its threads, into LDS; a pixel then costs four LDS reads
// and the blend, never a hash and never a load of a mask from memory.
// ---------------------------------------------------------------------------------------------------------
struct RiseViewArgs {
  const float* raw;          // [m][Hp][Wp][Cp] fp32; read inside the real extent of images < m only
  void* out;                 // staging tensor [cap][Hp][Wp][Cp], bf16 (prec 0) or fp32 (prec 1); rows [0, rows)
  const float* fill;         // [Cp] fp32 (channels >= Cr are not used)
  int m;                     // images in the raw buffer
  int w0;                    // first item of this launch (ignored in base mode)
  int masks, cells;
  uint32_t seed, thr;        // thr = uint32(p * 2^32)
  int rows, cap;             // rows this launch writes, rows the staging tensor holds
  int Hp, Wp, Hr, Wr, Cp, Cr;
  int prec, base;
};

template <int PREC>
__global__ __launch_bounds__(RISE_BLOCK) void rise_views_kernel(const RiseViewArgs a) {
#pragma clang fp contract(off)
  typedef typename ActT<PREC>::T AT;
  __shared__ float bits[RISE_MAXG * RISE_MAXG];
  __shared__ uint32_t off[2];
  const uint32_t j = blockIdx.x;                   // launch row
  // block-uniform: the item, its image and its mask
  const uint32_t w = a.base ? j : (uint32_t)a.w0 + j;
  const uint32_t items = a.base ? (uint32_t)a.m : (uint32_t)a.m * (uint32_t)a.masks;
  const bool live = w < items;
  const bool masked = live && !a.base;
  const uint32_t gs = (uint32_t)a.cells + 2u;
  const uint32_t ch = ((uint32_t)a.Hr + a.cells - 1) / (uint32_t)a.cells;
  const uint32_t cw = ((uint32_t)a.Wr + a.cells - 1) / (uint32_t)a.cells;
  uint32_t r = w;
  if (masked) {
    r = w / (uint32_t)a.masks;
    const uint32_t i = w - r * (uint32_t)a.masks;
    const uint32_t key = hash4(a.seed, i, RISE_KEY, 0u);
    for (uint32_t t = threadIdx.x; t < gs * gs; t += RISE_BLOCK) {
      const uint32_t ga = t / gs, gb = t - ga * gs;
      bits[t] = hash4(key, ga, gb, 1u) < a.thr ? 1.f : 0.f;
    }
    if (threadIdx.x == RISE_BLOCK - 1) off[0] = hash4(key, 0u, 0u, 2u) % ch;
    if (threadIdx.x == RISE_BLOCK - 2) off[1] = hash4(key, 0u, 0u, 3u) % cw;
  }
  __syncthreads();                                 // reached by every thread of the block

  const uint32_t CB = (uint32_t)a.Cp >> 3;
  const uint32_t chunks = (uint32_t)a.Hp * a.Wp * CB;
  const uint32_t c = blockIdx.y * RISE_BLOCK + threadIdx.x;
  if (c >= chunks) return;
  const FastDiv dcb(CB), dw((uint32_t)a.Wp);
  uint32_t px, cb, y, x;
  dcb.divmod(c, px, cb);
  dw.divmod(px, y, x);
  const bool real = live && (int)y < a.Hr && (int)x < a.Wr;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 0.f;
  if (real) {
    // dereferenced only where `real`: a pixel outside the real extent, or of an image past m, is never loaded
    float img[8];
    load8f(a.raw + ((int64_t)r * chunks + c) * 8, img);
    float mk = 1.f;
    if (masked) {
      const uint32_t Y = y + off[0], X = x + off[1];
      const uint32_t ga = Y / ch, gb = X / cw;
      const float ty = rise_frac(Y - ga * ch, ch), tx = rise_frac(X - gb * cw, cw);
      const float* g = bits + ga * gs + gb;
      mk = rise_blend(g[0], g[1], g[gs], g[gs + 1], tx, ty);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int cc = (int)cb * 8 + e;
      const float f = a.fill[min(cc, a.Cr - 1)];
      const float d = img[e] - f;
      const float t = mk * d;
      const float blended = f + t;
      v[e] = cc < a.Cr ? (masked ? blended : img[e]) : 0.f;
    }
  }
  st_chunk(static_cast<AT*>(a.out) + ((int64_t)j * chunks + c) * 8, v);
}

// ---------------------------------------------------------------------------------------------------------
// gt_rise_masks, once per setting: the three exact bf16 planes of every mask (split8: M = p0 + p1 + p2),
// transposed for the GEMM as [3][Pp][Kp] -- pixel-major, the mask index contiguous, so one lane's 8 consecutive k
// of a pixel are one 16-byte load per plane. Pixels >= Hr * Wr and masks >= masks are zero planes. One thread per
// (pixel, 8 masks), consecutive threads on consecutive chunks of a pixel's row; every value hashes its own four
// bits and offsets (the cost of a setting, not of a call).
// ---------------------------------------------------------------------------------------------------------
struct RiseMaskArgs {
  uint16_t* planes;          // [3][Pp][Kp] bf16
  int masks, Kp, cells;
  uint32_t seed, thr;
  int Hr, Wr, Pp;
};

__global__ __launch_bounds__(RISE_BLOCK) void rise_masks_kernel(const RiseMaskArgs a) {
  const uint32_t KB = (uint32_t)a.Kp >> 3;
  const int64_t idx = (int64_t)blockIdx.x * RISE_BLOCK + threadIdx.x;
  if (idx >= (int64_t)a.Pp * KB) return;
  const uint32_t pix = (uint32_t)(idx / KB), kc = (uint32_t)(idx - (int64_t)pix * KB);
  const uint32_t ch = ((uint32_t)a.Hr + a.cells - 1) / (uint32_t)a.cells;
  const uint32_t cw = ((uint32_t)a.Wr + a.cells - 1) / (uint32_t)a.cells;
  const uint32_t y = pix / (uint32_t)a.Wr, x = pix - y * (uint32_t)a.Wr;
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t i = kc * 8 + e;
    f[e] = 0.f;
    if (pix < (uint32_t)a.Hr * a.Wr && i < (uint32_t)a.masks) {
      const uint32_t key = hash4(a.seed, i, RISE_KEY, 0u);
      const uint32_t Y = y + hash4(key, 0u, 0u, 2u) % ch, X = x + hash4(key, 0u, 0u, 3u) % cw;
      const uint32_t ga = Y / ch, gb = X / cw;
      const float g00 = hash4(key, ga, gb, 1u) < a.thr ? 1.f : 0.f;
      const float g01 = hash4(key, ga, gb + 1, 1u) < a.thr ? 1.f : 0.f;
      const float g10 = hash4(key, ga + 1, gb, 1u) < a.thr ? 1.f : 0.f;
      const float g11 = hash4(key, ga + 1, gb + 1, 1u) < a.thr ? 1.f : 0.f;
      f[e] = rise_blend(g00, g01, g10, g11, rise_frac(X - gb * cw, cw), rise_frac(Y - ga * ch, ch));
    }
  }
  uint4 q[3];
  split8(f, q[0], q[1], q[2]);
  const int64_t plane = (int64_t)a.Pp * a.Kp;
#pragma unroll
  for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(a.planes + p * plane + (int64_t)pix * a.Kp + kc * 8) = q[p];
}

// ---------------------------------------------------------------------------------------------------------
// gt_rise_accumulate: out[image][pixel] = inv * sum_k M[pixel][k] * S[image][k], the fp32 product on the bf16
// matrix cores through common.h's exact three-plane split (six v_mfma_f32_16x16x32_bf16 per 32-deep k-step).
//
// A workgroup of 4 waves owns 64 pixels x 32 images; grid (Pp / 64, ceil(m / 32)). Wave w owns pixels
// 16w .. 16w + 15 of the tile as the rows of D and both 16-image tiles as its columns. Per 32-mask k-step:
//   A  lane (l16, kq) loads the 8 masks kq * 8 .. + 7 of pixel l16 straight from the planes in global memory
//      (one 16-byte load per plane, prefetched one k-step ahead): no wave shares a pixel, so LDS would add a
//      round trip and no reuse;
//   B  the [32 images][32 masks] tile of S is what all four waves share: threads 0..127 load 8 scores each, split
//      them (split8) and store the three planes into LDS, double-buffered -- step k + 1 is staged while step k
//      multiplies, one barrier per step. Images >= m are never loaded: their columns are zeros.
// The leading term a0 b0 and the five small terms accumulate apart and join after the last k-step (gt_head_mc
// records why: the sum of full size is rounded once per k-step, not six times). One fixed k order, no split-K,
// no atomics: a column depends on its own row of S only, so a map does not depend on the images beside it.
// ---------------------------------------------------------------------------------------------------------
#define RISE_LD 40           // bf16 per image row of a staged plane: 32 masks + 8 of padding (80 B, 16 B aligned)

struct RiseAccArgs {
  const uint16_t* planes;    // [3][Pp][Kp] bf16 (gt_rise_masks)
  const float* S;            // [>= m][Kp] fp32 scores; entries [masks, Kp) of a row are finite (zero)
  float* out;                // [m][P] fp32
  int m, masks, Kp;
  int P, Pp;                 // real pixels Hr * Wr, rounded up to 64
  float inv;                 // fp32 1 / (masks * p)
};

__global__ __launch_bounds__(256) void rise_accumulate_kernel(const RiseAccArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t sl[2][3][32 * RISE_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4, l16 = lane & 15;
  const int64_t pix = (int64_t)blockIdx.x * 64 + wave * 16 + l16;          // < Pp: the planes hold it
  const int c0 = blockIdx.y * 32;
  const int64_t plane = (int64_t)a.Pp * a.Kp;
  const uint16_t* ap = a.planes + pix * a.Kp + kq * 8;
  // staging role of threads 0..127: image si of the tile, masks sk .. sk + 7 of the k-step
  const int si = tid >> 2, sk = (tid & 3) * 8;
  const bool stager = tid < 128;
  const bool sok = stager && c0 + si < a.m;
  const float* sp = a.S + (int64_t)min(c0 + si, a.m - 1) * a.Kp + sk;
  const int nk = a.Kp >> 5;

  f32x4_t acc[2], lo[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) acc[t] = lo[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  uint4 af[3], an[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) af[p] = an[p] = *reinterpret_cast<const uint4*>(ap + p * plane);
  if (stager) {
    float f[8];
    uint4 q[3];
    load8f_or0(sp, sok, f);
    split8(f, q[0], q[1], q[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(&sl[0][p][si * RISE_LD + sk]) = q[p];
  }
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const int cur = ks & 1;
    if (ks + 1 < nk) {                                                     // block-uniform
#pragma unroll
      for (int p = 0; p < 3; ++p) an[p] = *reinterpret_cast<const uint4*>(ap + p * plane + (ks + 1) * 32);
      if (stager) {
        float f[8];
        uint4 q[3];
        load8f_or0(sp + (ks + 1) * 32, sok, f);
        split8(f, q[0], q[1], q[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(&sl[cur ^ 1][p][si * RISE_LD + sk]) = q[p];
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      uint4 bf[3];
#pragma unroll
      for (int p = 0; p < 3; ++p)
        bf[p] = *reinterpret_cast<const uint4*>(&sl[cur][p][(t * 16 + l16) * RISE_LD + kq * 8]);
      lo[t] = mfma16(af[2], bf[0], lo[t]);                                 // D[row = pixel][col = image];
      lo[t] = mfma16(af[1], bf[1], lo[t]);                                 // mfma_np<3>'s terms, smallest first
      lo[t] = mfma16(af[0], bf[2], lo[t]);
      lo[t] = mfma16(af[1], bf[0], lo[t]);
      lo[t] = mfma16(af[0], bf[1], lo[t]);
      acc[t] = mfma16(af[0], bf[0], acc[t]);
    }
    __syncthreads();               // buffer `cur` is free for step ks + 2, buffer `cur ^ 1` is complete
#pragma unroll
    for (int p = 0; p < 3; ++p) af[p] = an[p];
  }
  // lane (l16, kq) holds pixels kq * 4 .. + 3 of the wave's 16 for image l16 of each tile
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int img = c0 + t * 16 + l16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t p = (int64_t)blockIdx.x * 64 + wave * 16 + kq * 4 + i;
      float v;
      {
#pragma clang fp contract(off)
        const float sum = acc[t][i] + lo[t][i];
        v = sum * a.inv;
      }
      if (img < a.m && p < a.P) a.out[(int64_t)img * a.P + p] = v;
    }
  }
}

static bool rise_setting_ok(int masks, int cells, int Hr, int Wr) {
  if (masks < 1 || masks > RISE_MAX_MASKS) return false;
  if (Hr < 1 || Wr < 1) return false;
  return cells >= 2 && cells <= RISE_MAX_CELLS && cells <= (Hr < Wr ? Hr : Wr);
}

extern "C" {

size_t gt_sizeof_rise_view_args() { return sizeof(RiseViewArgs); }
size_t gt_sizeof_rise_mask_args() { return sizeof(RiseMaskArgs); }
size_t gt_sizeof_rise_acc_args() { return sizeof(RiseAccArgs); }
int gt_rise_max_masks() { return RISE_MAX_MASKS; }
int gt_rise_max_cells() { return RISE_MAX_CELLS; }

// Every launcher returns a negative code (nothing launched) on arguments its kernel cannot run.
int gt_rise_views(const void* ap, hipStream_t s) {
  if (!ap) return -1;
  const RiseViewArgs& a = *static_cast<const RiseViewArgs*>(ap);
  if (!a.raw || !a.out || !a.fill) return -2;
  if (a.m <= 0 || a.rows <= 0 || a.Hp <= 0 || a.Wp <= 0 || a.Cp <= 0 || a.Cp % 8) return -3;
  if (a.Hr <= 0 || a.Wr <= 0 || a.Hr > a.Hp || a.Wr > a.Wp || a.Cr < 1 || a.Cr > a.Cp) return -4;
  if (!rise_setting_ok(a.masks, a.cells, a.Hr, a.Wr)) return -5;
  if (a.prec != 0 && a.prec != 1) return -6;
  if (a.base != 0 && a.base != 1) return -6;
  if (a.w0 < 0 || a.rows > a.cap) return -8;
  // the items of the launch and of the raw buffer as 32-bit numbers
  if ((long)a.m * a.masks > 0x7fffffffL || (long)a.w0 + a.rows > 0x7fffffffL) return -7;
  const long chunks = (long)a.Hp * a.Wp * (a.Cp / 8);
  const long dmax = a.Wp > a.Cp / 8 ? a.Wp : a.Cp / 8;
  if (chunks * dmax >= (1L << 32)) return -7;                              // FastDiv's range
  const long gy = (chunks + RISE_BLOCK - 1) / RISE_BLOCK;
  if (gy > 65535) return -7;
  const dim3 grid((unsigned)a.rows, (unsigned)gy);
  if (a.prec) hipLaunchKernelGGL(rise_views_kernel<1>, grid, dim3(RISE_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(rise_views_kernel<0>, grid, dim3(RISE_BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

int gt_rise_masks(const void* ap, hipStream_t s) {
  if (!ap) return -1;
  const RiseMaskArgs& a = *static_cast<const RiseMaskArgs*>(ap);
  if (!a.planes) return -2;
  if (!rise_setting_ok(a.masks, a.cells, a.Hr, a.Wr)) return -5;
  if (a.Kp != (a.masks + 31) / 32 * 32) return -3;
  const long P = (long)a.Hr * a.Wr;
  if (P > 0x7fffffffL - 64 || a.Pp != (P + 63) / 64 * 64) return -4;
  const long blocks = ((long)a.Pp * (a.Kp / 8) + RISE_BLOCK - 1) / RISE_BLOCK;
  if (blocks > 0x7fffffffL) return -7;
  hipLaunchKernelGGL(rise_masks_kernel, dim3((unsigned)blocks), dim3(RISE_BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

int gt_rise_accumulate(const void* ap, hipStream_t s) {
  if (!ap) return -1;
  const RiseAccArgs& a = *static_cast<const RiseAccArgs*>(ap);
  if (!a.planes || !a.S || !a.out) return -2;
  if (a.masks < 1 || a.masks > RISE_MAX_MASKS || a.Kp != (a.masks + 31) / 32 * 32) return -3;
  if (a.P < 1 || a.P > 0x7fffffff - 64 || a.Pp != (a.P + 63) / 64 * 64) return -4;
  if (a.m < 1 || (long)a.m * a.masks > 0x7fffffffL) return -7;
  if (!(a.inv > 0.f) || a.inv > 3.4e38f) return -5;                        // a finite positive number
  const long gy = ((long)a.m + 31) / 32;
  if (gy > 65535) return -7;
  hipLaunchKernelGGL(rise_accumulate_kernel, dim3((unsigned)(a.Pp / 64), (unsigned)gy), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
