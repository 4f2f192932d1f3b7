// Noise-averaged input gradients of a fitted Genetic-CNN (models/cnn_fitted.py SaliencyState, smooth=):
// SmoothGrad, SmoothGrad^2 and VarGrad. The evaluation-mode backward chain of cnn_saliency.hip runs unchanged over
// S Gaussian points per image; the two kernels here sit in front of it and behind it.
//
//   gt_sg_points   the S noisy copies of a raw chunk, drawn on the device, raw chunk -> staging rows
//   gt_sg_reduce   the sample statistics of the points' gradients (ordered s1 and s2, mean / mean of squares /
//                  variance), the method factor, the members' weighted mean and the channel reduction
//
// The draw (numpy twin: utils/rng.sg_noise). For image n (its index within the call), sample k, real pixel
// p = i * Wr + j and real channel c:
//     r_j = hash4(seed ^ SG_KEY, n, k, (p * 4 + c) * 2 + j)            j = 0, 1
//     u_j = ((r_j >> 9) * 2 + 1) * 2^-24                                exact in fp32, inside (0, 1)
//     z   = sqrt(-2 ln u_0) * cos(2 pi u_1)                             |z| <= 5.77
//     x_k = x + sigma[n] * z                                            product and sum rounded separately
// so a value depends on (seed, n, k, p, c) alone: not on the chunk, the row position or the launch geometry.
//
// gt_sg_points, work split. The grid is (staging row, block of 256 real pixels): k, r, the image index n0 + r and
// sigma[r] are functions of blockIdx.x, so they and the first three of hash4's four mixing rounds -- which see
// (seed, n, k) only -- are wave-uniform and stay on the scalar unit, as augment_kernel keeps its draws. What is
// left per value on the vector unit is one mixing round per hash (two per value), a log, a square root and a
// cosine, against a 16- or 32-byte store per pixel.
//   * Pixels per thread: one. A thread already carries Cr (up to 3) independent values, which is enough
//     instruction-level parallelism to cover the transcendental latencies; more pixels per thread would only
//     shrink a grid that at 32 x 32 x 256 rows is 1024 workgroups, four per CU, and would turn the coalesced
//     chunk-per-lane store into a strided one.
//   * Both Box-Muller outputs: not used. The sine would halve the hashes, logs and roots, but a pair then spans
//     two channels or -- with 1 or 3 real channels -- two pixels, so a value would no longer be a function of its
//     own (p, c), the twin would have to pair the same way, and odd counts need a tail rule. The kernel runs once
//     per chunk, in front of S forward and backward chains: measured at 32 x 32 x 3 and 256 rows it takes 6.3 us
//     of a chunk's 1.2 ms (profiles/cnn_smoothgrad.txt), so the simpler rule stays.
//   * cos(2 pi u) is taken as cospi(2 u): 2 u is exact, so no rounding of 2 pi u enters, and no large-argument
//     reduction is needed. logf, sqrtf and cospif are the library's accurate versions, not the hardware's
//     approximate transcendentals: the test holds |z - z64| to four times the error of an fp32 numpy evaluation.
// The staging chunk is read, its real channels replaced and written back: padded channels, padded pixels and the
// rows >= S * R keep their bytes (gt_ig_points' contract). The raw chunk's padded pixels are never read.
//
// gt_sg_reduce, work split. The grid is (raw row, block of 256 real pixels); one thread owns one pixel of one
// image for every member. Per member it walks the S gradients of its pixel in ascending k with one 16-byte load
// each (the real channels are the first 3 of the 8-channel chunk; consecutive lanes read consecutive 32-byte
// chunks), keeping s1 and s2 of the Cr channels in registers. Every operation is rounded separately (fp
// contraction off), so fp32 numpy reproduces the result bit for bit (models/cnn_fitted.py smooth_finish).
#include "common.h"

#define SG_MAXS 64              // samples per image at most (SAL_MAX_STEPS)
#define SG_KEY 0x534D4752u      // "SMGR": xor of the seed in the draw key
#define SG_C8 8
#define SG_MAXCR 3
#define SG_BLOCK 256

struct SgPointsArgs {
  const void* raw;       // [R][Hp][Wp][C8] the clean images, staging layout and type
  void* out;             // [rows][Hp][Wp][C8] the staging tensor
  const float* sigma;    // [R] fp32(noise) * (max - min) of every image, from the host
  int R, S, rows;
  int n0;                // index within the call of the chunk's first image
  unsigned seed;
  int Hp, Wp, Hr, Wr, Cr;
  int prec;
};

template <int PREC>
__global__ void __launch_bounds__(SG_BLOCK) sg_points_kernel(SgPointsArgs a) {
#pragma clang fp contract(off)
  typedef typename ActT<PREC>::T AT;
  // ---- wave-uniform: the staging row, its image and sample, the first three rounds of the hash
  const int row = blockIdx.x;
  const int k = row / a.R, r = row - k * a.R;
  const float sg = a.sigma[r];
  uint32_t h = mix32((a.seed ^ SG_KEY) ^ 0x9e3779b9U);
  h = mix32(h ^ (uint32_t)(a.n0 + r));
  h = mix32(h ^ ((uint32_t)k * 0x85ebca6bU));
  // ---- this thread's real pixel
  const int px = blockIdx.y * SG_BLOCK + threadIdx.x;
  if (px >= a.Hr * a.Wr) return;
  const int i = px / a.Wr, j = px - i * a.Wr;
  const long pix = ((long)i * a.Wp + j) * SG_C8, img = (long)a.Hp * a.Wp * SG_C8;
  float v[8], o[8];
  ld_chunk(static_cast<const AT*>(a.raw) + r * img + pix, v);
  AT* dst = static_cast<AT*>(a.out) + row * img + pix;
  ld_chunk(dst, o);
#pragma unroll
  for (int c = 0; c < SG_MAXCR; ++c) {
    if (c < a.Cr) {
      const uint32_t d = ((uint32_t)px * 4u + (uint32_t)c) * 2u;
      const uint32_t r0 = mix32(h ^ (d * 0xc2b2ae35U));
      const uint32_t r1 = mix32(h ^ ((d + 1u) * 0xc2b2ae35U));
      const float u0 = (float)((r0 >> 9) * 2u + 1u) * 0x1p-24f;
      const float u1 = (float)((r1 >> 9) * 2u + 1u) * 0x1p-24f;
      const float rad = sqrtf(-2.f * logf(u0));
      const float z = rad * cospif(2.f * u1);
      const float nz = sg * z;
      o[c] = v[c] + nz;
    }
  }
  st_chunk(dst, o);
}

// Per raw row r, real pixel and channel c < Cr, for every member g in order, with d_k = dx[g][k * R + r]:
//   s1   = d_0, then s1 + d_k for k = 1 .. S - 1            s2 = d_0 * d_0, then s2 + d_k * d_k
//   mean = s1 * inv_s                                        msq = s2 * inv_s
//   a_g  = mean                          stat 0 (SmoothGrad)
//          msq                           stat 1 (SmoothGrad^2)
//          max(msq - mean * mean, 0)     stat 2 (VarGrad)
//   method 1 (gradient x input): a_g * x for stat 0, a_g * (x * x) for stats 1 and 2, x the clean image
//   v    = w[0] * a_0, then v + w[g] * a_g                                     (ensemble_mean's rounding)
// and gt_ig_reduce's channel reduction and output layouts: 0 signed [R][Hr][Wr][Cr]; 1 max_c |v| [R][Hr][Wr];
// 2 v_0 + v_1 + ... in channel order.
struct SgReduceArgs {
  const float* dx;       // [G][B][Hp][Wp][C8] fp32 from gt_conv_in_dgrad
  const void* x;         // [>= R][Hp][Wp][C8] the clean images, staging layout and type
  const float* weight;   // [G]
  float* out;
  int G, B, R, S;
  int Hp, Wp, Hr, Wr, Cr;
  int stat, method, reduce, prec;
  float inv_s;           // fp32(1) / fp32(S) from the host
};

template <int PREC>
__global__ void __launch_bounds__(SG_BLOCK) sg_reduce_kernel(SgReduceArgs a) {
#pragma clang fp contract(off)
  typedef typename ActT<PREC>::T AT;
  const int r = blockIdx.x;
  const int px = blockIdx.y * SG_BLOCK + threadIdx.x;
  const int per = a.Hr * a.Wr;
  if (px >= per) return;
  const int i = px / a.Wr, j = px - i * a.Wr;
  const long pix = ((long)i * a.Wp + j) * SG_C8, img = (long)a.Hp * a.Wp * SG_C8;
  const long kstride = (long)a.R * img;
  float f[SG_MAXCR] = {1.f, 1.f, 1.f};                       // the method factor of every channel
  if (a.method == 1) {
    float xv[8];
    ld_chunk(static_cast<const AT*>(a.x) + r * img + pix, xv);
#pragma unroll
    for (int c = 0; c < SG_MAXCR; ++c) f[c] = a.stat == 0 ? xv[c] : xv[c] * xv[c];
  }
  float v[SG_MAXCR] = {0.f, 0.f, 0.f};
  for (int g = 0; g < a.G; ++g) {
    const float* d = a.dx + ((long)g * a.B + r) * img + pix;
    const float wg = a.weight[g];
    float4 q = *reinterpret_cast<const float4*>(d);
    float s1[SG_MAXCR] = {q.x, q.y, q.z};
    float s2[SG_MAXCR] = {q.x * q.x, q.y * q.y, q.z * q.z};
    for (int k = 1; k < a.S; ++k) {
      q = *reinterpret_cast<const float4*>(d + k * kstride);
      const float e[SG_MAXCR] = {q.x, q.y, q.z};
#pragma unroll
      for (int c = 0; c < SG_MAXCR; ++c) {
        const float sq = e[c] * e[c];
        s1[c] = s1[c] + e[c];
        s2[c] = s2[c] + sq;
      }
    }
#pragma unroll
    for (int c = 0; c < SG_MAXCR; ++c) {
      const float mean = s1[c] * a.inv_s, msq = s2[c] * a.inv_s;
      float at = mean;
      if (a.stat == 1) {
        at = msq;
      } else if (a.stat == 2) {
        const float m2 = mean * mean;
        at = fmaxf(msq - m2, 0.f);
      }
      if (a.method == 1) at = at * f[c];
      const float term = wg * at;
      v[c] = g == 0 ? term : v[c] + term;
    }
  }
  const long idx = (long)r * per + px;
  if (a.reduce == 0) {
    for (int c = 0; c < a.Cr; ++c) a.out[idx * a.Cr + c] = v[c];
  } else if (a.reduce == 1) {
    float mx = fabsf(v[0]);
    for (int c = 1; c < a.Cr; ++c) mx = fmaxf(mx, fabsf(v[c]));
    a.out[idx] = mx;
  } else {
    float s = v[0];
    for (int c = 1; c < a.Cr; ++c) s = s + v[c];
    a.out[idx] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------
// launchers: refuse (negative code, nothing launched) what the kernels cannot run
// ---------------------------------------------------------------------------------------------------------
static bool sg_image_ok(int Hp, int Wp, int Hr, int Wr, int Cr) {      // cnn_saliency.hip sal_image_ok
  return Hp >= 1 && Wp >= 1 && Hp <= 0x7fff && Wp <= 0x7fff && Hr >= 1 && Wr >= 1 && Hr <= Hp && Wr <= Wp &&
         Cr >= 1 && Cr <= SG_MAXCR;
}

// grid (rows, blocks of real pixels); false when a dimension does not fit
static bool sg_grid(long rows, int Hr, int Wr, dim3& grid) {
  const long gy = ((long)Hr * Wr + SG_BLOCK - 1) / SG_BLOCK;
  if (rows < 1 || rows > 0x7fffffffL || gy > 65535) return false;
  grid = dim3((unsigned)rows, (unsigned)gy);
  return true;
}

extern "C" {

int gt_sg_points(const SgPointsArgs* a, hipStream_t stream) {
  if (!a || !a->raw || !a->out || !a->sigma) return -3;
  if (a->prec != 0 && a->prec != 1) return -1;
  if (!sg_image_ok(a->Hp, a->Wp, a->Hr, a->Wr, a->Cr)) return -1;
  if (a->S < 1 || a->S > SG_MAXS || a->R < 1 || (long)a->S * a->R > a->rows || a->n0 < 0) return -4;
  dim3 grid;
  if (!sg_grid((long)a->S * a->R, a->Hr, a->Wr, grid)) return -4;
  if (a->prec) hipLaunchKernelGGL(sg_points_kernel<1>, grid, dim3(SG_BLOCK), 0, stream, *a);
  else hipLaunchKernelGGL(sg_points_kernel<0>, grid, dim3(SG_BLOCK), 0, stream, *a);
  return (int)hipGetLastError();
}

int gt_sg_reduce(const SgReduceArgs* a, hipStream_t stream) {
  if (!a || !a->dx || !a->x || !a->weight || !a->out) return -3;
  if (a->prec != 0 && a->prec != 1) return -1;
  if (!sg_image_ok(a->Hp, a->Wp, a->Hr, a->Wr, a->Cr)) return -1;
  if (a->G < 1 || a->S < 1 || a->S > SG_MAXS || a->R < 1 || (long)a->S * a->R > a->B) return -4;
  if (a->stat < 0 || a->stat > 2 || a->method < 0 || a->method > 1 || a->reduce < 0 || a->reduce > 2) return -4;
  dim3 grid;
  if (!sg_grid(a->R, a->Hr, a->Wr, grid)) return -4;
  if (a->prec) hipLaunchKernelGGL(sg_reduce_kernel<1>, grid, dim3(SG_BLOCK), 0, stream, *a);
  else hipLaunchKernelGGL(sg_reduce_kernel<0>, grid, dim3(SG_BLOCK), 0, stream, *a);
  return (int)hipGetLastError();
}

size_t gt_sizeof_sg_points_args() { return sizeof(SgPointsArgs); }
size_t gt_sizeof_sg_reduce_args() { return sizeof(SgReduceArgs); }
int gt_sg_max_samples() { return SG_MAXS; }
unsigned gt_sg_key() { return SG_KEY; }

}  // extern "C"
