// Input-gradient saliency of a fitted Genetic-CNN (models/cnn_fitted.py SaliencyState): the kernels the
// evaluation-mode backward chain adds to the training step's own data-gradient launches.
//
//   gt_conv_in_dgrad  data gradient of the network's input conv (the training step has none: the dataset
//                     has no gradient), as a GEMM over the output channels plus a col2im in LDS
//   gt_bn_bwd_eval    BatchNorm backward under running statistics: a per-channel scale, in place
//   gt_ig_points      the interpolation points of integrated gradients, raw chunk -> staging rows
//   gt_ig_reduce      the finishing kernel of every method: ordered sum over the points, the 1/m and
//                     (x - x0) factors, the members' weighted mean and the channel reduction
//
// gt_head_saliency, which seeds the chain, sits in cnn_dense.hip next to the head helpers it shares.
// Element-wise arithmetic here is rounded operation by operation (fp contraction off), so fp32 numpy
// reproduces it bit for bit.
#include "common.h"

#include <algorithm>

// ---------------------------------------------------------------------------------------------------------
// gt_conv_in_dgrad
// ---------------------------------------------------------------------------------------------------------
// dx[i][j][c] = sum_{kh, kw, co} dz[i + ph - kh][j + pw - kw][co] * w[co][kh][kw][c]   (ph = KH / 2, pw = KW / 2)
// over the dz pixels inside the real image. With 1 or 3 real input channels the implicit-GEMM data gradient
// would run 16-wide MFMA tiles that are more than 80 % padding. Instead every dz pixel q is multiplied once
// with the whole kernel,
//     Y[q][(kh, kw, c)] = sum_co dz[q][co] * w[co][kh][kw][c]          M = pixels, K = Coutp, N = KH * KW * Cr,
// N rounded up to 16 (5x5x3: 75 -> 80, 5x5x1: 25 -> 32, 3x3x3: 27 -> 32, 3x3x1: 9 -> 16), and the output pixel
// (i, j) gathers its KH * KW taps from Y.
//
// Work split: one workgroup (4 waves) per band of TR output rows of one image, TR * Wp = 256 output pixels (one
// per thread; narrower images leave threads idle). The band needs the dz rows [r0 - ph, r0 + TR - 1 + ph]; they
// are walked in steps of 64 pixels (64 / Wp whole rows). Per step wave w owns the 16-pixel M tile w: its A
// fragment comes straight from global memory (a lane's 8 consecutive channels of its pixel are one 16- or
// 32-byte load; padded pixels and the chunks past Coutp select a zero source and are never read; channels
// >= Cout are zeroed after the load), the B fragments -- the weights of every N tile and k-step, three exact
// bf16 planes of the fp32 master -- are gathered once per workgroup and stay in registers. fp32 activations go
// through the three-way split too (six MFMA terms per product, common.h); bf16 activations are exact in one
// plane (three terms). Y [64][N] goes to LDS in fp32; after a barrier every thread adds the taps that these dz
// rows hold for its output pixel: dz rows ascending (kh descending), kw ascending, one fp32 add per tap and
// channel. No atomics: the order is a function of the output pixel alone, so the result does not depend on
// the band, the row position, the batch or the other groups. The next step's A operands are loaded before
// the gather, so the global loads overlap it.
struct ConvInDgradArgs {
  const void* dz;        // [G][B][Hp][Wp][Coutp] bf16 or fp32 (prec): gradient of the conv's output
  const float* w;        // [G][Coutp][KH][KW][C8] fp32 master weights
  float* dx;             // [G][B][Hp][Wp][C8] fp32
  int G, B, m;           // rows b < m are computed, the others left alone
  int Hp, Wp, Hr, Wr;    // stored and real image
  int Coutp, Cout;       // stored and real output channels of the conv
  int C8, Cr;            // stored (8) and real (1..3) input channels
  int KH, KW;
  int prec;
};

#define CID_C8 8
#define CID_MAXCR 3

template <int PREC, int NT, int KS>
__global__ void __launch_bounds__(256) conv_in_dgrad_kernel(ConvInDgradArgs a) {
#pragma clang fp contract(off)
  typedef typename ActT<PREC>::T AT;
  constexpr int NPA = PREC ? GT_NPL_F32 : 1;       // planes of the dz operand
  constexpr int LDY = NT * 16 + 1;                 // odd row stride: the gather reads a column without conflicts
  __shared__ float Y[64 * LDY];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4, l16 = lane & 15;
  const int g = blockIdx.z, b = blockIdx.y;
  const int Wp = a.Wp, KH = a.KH, KW = a.KW, ph = KH >> 1, pw = KW >> 1, Cr = a.Cr;
  const int TR = min(a.Hp, 256 / Wp), r0 = blockIdx.x * TR;
  const int nreal = KH * KW * Cr;
  // ---- B fragments: w[co = 32 ks + 8 kq + e][n = 16 nt + l16], n = (kh * KW + kw) * Cr + c
  uint4 wf[NT][KS][GT_NPL_F32];
  {
    const float* wg = a.w + (long)g * a.Coutp * KH * KW * CID_C8;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = nt * 16 + l16;
      const bool nok = n < nreal;
      const int tap = nok ? n / Cr : 0, c = nok ? n - tap * Cr : 0;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int co = ks * 32 + kq * 8 + e;
          const bool ok = nok && co < a.Cout;
          f[e] = ok ? wg[((long)co * KH * KW + tap) * CID_C8 + c] : 0.f;
        }
        split8(f, wf[nt][ks][0], wf[nt][ks][1], wf[nt][ks][2]);
      }
    }
  }
  // ---- this thread's output pixel
  const int oi = r0 + tid / Wp, oj = tid % Wp;
  const bool owner = tid < TR * Wp;
  float acc[CID_MAXCR] = {0.f, 0.f, 0.f};
  // ---- dz rows of the band inside the real image
  const int d_first = max(0, r0 - ph), d_last = min(a.Hr - 1, r0 + TR - 1 + ph);
  const int rows_it = 64 / Wp;
  const AT* dzi = static_cast<const AT*>(a.dz) + ((long)g * a.B + b) * a.Hp * Wp * a.Coutp;
  float raw[KS][8];
  auto load = [&](int da) {
    const int q = wave * 16 + l16, d = da + q / Wp, x = q % Wp;
    const bool pok = d <= d_last && x < a.Wr;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int co0 = ks * 32 + kq * 8;
      const bool ok = pok && co0 < a.Coutp;
      const AT* p = dzi + ((long)d * Wp + x) * a.Coutp + co0;
      if constexpr (PREC) {
        load8f_or0(reinterpret_cast<const float*>(p), ok, raw[ks]);
      } else {
        const uint4 v = *(ok ? reinterpret_cast<const uint4*>(p) : reinterpret_cast<const uint4*>(gt_zero8));
        unpack8(v, raw[ks]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) raw[ks][e] = (ok && co0 + e < a.Cout) ? raw[ks][e] : 0.f;
    }
  };
  if (d_first <= d_last) load(d_first);
  for (int da = d_first; da <= d_last; da += rows_it) {
    // ---- Y tile of the 64 pixels from row da
    uint4 af[KS][NPA];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr (PREC) split8(raw[ks], af[ks][0], af[ks][1], af[ks][2]);
      else af[ks][0] = pack8(raw[ks]);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      f32x4_t c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if constexpr (PREC) {
          c = mfma_np<GT_NPL_F32>(af[ks], wf[nt][ks], c);
        } else {
          c = mfma16(af[ks][0], wf[nt][ks][2], c);
          c = mfma16(af[ks][0], wf[nt][ks][1], c);
          c = mfma16(af[ks][0], wf[nt][ks][0], c);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) Y[(wave * 16 + 4 * kq + r) * LDY + nt * 16 + l16] = c[r];
    }
    if (da + rows_it <= d_last) load(da + rows_it);
    __syncthreads();
    // ---- col2im: the taps these rows hold for the thread's pixel
    if (owner && oi < a.Hr && oj < a.Wr) {
      for (int dr = 0; dr < rows_it; ++dr) {
        const int d = da + dr, kh = oi + ph - d;
        if (d > d_last || kh < 0 || kh >= KH) continue;
        for (int kw = 0; kw < KW; ++kw) {
          const int x = oj + pw - kw;
          if (x < 0 || x >= a.Wr) continue;
          const float* y = Y + (dr * Wp + x) * LDY + (kh * KW + kw) * Cr;
#pragma unroll
          for (int c = 0; c < CID_MAXCR; ++c)
            if (c < Cr) acc[c] = acc[c] + y[c];
        }
      }
    }
    __syncthreads();
  }
  if (owner) {
    const bool real = oi < a.Hr && oj < a.Wr;
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < CID_MAXCR; ++c)
      if (real && c < Cr) o[c] = acc[c];
    store8f(a.dx + ((((long)g * a.B + b) * a.Hp + oi) * Wp + oj) * CID_C8, o);
  }
}

// ---------------------------------------------------------------------------------------------------------
// gt_bn_bwd_eval
// ---------------------------------------------------------------------------------------------------------
// Evaluation-mode BatchNorm is y = z * sc + sh with constants of the fitted model, so its backward is
// dz = dy * (gamma * (1 / sqrt(running_var + eps))), every operation rounded once (the square root and the
// division correctly rounded), in place on the ReLU-masked gradient. Exact zeros at padded pixels and channels.
// One workgroup per chunk_px pixels of a group (BnArgs' chunk geometry); no statistics pass.
struct BnBwdEvalArgs {
  void* dy;              // [G][B][H][W][Cp] bf16 or fp32 (prec): gradient in, dz out
  const float* gamma;    // [G][Cp]
  const float* run;      // [2][G][Cp] running mean, running variance
  int G, B, H, W, Hr, Wr, Cp, Cr;
  int nchunk, chunk_px;
  float eps;
  int prec;
};

template <int PREC>
__global__ void __launch_bounds__(256) bn_bwd_eval_kernel(BnBwdEvalArgs a) {
#pragma clang fp contract(off)
  typedef typename ActT<PREC>::T AT;
  __shared__ float sc[256];
  const int g = blockIdx.y, Cp = a.Cp, nc8 = Cp >> 3, t = threadIdx.x;
  if (t < Cp) {
    const float var = a.run[(long)a.G * Cp + (long)g * Cp + t];
    const float rstd = 1.f / sqrtf(var + a.eps);
    sc[t] = t < a.Cr ? a.gamma[(long)g * Cp + t] * rstd : 0.f;
  }
  __syncthreads();
  const long HW = (long)a.H * a.W, npx = (long)a.B * HW;
  const long p0 = (long)blockIdx.x * a.chunk_px;
  const long p1 = p0 + a.chunk_px < npx ? p0 + a.chunk_px : npx;
  AT* dy = static_cast<AT*>(a.dy) + (long)g * npx * Cp;
  for (long i = t; i < (p1 - p0) * nc8; i += 256) {
    const long p = p0 + i / nc8;
    const int c8 = (int)(i % nc8);
    const int px = (int)(p % HW), row = px / a.W, col = px - row * a.W;
    const bool real = row < a.Hr && col < a.Wr;
    float v[8];
    ld_chunk(dy + p * Cp + c8 * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (real && c8 * 8 + e < a.Cr) ? v[e] * sc[c8 * 8 + e] : 0.f;
    st_chunk(dy + p * Cp + c8 * 8, v);
  }
}

// ---------------------------------------------------------------------------------------------------------
// gt_ig_points / gt_ig_reduce
// ---------------------------------------------------------------------------------------------------------
#define IG_MAXM 64

// Staging row k * R + r = x0 + alpha[k] * (x[r] - x0) at the real pixels and channels (the subtraction, the
// product and the sum rounded separately in fp32, then once to the staging type), for k < m and r < R. Rows
// >= m * R, padded pixels and padded channels are not touched. gt_tta_views' shape: one thread per 8-channel
// pixel of an output row.
struct IgPointsArgs {
  const void* raw;       // [R][Hp][Wp][C8] the images, staging layout and type
  void* out;             // [rows][Hp][Wp][C8] the staging tensor
  const float* x0;       // [C8] the baseline per channel (already rounded to the staging type)
  int R, m, rows;
  int Hp, Wp, Hr, Wr, Cr;
  int prec;
  float alpha[IG_MAXM];  // fp32((k + 0.5) / m) from the host
};

template <int PREC>
__global__ void __launch_bounds__(256) ig_points_kernel(IgPointsArgs a) {
#pragma clang fp contract(off)
  typedef typename ActT<PREC>::T AT;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)a.Hr * a.Wr, total = (long)a.m * a.R * per;
  if (idx >= total) return;
  const int row = (int)(idx / per), px = (int)(idx % per);
  const int k = row / a.R, r = row - k * a.R;
  const int i = px / a.Wr, j = px - i * a.Wr;
  const long pix = ((long)i * a.Wp + j) * CID_C8, img = (long)a.Hp * a.Wp * CID_C8;
  float v[8], o[8];
  ld_chunk(static_cast<const AT*>(a.raw) + r * img + pix, v);
  AT* dst = static_cast<AT*>(a.out) + row * img + pix;
  ld_chunk(dst, o);
  const float al = a.alpha[k];
#pragma unroll
  for (int c = 0; c < CID_MAXCR; ++c) {
    if (c < a.Cr) {
      const float x0 = a.x0[c];
      const float d = v[c] - x0;
      const float s = al * d;
      o[c] = x0 + s;
    }
  }
  st_chunk(dst, o);
}

// Per raw row r, real pixel and channel c < Cr, for every member g in order:
//   s   = dx[g][r], then s + dx[g][k * R + r] for k = 1 .. m - 1           (ordered fp32 sum over the points)
//   a_g = s                     method 0 (gradient; m = 1)
//         x * s                 method 1 (gradient x input; m = 1)
//         (x - x0) * (s * inv_m)  method 2 (integrated gradients)
//   v   = w[0] * a_0, then v + w[g] * a_g                                  (ensemble_mean's rounding)
// and the channel reduction: 0 signed [R][Hr][Wr][Cr]; 1 max_c |v| [R][Hr][Wr]; 2 v_0 + v_1 + ... in channel
// order. One thread per (row, real pixel).
struct IgReduceArgs {
  const float* dx;       // [G][B][Hp][Wp][C8] fp32 from gt_conv_in_dgrad
  const void* x;         // [>= R][Hp][Wp][C8] the images, staging layout and type
  const float* x0;       // [C8]
  const float* weight;   // [G]
  float* out;
  int G, B, R, m;
  int Hp, Wp, Hr, Wr, Cr;
  int method, reduce, prec;
  float inv_m;           // fp32(1) / fp32(m) from the host
};

template <int PREC>
__global__ void __launch_bounds__(256) ig_reduce_kernel(IgReduceArgs a) {
#pragma clang fp contract(off)
  typedef typename ActT<PREC>::T AT;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)a.Hr * a.Wr;
  if (idx >= (long)a.R * per) return;
  const int r = (int)(idx / per), px = (int)(idx % per);
  const int i = px / a.Wr, j = px - i * a.Wr;
  const long pix = ((long)i * a.Wp + j) * CID_C8, img = (long)a.Hp * a.Wp * CID_C8;
  float xv[8];
  ld_chunk(static_cast<const AT*>(a.x) + r * img + pix, xv);
  float v[CID_MAXCR] = {0.f, 0.f, 0.f};
  for (int g = 0; g < a.G; ++g) {
    const float* d = a.dx + ((long)g * a.B + r) * img + pix;
    const float wg = a.weight[g];
#pragma unroll
    for (int c = 0; c < CID_MAXCR; ++c) {
      if (c >= a.Cr) continue;
      float s = d[c];
      for (int k = 1; k < a.m; ++k) s = s + d[(long)k * a.R * img + c];
      float at = s;
      if (a.method == 1) {
        at = xv[c] * s;
      } else if (a.method == 2) {
        const float mean = s * a.inv_m;
        const float dxx = xv[c] - a.x0[c];
        at = dxx * mean;
      }
      const float term = wg * at;
      v[c] = g == 0 ? term : v[c] + term;
    }
  }
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
static bool sal_image_ok(int Hp, int Wp, int Hr, int Wr, int Cr) {
  return Hp >= 1 && Wp >= 1 && Hp <= 0x7fff && Wp <= 0x7fff && Hr >= 1 && Wr >= 1 && Hr <= Hp && Wr <= Wp &&
         Cr >= 1 && Cr <= CID_MAXCR;
}

template <int PREC, int KS>
static void conv_in_dgrad_launch(const ConvInDgradArgs& a, int nt, dim3 grid, hipStream_t stream) {
  if (nt == 1) hipLaunchKernelGGL((conv_in_dgrad_kernel<PREC, 1, KS>), grid, dim3(256), 0, stream, a);
  else if (nt == 2) hipLaunchKernelGGL((conv_in_dgrad_kernel<PREC, 2, KS>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((conv_in_dgrad_kernel<PREC, 5, KS>), grid, dim3(256), 0, stream, a);
}

extern "C" {

int gt_conv_in_dgrad(const ConvInDgradArgs* a, hipStream_t stream) {
  if (!a || !a->dz || !a->w || !a->dx) return -3;
  if (a->prec != 0 && a->prec != 1) return -1;
  if (a->C8 != CID_C8 || !sal_image_ok(a->Hp, a->Wp, a->Hr, a->Wr, a->Cr)) return -1;
  if (a->Wp != 8 && a->Wp != 16 && a->Wp != 32) return -2;             // 64-pixel steps hold whole rows
  const int TR = std::min(a->Hp, 256 / a->Wp);
  if (a->Hp % TR) return -2;
  if (!((a->KH == 5 && a->KW == 5) || (a->KH == 3 && a->KW == 3))) return -2;
  if (a->Coutp < 8 || a->Coutp % 8 || a->Coutp > 64 || a->Cout < 1 || a->Cout > a->Coutp) return -2;
  if (a->G < 1 || a->G > 65535 || a->B < 1 || a->B > 65535 || a->m < 1 || a->m > a->B) return -4;
  const int nt = (a->KH * a->KW * a->Cr + 15) / 16;                     // 1, 2 or 5
  if (nt != 1 && nt != 2 && nt != 5) return -2;
  const int ks = (a->Coutp + 31) / 32;
  dim3 grid((unsigned)(a->Hp / TR), (unsigned)a->m, (unsigned)a->G);
  if (a->prec) {
    if (ks == 1) conv_in_dgrad_launch<1, 1>(*a, nt, grid, stream);
    else conv_in_dgrad_launch<1, 2>(*a, nt, grid, stream);
  } else {
    if (ks == 1) conv_in_dgrad_launch<0, 1>(*a, nt, grid, stream);
    else conv_in_dgrad_launch<0, 2>(*a, nt, grid, stream);
  }
  return (int)hipGetLastError();
}

int gt_bn_bwd_eval(const BnBwdEvalArgs* a, hipStream_t stream) {
  if (!a || !a->dy || !a->gamma || !a->run) return -3;
  if (a->prec != 0 && a->prec != 1) return -1;
  if (a->Cp < 8 || a->Cp % 8 || a->Cp > 256 || a->Cr < 1 || a->Cr > a->Cp) return -1;
  if (a->H < 1 || a->W < 1 || a->Hr < 1 || a->Wr < 1 || a->Hr > a->H || a->Wr > a->W) return -1;
  if (a->G < 1 || a->G > 65535 || a->B < 1 || a->chunk_px < 1) return -4;
  if ((long)a->nchunk * a->chunk_px < (long)a->B * a->H * a->W || a->nchunk < 1) return -4;
  dim3 grid((unsigned)a->nchunk, (unsigned)a->G);
  if (a->prec) hipLaunchKernelGGL(bn_bwd_eval_kernel<1>, grid, dim3(256), 0, stream, *a);
  else hipLaunchKernelGGL(bn_bwd_eval_kernel<0>, grid, dim3(256), 0, stream, *a);
  return (int)hipGetLastError();
}

int gt_ig_points(const IgPointsArgs* a, hipStream_t stream) {
  if (!a || !a->raw || !a->out || !a->x0) return -3;
  if (a->prec != 0 && a->prec != 1) return -1;
  if (!sal_image_ok(a->Hp, a->Wp, a->Hr, a->Wr, a->Cr)) return -1;
  if (a->m < 1 || a->m > IG_MAXM || a->R < 1 || (long)a->m * a->R > a->rows) return -4;
  const long total = (long)a->m * a->R * a->Hr * a->Wr;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (a->prec) hipLaunchKernelGGL(ig_points_kernel<1>, grid, dim3(256), 0, stream, *a);
  else hipLaunchKernelGGL(ig_points_kernel<0>, grid, dim3(256), 0, stream, *a);
  return (int)hipGetLastError();
}

int gt_ig_reduce(const IgReduceArgs* a, hipStream_t stream) {
  if (!a || !a->dx || !a->x || !a->x0 || !a->weight || !a->out) return -3;
  if (a->prec != 0 && a->prec != 1) return -1;
  if (!sal_image_ok(a->Hp, a->Wp, a->Hr, a->Wr, a->Cr)) return -1;
  if (a->G < 1 || a->m < 1 || a->m > IG_MAXM || a->R < 1 || (long)a->m * a->R > a->B) return -4;
  if (a->method < 0 || a->method > 2 || a->reduce < 0 || a->reduce > 2) return -4;
  if (a->method != 2 && a->m != 1) return -4;
  const long total = (long)a->R * a->Hr * a->Wr;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (a->prec) hipLaunchKernelGGL(ig_reduce_kernel<1>, grid, dim3(256), 0, stream, *a);
  else hipLaunchKernelGGL(ig_reduce_kernel<0>, grid, dim3(256), 0, stream, *a);
  return (int)hipGetLastError();
}

size_t gt_sizeof_conv_in_dgrad_args() { return sizeof(ConvInDgradArgs); }
size_t gt_sizeof_bn_bwd_eval_args() { return sizeof(BnBwdEvalArgs); }
size_t gt_sizeof_ig_points_args() { return sizeof(IgPointsArgs); }
size_t gt_sizeof_ig_reduce_args() { return sizeof(IgReduceArgs); }
int gt_ig_max_steps() { return IG_MAXM; }

}  // extern "C"
