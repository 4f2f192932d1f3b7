// Monte-Carlo dropout head for fitted Genetic-CNN models on MI355X (gfx950)
// (models/cnn_fitted.py predict_mc, models/cnn_ensemble.py).
//
// Dropout sits only between the two dense layers, so the conv stages and gt_dense_fwd run once per image
// (evaluation mode) and only the second dense layer is repeated: T masked copies of the hidden row h of every
// member, a [C <= 16 classes] x [Up units] x [T <= 64 samples] product per (member, image), on the matrix cores
// in the exact three-plane split of common.h. The masks are drawn here (hash4, keyed by seed, member, sample,
// image index and unit), the samples' probabilities stay in LDS and only the statistics go to memory.
//
//   key_g  = hash4(seed, g, 0x4D434452, 0)
//   keep   = hash4(key_g, t, n0 + row, u) >= thr          thr = uint32(dropout * 2^32), from the host
//   p_{g,t} = softmax((keep ? h_g[u] * keep_scale : 0) W2_g + b2_g)
//   mean_g = p_{g,0} + (sum_t (p_{g,t} - p_{g,0})) * inv_T      (the mean, shifted by the first sample: exact
//                                                                when every sample is the same)
//   var_g  = (sum_t (p_{g,t} - mean_g)^2) * inv_T               (two-pass, around the member's own mean)
//   proba  = sum_g w_g mean_g            std = sqrt(sum_g w_g (var_g + (mean_g - proba)^2))
//   entropy = H(proba)                   expected_entropy = sum_g w_g (H(p_{g,0}) + (sum_t (H(p_{g,t}) - H(p_{g,0}))) * inv_T)
//   mutual_info = max(entropy - expected_entropy, 0), both entropies taken again in fp64 from the fp32 samples and
//                 their fp64 means and the difference rounded once: the difference of the two fp32 outputs would
//                 carry 2^-23 of an entropy near 1, 2e-5 of a mutual information of 5e-3
//   label  = first maximum of proba
// Every sum has one fixed order and a row's result depends on that row, n0 + row and the arguments only:
// equal bits run to run and for any chunking of the images into launches.

#include <cstring>

#include "common.h"

#define MC_MAXC 16
#define MC_MAXT 64
#define MC_MAXG 64
#define MC_MAXU 4096
#define MC_RPW 4              // image rows per workgroup: one W2 staging serves them all
#define MC_CHUNK 512          // units of W2 staged at a time
#define MC_WLD (MC_CHUNK + 8) // W2^T row stride (bf16): the 16 class rows of a b128 read fall on distinct banks
#define MC_KEY 0x4D434452u

struct HeadMcArgs {
  const void* h;            // [G][B][Up] gt_dense_fwd's output in evaluation mode, bf16 or fp32 (prec)
  const float* w2;          // [G][Up][C] fp32 master
  const float* b2;          // [G][C]
  const float* weight;      // [G] fp32, normalised on the host
  float* proba;             // [B][C]
  float* std;               // [B][C]
  float* entropy;           // [B]
  float* expected_entropy;  // [B]
  float* mutual_info;       // [B]
  int* label;               // [B]
  float* samples;           // [B][G][T][C] every p_{g,t}, or null
  int G, B, Up, Ur, C, T, m, prec;
  unsigned thr, seed, n0;
  float keep_scale, inv_T;
};

// -sum_c term[c] over 16 classes in the one order both users share: four runs of four classes, each summed
// left to right, then (q0 + q1) + (q2 + q3) -- what a lane's four classes and the xor steps 16, 32 give.
__device__ __forceinline__ float mc_plogp(float p) { return p > 0.f ? p * logf(p) : 0.f; }

__device__ __forceinline__ float mc_sum4(float t0, float t1, float t2, float t3) {
#pragma clang fp contract(off)
  return ((t0 + t1) + t2) + t3;
}

__global__ void __launch_bounds__(256) head_mc_kernel(HeadMcArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char mc_smem[];
  uint16_t* wl = reinterpret_cast<uint16_t*>(mc_smem);                       // [3][16][MC_WLD] planes of W2^T
  float* hl = reinterpret_cast<float*>(mc_smem + 3 * 16 * MC_WLD * 2);       // [MC_RPW][MC_CHUNK] rows of h
  float* ps = hl + MC_RPW * MC_CHUNK;                                        // [MC_MAXT][16] one row's samples
  float* ent = ps + MC_MAXT * 16;                                            // [MC_MAXT] their entropies
  double* ent64 = reinterpret_cast<double*>(ent + MC_MAXT);                  // [MC_MAXT] the same in fp64
  float* mean_m = reinterpret_cast<float*>(ent64 + MC_MAXT);                 // [MC_RPW][G][16]
  float* var_m = mean_m + MC_RPW * a.G * 16;                                 // [MC_RPW][G][16]
  float* hent_m = var_m + MC_RPW * a.G * 16;                                 // [MC_RPW][G]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4, l16 = lane & 15;
  const int C = a.C, T = a.T, G = a.G, Up = a.Up;
  const int row0 = blockIdx.x * MC_RPW;
  const int nrows = min(MC_RPW, a.m - row0);                 // >= 1: the grid is ceil(m / MC_RPW)
  const int nw = (T + 15) >> 4;                              // waves with samples
  const int t = wave * 16 + l16;                             // this lane's sample
  const float ks = a.keep_scale;
  const uint32_t thr = a.thr;

  // wave 0, lane c: the fp64 mean probability of class c and (every lane) the fp64 expected entropy of each row
  double pq[MC_RPW], eq[MC_RPW];
#pragma unroll
  for (int r = 0; r < MC_RPW; ++r) pq[r] = eq[r] = 0.0;
  for (int g = 0; g < G; ++g) {
    const uint32_t key = hash4(a.seed, (uint32_t)g, MC_KEY, 0u);
    // two accumulators per row: the leading term a0 b0 of the six-term product and the five small ones apart, so
    // the sum of logit size is rounded once per k-step, not six times (over 16 k-steps the six roundings per step
    // cost 2 to 5 times stock fp32's error in the statistics); they join after the last k-step
    f32x4_t acc[MC_RPW], lo[MC_RPW];
#pragma unroll
    for (int r = 0; r < MC_RPW; ++r) acc[r] = lo[r] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int u0 = 0; u0 < Up; u0 += MC_CHUNK) {
      const int cu = min(MC_CHUNK, Up - u0);                 // a multiple of 64
      __syncthreads();                                       // the previous chunk's readers are done
      // W2^T planes: item (class c, 8 units j), c fastest (the 16 classes of a unit are contiguous in W2);
      // classes >= C and units >= Ur become zero whatever the memory holds
      for (int it = tid; it < 16 * (cu >> 3); it += 256) {
        const int c = it & 15, j = it >> 4;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int u = u0 + 8 * j + e;
          const bool ok = c < C && u < a.Ur;
          f[e] = ok ? a.w2[((long)g * Up + u) * C + c] : 0.f;
        }
        uint4 q[3];
        split8(f, q[0], q[1], q[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(&wl[(p * 16 + c) * MC_WLD + 8 * j]) = q[p];
      }
      // the rows' hidden activations of this chunk as fp32; rows past the last and units >= Ur are zero
      for (int r = 0; r < MC_RPW; ++r) {
        const long base = ((long)g * a.B + (row0 + min(r, nrows - 1))) * Up + u0;
        for (int k = tid; k < cu; k += 256) {
          float v = 0.f;
          if (r < nrows && u0 + k < a.Ur)
            v = a.prec ? static_cast<const float*>(a.h)[base + k] : bf2f(static_cast<const uint16_t*>(a.h)[base + k]);
          hl[r * MC_CHUNK + k] = v;
        }
      }
      __syncthreads();
      if (wave < nw) {
#pragma unroll
        for (int r = 0; r < MC_RPW; ++r) {
          if (r >= nrows) continue;                          // block-uniform
          const uint32_t n = a.n0 + (uint32_t)(row0 + r);
          for (int s = 0; s < (cu >> 5); ++s) {
            const int k0 = s * 32 + kq * 8;                  // this lane's 8 units of the k-step
            uint4 af[3], bf[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) af[p] = *reinterpret_cast<const uint4*>(&wl[(p * 16 + l16) * MC_WLD + k0]);
            float f[8];
            load8f(&hl[r * MC_CHUNK + k0], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint32_t rr = hash4(key, (uint32_t)t, n, (uint32_t)(u0 + k0 + e));
              const float kept = f[e] * ks;
              f[e] = rr >= thr ? kept : 0.f;
            }
            split8(f, bf[0], bf[1], bf[2]);
            lo[r] = mfma16(af[2], bf[0], lo[r]);             // D[row = class][col = sample]; mfma_np<3>'s terms,
            lo[r] = mfma16(af[1], bf[1], lo[r]);             // smallest first
            lo[r] = mfma16(af[0], bf[2], lo[r]);
            lo[r] = mfma16(af[1], bf[0], lo[r]);
            lo[r] = mfma16(af[0], bf[1], lo[r]);
            acc[r] = mfma16(af[0], bf[0], acc[r]);
          }
        }
      }
    }
    // softmax of every sample, then the member's statistics, row by row
#pragma unroll
    for (int r = 0; r < MC_RPW; ++r) {
      if (r >= nrows) continue;                              // block-uniform: no barrier is skipped by a part
      acc[r] += lo[r];
      if (wave < nw) {
        float z[4], p[4];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = kq * 4 + i;
          z[i] = c < C ? acc[r][i] + a.b2[(long)g * C + c] : -INFINITY;
          mx = fmaxf(mx, z[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = kq * 4 + i < C ? expf(z[i] - mx) : 0.f;
        float sum = mc_sum4(p[0], p[1], p[2], p[3]);
        sum = sum + __shfl_xor(sum, 16);
        sum = sum + __shfl_xor(sum, 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = p[i] / sum;
        float hs = mc_sum4(mc_plogp(p[0]), mc_plogp(p[1]), mc_plogp(p[2]), mc_plogp(p[3]));
        hs = hs + __shfl_xor(hs, 16);
        hs = hs + __shfl_xor(hs, 32);
        double hd = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (p[i] > 0.f) hd = hd + (double)p[i] * log((double)p[i]);
        hd = hd + __shfl_xor(hd, 16);
        hd = hd + __shfl_xor(hd, 32);
        if (t < T && kq == 0) ent64[t] = -hd;
        if (t < T) {
          *reinterpret_cast<float4*>(&ps[t * 16 + kq * 4]) = make_float4(p[0], p[1], p[2], p[3]);
          if (kq == 0) ent[t] = -hs;
          if (a.samples) {
            float* dst = a.samples + (((long)(row0 + r) * G + g) * T + t) * C;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (kq * 4 + i < C) dst[kq * 4 + i] = p[i];
          }
        }
      }
      __syncthreads();
      if (wave == 0 && lane < 16) {                          // lane c owns class c; fixed t order
        const float p0 = ps[lane], e0 = ent[0];
        float s = 0.f, es = 0.f;
        for (int tt = 1; tt < T; ++tt) {
          s = s + (ps[tt * 16 + lane] - p0);
          es = es + (ent[tt] - e0);
        }
        const float mean = p0 + s * a.inv_T;
        float v = 0.f;
        for (int tt = 0; tt < T; ++tt) {
          const float d = ps[tt * 16 + lane] - mean;
          v = v + d * d;
        }
        mean_m[(r * G + g) * 16 + lane] = mean;
        var_m[(r * G + g) * 16 + lane] = v * a.inv_T;
        if (lane == 0) hent_m[r * G + g] = e0 + es * a.inv_T;
        double sd = 0.0, ed = 0.0;
        for (int tt = 0; tt < T; ++tt) {
          sd = sd + (double)ps[tt * 16 + lane];
          ed = ed + ent64[tt];
        }
        pq[r] = pq[r] + (double)a.weight[g] * (sd / (double)T);
        eq[r] = eq[r] + (double)a.weight[g] * (ed / (double)T);
      }
      __syncthreads();                                       // ps / ent are free for the next row
    }
  }
  if (wave == 0) {                                           // the mutual information from the fp64 sums
#pragma unroll
    for (int r = 0; r < MC_RPW; ++r) {
      if (r >= nrows) continue;
      const double term = (lane < 16 && pq[r] > 0.0) ? pq[r] * log(pq[r]) : 0.0;
      double hq = 0.0;
#pragma unroll
      for (int k = 0; k < MC_MAXC; ++k) hq = hq + __shfl(term, k);
      if (lane == 0) a.mutual_info[row0 + r] = (float)fmax(-hq - eq[r], 0.0);
    }
  }
  // the members combined in member order: wave r serves row r, lane c class c (lanes >= C carry zeros)
  for (int r = wave; r < nrows; r += 4) {
    const int c = lane & 15;
    const float* mm = mean_m + r * G * 16 + c;
    const float* vm = var_m + r * G * 16 + c;
    float pr = a.weight[0] * mm[0];
    for (int g = 1; g < G; ++g) pr = pr + a.weight[g] * mm[g * 16];
    float tv = 0.f, eh = 0.f;
    for (int g = 0; g < G; ++g) {
      const float d = mm[g * 16] - pr;
      tv = tv + a.weight[g] * (vm[g * 16] + d * d);
      eh = eh + a.weight[g] * hent_m[r * G + g];
    }
    const float term = mc_plogp(pr);
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      q[k] = mc_sum4(__shfl(term, 4 * k), __shfl(term, 4 * k + 1), __shfl(term, 4 * k + 2), __shfl(term, 4 * k + 3));
    const float hsum = (q[0] + q[1]) + (q[2] + q[3]);
    float best = __shfl(pr, 0);
    int am = 0;
#pragma unroll
    for (int k = 1; k < MC_MAXC; ++k) {
      const float v = __shfl(pr, k);
      if (k < C && v > best) { best = v; am = k; }
    }
    const long row = row0 + r;
    if (lane < C) {
      a.proba[row * C + lane] = pr;
      a.std[row * C + lane] = sqrtf(tv);
    }
    if (lane == 0) {
      a.entropy[row] = -hsum;
      a.expected_entropy[row] = eh;
      a.label[row] = am;
    }
  }
}

static inline bool mc_finite(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof(u));
  return (u & 0x7f800000u) != 0x7f800000u;
}

extern "C" {

// LDS bytes of a launch: the W2^T planes of one chunk, MC_RPW rows of h, one row's samples and entropies (fp32 and fp64), and
// the members' means, variances and mean entropies of MC_RPW rows.
size_t gt_head_mc_lds(int G) {
  return (size_t)3 * 16 * MC_WLD * 2 + sizeof(float) * ((size_t)MC_RPW * MC_CHUNK + MC_MAXT * 16 + MC_MAXT +
                                                        (size_t)MC_RPW * G * (16 + 16 + 1)) + sizeof(double) * MC_MAXT;
}

// One workgroup of 4 waves per MC_RPW image rows of the launch's first m. Refuses (negative code, nothing
// launched) what the kernel cannot run.
int gt_head_mc(const HeadMcArgs* a, hipStream_t stream) {
  if (!a) return -3;
  if (!a->h || !a->w2 || !a->b2 || !a->weight) return -3;
  if (!a->proba || !a->std || !a->entropy || !a->expected_entropy || !a->mutual_info || !a->label) return -3;
  if (a->C < 1 || a->C > MC_MAXC || a->G < 1 || a->G > MC_MAXG) return -1;
  if (a->Up < 64 || a->Up % 64 || a->Up > MC_MAXU || a->Ur < 1 || a->Ur > a->Up) return -2;
  if (a->T < 1 || a->T > MC_MAXT || a->B < 1 || a->m < 1 || a->m > a->B) return -4;
  if ((a->prec != 0 && a->prec != 1) || !mc_finite(a->keep_scale) || !mc_finite(a->inv_T)) return -4;
  const size_t lds = gt_head_mc_lds(a->G);
  if (lds > 65536 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(head_mc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return -5;
  const unsigned blocks = (unsigned)((a->m + MC_RPW - 1) / MC_RPW);
  hipLaunchKernelGGL(head_mc_kernel, dim3(blocks), dim3(256), lds, stream, *a);
  return (int)hipGetLastError();
}

size_t gt_sizeof_head_mc_args() { return sizeof(HeadMcArgs); }

}  // extern "C"
