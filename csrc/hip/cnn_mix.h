// The mixup / cutmix draw of one (group, global step), shared by gt_augment_mix (cnn_mix.hip) and
// gt_head_mix (cnn_dense.hip). The definition is written down once, in gentun_amd/models/cnn_engine.py
// ("The mixed step"); gentun_amd/utils/rng.py mix_draws is the numpy twin and tests/mix_ref.py the oracle.
//
// Integer work only. Every input is uniform over a workgroup (the key, the step and the batch's real rows
// depend on the group alone), so the compiler keeps the whole draw on the scalar unit: once per wave, no
// LDS and no per-thread hashing.
#pragma once

#include "common.h"

#define MIX_CTR 0xA0610000u     // hash4 counters of the draw (the augmentation uses 0xA0600000 + k)
#define MIX_MAX_ALPHA 8
#define MIX_MAXU (2 * MIX_MAX_ALPHA - 1)
#define MIX_ONE24 0x1000000u

struct MixDraw {
  bool applied;         // this step is mixed (never with fewer than two real rows)
  uint32_t o;           // partner offset: p(b) = (b + o) % nv for b < nv
  uint32_t m;           // 24-bit Beta(alpha, alpha) draw
};

struct MixBox { int y0, y1, x0, x1; };

// floor(sqrt(v)), digit by digit
__device__ __forceinline__ uint32_t mix_isqrt(uint32_t v) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t bit = 1u << 30; bit; bit >>= 2) {
    if (v >= r + bit) { v -= r + bit; r = (r >> 1) + bit; }
    else r >>= 1;
  }
  return r;
}

__device__ __forceinline__ MixDraw mix_draw(uint32_t key, uint32_t t, int nv, int alpha, uint32_t p24) {
  MixDraw d;
  d.o = 0u;
  d.m = 0u;
  d.applied = nv >= 2 && (hash4(key, t, 0u, MIX_CTR) >> 8) < p24;
  if (!d.applied) return d;
  d.o = 1u + hash4(key, t, 0u, MIX_CTR + 1u) % (uint32_t)(nv - 1);
  // the alpha-th smallest of 2 alpha - 1 uniforms, by counting the smaller elements of each (ties by index).
  // Only the 2 alpha - 1 draws in use are hashed and ranked (uniform branches: alpha = 1 is one hash); the
  // unused tail holds values above every draw and never counts
  const int n = 2 * alpha - 1;
  uint32_t u[MIX_MAXU];
#pragma unroll
  for (int j = 0; j < MIX_MAXU; ++j) u[j] = 0xFFFFFFFFu;
#pragma unroll
  for (int j = 0; j < MIX_MAXU; ++j) {
    if (j >= n) break;
    u[j] = hash4(key, t, 0u, MIX_CTR + 16u + j) >> 8;
  }
#pragma unroll
  for (int i = 0; i < MIX_MAXU; ++i) {
    if (i >= n) break;
    int below = 0;
#pragma unroll
    for (int j = 0; j < MIX_MAXU; ++j) below += (u[j] < u[i] || (u[j] == u[i] && j < i)) ? 1 : 0;
    if (below == alpha - 1) d.m = u[i];
  }
  return d;
}

// the cutmix box of an applied step, clipped to the real image (Hr, Wr < 2^15: the squares fit 32 bits)
__device__ __forceinline__ MixBox mix_box(uint32_t key, uint32_t t, uint32_t m, int Hr, int Wr) {
  const int cy = (int)(hash4(key, t, 0u, MIX_CTR + 2u) % (uint32_t)Hr);
  const int cx = (int)(hash4(key, t, 0u, MIX_CTR + 3u) % (uint32_t)Wr);
  const uint64_t keep = MIX_ONE24 - m;
  const int bh = (int)mix_isqrt((uint32_t)(((uint64_t)Hr * Hr * keep) >> 24));
  const int bw = (int)mix_isqrt((uint32_t)(((uint64_t)Wr * Wr * keep) >> 24));
  const int ty = cy - bh / 2, tx = cx - bw / 2;
  MixBox b;
  b.y0 = max(ty, 0);
  b.y1 = min(ty + bh, Hr);
  b.x0 = max(tx, 0);
  b.x1 = min(tx + bw, Wr);
  return b;
}

// the weights of a row and of its partner in the mixed target (kind 0: also in the mixed image)
__device__ __forceinline__ void mix_weights(int kind, uint32_t m, const MixBox& bx, int Hr, int Wr, float inv_hw,
                                            float& lam, float& lam1) {
  if (kind == 0) {
    lam = (float)m * 0x1p-24f;                       // exact: m < 2^24
    lam1 = (float)(MIX_ONE24 - m) * 0x1p-24f;
  } else {
    const int area = (bx.y1 - bx.y0) * (bx.x1 - bx.x0);
    lam = (float)(Hr * Wr - area) * inv_hw;
    lam1 = (float)area * inv_hw;
  }
}

// fp32(lam a) + fp32(lam1 b): two products and a sum, each rounded (never contracted into an fma)
__device__ __forceinline__ float mix_blend(float lam, float a, float lam1, float b) {
#pragma clang fp contract(off)
  const float x = lam * a;
  const float y = lam1 * b;
  return x + y;
}
