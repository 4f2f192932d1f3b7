// Where the feature rows of a fitted Genetic-CNN live on the device, shared by the kernels that read them
// (cnn_neighbors.hip, cnn_gaussian.hip).
#pragma once
#include "common.h"

// where the features of a row live: gt_dense_fwd's output [G][B][Up], or (flat) a host array uploaded as
// [rows][ld] fp32 with member g's real units at columns g * Ur ..
struct NnSrc {
  const void* h;
  int G, B, Up, Ur, flat, ld;
};

// the 8 features of chunk c (of Dp / 8) of one row as fp32; padding units are zeros whatever the memory holds
template <int SP>
__device__ __forceinline__ void nn_chunk(const NnSrc& s, int row, int c, float* f) {
  const int cpu = s.Up >> 3;
  const int g = c / cpu, u = (c - g * cpu) * 8;
  if (s.flat) {
    const float* p = static_cast<const float*>(s.h) + (int64_t)row * s.ld + g * s.Ur + u;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = u + e < s.Ur ? p[e] : 0.f;
    return;
  }
  const int64_t at = ((int64_t)g * s.B + row) * s.Up + u;
  if (SP) load8f(static_cast<const float*>(s.h) + at, f);
  else unpack8(*reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(s.h) + at), f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = u + e < s.Ur ? f[e] : 0.f;
}

// what every launcher that reads `rows` rows of a source asks of it (sprec: 1 fp32 values, 0 bf16)
static inline bool nn_src_ok(const NnSrc& s, int rows, int sprec) {
  if (!s.h || s.G < 1 || s.Up < 32 || s.Up % 32 || s.Ur < 1 || s.Ur > s.Up) return false;
  if ((long)s.G * s.Up > (1L << 20) || rows < 1 || rows > s.B) return false;
  if (s.flat != 0 && s.flat != 1) return false;
  if (s.flat && (sprec != 1 || s.ld < s.G * s.Ur)) return false;
  return true;
}
