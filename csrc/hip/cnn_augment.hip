// Training-time augmentation of the Genetic-CNN input batch: a random
// translation with zero fill (pad and crop) and a random horizontal flip, per
// step and per batch row, drawn on the device.
//
// The first convolution of the HIP executor gathers its batch straight from
// the device-resident dataset (ConvArgs::gather). With augmentation on, this
// kernel runs right after gt_step_begin: it reads image gather[cur_step][g][b]
// and writes row (g, b) of an augmented batch [Q*B][Hp][Wp][Cp] in the same
// layout and element type (nhwc8 bf16 / nhwc8f fp32); the first conv and its
// weight gradient then read that batch through a constant table.
//
// Definition (gentun_amd/utils/rng.py aug_draws is the numpy twin, tests/augment_ref.py the oracle):
//   key  = seeds[g] ^ (fold_ids[g] * 0x632be5ab)             the dropout key of dense_fwd_epilogue
//   r_k  = hash4(key, global_step, row + row_off, 0xA0600000 + k), k = 0, 1, 2
//   dy   = r_0 % (2 shift + 1) - shift,  dx = r_1 % (2 shift + 1) - shift,  flip = flip_enabled & (r_2 >> 31)
//   out[i, j, c] = src[i - dy, f(j - dx), c] inside the real extent Hr x Wr, else 0;  f(u) = flip ? Wr-1-u : u
// Everything outside the real extent of a zero-padded image (28 x 28 in 32 x 32) is written as zeros;
// channel padding is copied from the dataset, where it is zero.
//
// Pure data movement: one 8-channel chunk (16 B bf16, 32 B fp32) per thread, consecutive threads on
// consecutive chunks of an output row, so stores coalesce and a flipped row is read contiguously in
// reverse. One workgroup column (blockIdx.x) is one batch row, so the key, the three hashes and the
// shifts are wave-uniform: the compiler keeps them on the scalar unit, computed once per wave -- no LDS
// broadcast and no per-thread hashing.

#include <hip/hip_runtime.h>

#include "common.h"

#define AUG_BLOCK 256
#define AUG_CTR 0xA0600000u     // hash4 counters no dense unit index reaches

struct AugArgs {
  const void* src;           // dataset [N][Hp][Wp][Cp], bf16 (prec 0) or fp32 (prec 1)
  void* out;                 // augmented batch [Q*B][Hp][Wp][Cp], same type
  const int64_t* gather;     // image table [steps][Q][B]
  const StepState* st;       // cur_step (table row) and global_step (draw key)
  const int* fold_ids;       // [Q] or null (then: the group index)
  const unsigned* seeds;     // [Q] per-group keys or null -> seed
  unsigned seed;
  int row_off;               // data parallelism: this rank's first row of the full batch
  int Q, B, Hp, Wp, Hr, Wr, Cp;
  int shift, flip;
  int prec;
};

template <int PREC>
__global__ __launch_bounds__(AUG_BLOCK) void augment_kernel(const AugArgs a) {
  typedef typename ActT<PREC>::T AT;
  const int qb = blockIdx.x;                       // output row g * B + b
  const int g = qb / a.B, b = qb - g * a.B;
  const uint32_t fid = a.fold_ids ? (uint32_t)a.fold_ids[g] : (uint32_t)g;
  const uint32_t key = (a.seeds ? a.seeds[g] : a.seed) ^ (fid * 0x632be5abU);
  const uint32_t t = (uint32_t)a.st->global_step, row = (uint32_t)(b + a.row_off);
  const uint32_t span = 2u * (uint32_t)a.shift + 1u;
  const int dy = (int)(hash4(key, t, row, AUG_CTR + 0u) % span) - a.shift;
  const int dx = (int)(hash4(key, t, row, AUG_CTR + 1u) % span) - a.shift;
  const bool flip = a.flip && (hash4(key, t, row, AUG_CTR + 2u) >> 31);
  const int64_t img = a.gather[((int64_t)a.st->cur_step * a.Q + g) * a.B + b];

  const uint32_t CB = (uint32_t)a.Cp >> 3;
  const uint32_t chunks = (uint32_t)a.Hp * a.Wp * CB;
  const uint32_t c = blockIdx.y * AUG_BLOCK + threadIdx.x;
  if (c >= chunks) return;
  const FastDiv dcb(CB), dw((uint32_t)a.Wp);
  uint32_t px, cb, ui, uj;
  dcb.divmod(c, px, cb);
  dw.divmod(px, ui, uj);
  const int i = (int)ui, j = (int)uj;
  const int si = i - dy, u = j - dx;
  const bool ok = i < a.Hr && j < a.Wr && si >= 0 && si < a.Hr && u >= 0 && u < a.Wr;
  const int sj = flip ? a.Wr - 1 - u : u;
  AT* dst = static_cast<AT*>(a.out) + ((int64_t)qb * chunks + c) * 8;
  if (PREC) {
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (ok) {
      const float4* p = reinterpret_cast<const float4*>(
          static_cast<const AT*>(a.src) + (((img * a.Hp + si) * a.Wp + sj) * (int64_t)CB + cb) * 8);
      v0 = p[0];
      v1 = p[1];
    }
    reinterpret_cast<float4*>(dst)[0] = v0;
    reinterpret_cast<float4*>(dst)[1] = v1;
  } else {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (ok)
      v = *reinterpret_cast<const uint4*>(
          static_cast<const AT*>(a.src) + (((img * a.Hp + si) * a.Wp + sj) * (int64_t)CB + cb) * 8);
    *reinterpret_cast<uint4*>(dst) = v;
  }
}

extern "C" {

size_t gt_sizeof_aug_args() { return sizeof(AugArgs); }

// Returns non-zero (nothing launched) on arguments the kernel cannot run.
int gt_augment(const void* ap, hipStream_t s) {
  if (!ap) return -1;
  const AugArgs& a = *static_cast<const AugArgs*>(ap);
  if (!a.src || !a.out || !a.gather || !a.st) return -2;
  if (a.Q <= 0 || a.B <= 0 || a.Hp <= 0 || a.Wp <= 0 || a.Cp <= 0 || a.Cp % 8) return -3;
  if (a.Hr <= 0 || a.Wr <= 0 || a.Hr > a.Hp || a.Wr > a.Wp) return -4;
  if (a.shift < 0 || a.shift >= (a.Hr < a.Wr ? a.Hr : a.Wr)) return -5;
  if (a.prec != 0 && a.prec != 1) return -6;
  const long chunks = (long)a.Hp * a.Wp * (a.Cp / 8);
  const long rows = (long)a.Q * a.B;
  const long dmax = a.Wp > a.Cp / 8 ? a.Wp : a.Cp / 8;
  if (chunks * dmax >= (1L << 32) || rows > 0x7fffffffL) return -7;      // FastDiv's range, grid.x
  const long gy = (chunks + AUG_BLOCK - 1) / AUG_BLOCK;
  if (gy > 65535) return -7;
  const dim3 grid((unsigned)rows, (unsigned)gy);
  if (a.prec) hipLaunchKernelGGL(augment_kernel<1>, grid, dim3(AUG_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(augment_kernel<0>, grid, dim3(AUG_BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
