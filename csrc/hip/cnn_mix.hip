// Mixup / CutMix of the Genetic-CNN training batch, fused with the shift-and-flip augmentation: one pass
// from the device-resident dataset to the batch the first convolution reads (gt_augment then a mixing
// launch would write and re-read that batch once more).
//
// Definition: gentun_amd/models/cnn_engine.py ("The mixed step"); the draw itself is cnn_mix.h. Per group g
// and global step t every real row b < nv is mixed with row p(b) = (b + o) % nv of the same batch:
//   mixup   out = fp32(lam A[b]) + fp32(lam1 A[p(b)])       (bf16 storage: fp32 arithmetic, one f2bf)
//   cutmix  out = A[p(b)] inside the box, A[b] elsewhere     (a select: no arithmetic)
// where A[r] is row r as gt_augment defines it (cnn_augment.hip: its own shift and flip, zero fill, exact
// zeros outside the real extent); shift = 0, flip = 0 is the plain gathered row. A step that is not applied
// and a padding row b >= nv are gt_augment's copy.
//
// The work is split as in augment_kernel: one workgroup column (blockIdx.x) per output row (g, b), one
// 8-channel chunk (16 B bf16, 32 B fp32) per thread, consecutive threads on consecutive chunks of the output
// row, so stores coalesce and a flipped source row is read contiguously in reverse. The flag, o, m, the box
// and both rows' (dy, dx, flip) depend on (g, t, b) only: they are wave-uniform and sit in scalar registers.
// mixup gathers two source chunks, each through its own row's shift and flip, blends them in registers and
// stores once; cutmix picks the row per pixel and gathers exactly one chunk, gt_augment's traffic.

#include <hip/hip_runtime.h>

#include "cnn_mix.h"

#define MIXA_BLOCK 256
#define MIXA_AUG_CTR 0xA0600000u     // cnn_augment.hip AUG_CTR: the rows keep the draws gt_augment gives them

struct MixArgs {
  const void* src;           // dataset [N][Hp][Wp][Cp], bf16 (prec 0) or fp32 (prec 1)
  void* out;                 // mixed batch [Q*B][Hp][Wp][Cp], same type
  const int64_t* gather;     // image table [steps][Q][B]
  const int* valid;          // [steps][Q] real rows of every batch
  const StepState* st;       // cur_step (table row) and global_step (draw key)
  const int* fold_ids;       // [Q] or null (then: the group index)
  const unsigned* seeds;     // [Q] per-group keys or null -> seed
  unsigned seed;
  int Q, B, Hp, Wp, Hr, Wr, Cp;
  int shift, flip;           // the augmentation of every row (0, 0: none)
  int prec;
  int kind;                  // 0 mixup, 1 cutmix
  int alpha;                 // 1 .. MIX_MAX_ALPHA
  unsigned p24;              // round(prob * 2^24), 1 .. 2^24
};

struct MixRowDraw { int dy, dx; bool flip; };

__device__ __forceinline__ MixRowDraw mix_row_draw(const MixArgs& a, uint32_t key, uint32_t t, uint32_t row) {
  const uint32_t span = 2u * (uint32_t)a.shift + 1u;
  MixRowDraw r;
  r.dy = (int)(hash4(key, t, row, MIXA_AUG_CTR + 0u) % span) - a.shift;
  r.dx = (int)(hash4(key, t, row, MIXA_AUG_CTR + 1u) % span) - a.shift;
  r.flip = a.flip && (hash4(key, t, row, MIXA_AUG_CTR + 2u) >> 31);
  return r;
}

// element offset of the source chunk of output pixel (i, j) of a row under draw r, or -1: zero fill
__device__ __forceinline__ int64_t mix_src(const MixArgs& a, const MixRowDraw& r, int64_t img, int i, int j,
                                           uint32_t CB, uint32_t cb) {
  const int si = i - r.dy, u = j - r.dx;
  const bool ok = i < a.Hr && j < a.Wr && si >= 0 && si < a.Hr && u >= 0 && u < a.Wr;
  const int sj = r.flip ? a.Wr - 1 - u : u;
  return ok ? (((img * a.Hp + si) * a.Wp + sj) * (int64_t)CB + cb) * 8 : (int64_t)-1;
}

template <int PREC, int KIND>
__global__ __launch_bounds__(MIXA_BLOCK) void augment_mix_kernel(const MixArgs a) {
  typedef typename ActT<PREC>::T AT;
  const int qb = blockIdx.x;                       // output row g * B + b
  const int g = qb / a.B, b = qb - g * a.B;
  const uint32_t fid = a.fold_ids ? (uint32_t)a.fold_ids[g] : (uint32_t)g;
  const uint32_t key = (a.seeds ? a.seeds[g] : a.seed) ^ (fid * 0x632be5abU);
  const uint32_t t = (uint32_t)a.st->global_step;
  const int64_t tab = ((int64_t)a.st->cur_step * a.Q + g);
  int nv = a.valid[tab];
  nv = nv < a.B ? nv : a.B;                        // the partner stays inside this group's rows of the table
  const MixDraw d = mix_draw(key, t, nv, a.alpha, a.p24);
  const bool mixed = d.applied && b < nv;
  const int pb = mixed ? (int)(((uint32_t)b + d.o) % (uint32_t)nv) : b;
  const MixRowDraw r0 = mix_row_draw(a, key, t, (uint32_t)b), r1 = mix_row_draw(a, key, t, (uint32_t)pb);
  const int64_t img0 = a.gather[tab * a.B + b], img1 = a.gather[tab * a.B + pb];
  MixBox bx = {0, 0, 0, 0};
  float lam = 1.f, lam1 = 0.f;
  if (mixed) {
    if (KIND) bx = mix_box(key, t, d.m, a.Hr, a.Wr);
    else mix_weights(0, d.m, bx, a.Hr, a.Wr, 0.f, lam, lam1);
  }

  const uint32_t CB = (uint32_t)a.Cp >> 3;
  const uint32_t chunks = (uint32_t)a.Hp * a.Wp * CB;
  const uint32_t c = blockIdx.y * MIXA_BLOCK + threadIdx.x;
  if (c >= chunks) return;
  const FastDiv dcb(CB), dw((uint32_t)a.Wp);
  uint32_t px, cb, ui, uj;
  dcb.divmod(c, px, cb);
  dw.divmod(px, ui, uj);
  const int i = (int)ui, j = (int)uj;
  const AT* src = static_cast<const AT*>(a.src);
  AT* dst = static_cast<AT*>(a.out) + ((int64_t)qb * chunks + c) * 8;
  int64_t s0, s1 = -1;
  if (KIND) {
    // cutmix: one source chunk, the partner's inside the box (an empty box for an unmixed row)
    const bool in = i >= bx.y0 && i < bx.y1 && j >= bx.x0 && j < bx.x1;
    MixRowDraw r;
    r.dy = in ? r1.dy : r0.dy;
    r.dx = in ? r1.dx : r0.dx;
    r.flip = in ? r1.flip : r0.flip;
    s0 = mix_src(a, r, in ? img1 : img0, i, j, CB, cb);
  } else {
    s0 = mix_src(a, r0, img0, i, j, CB, cb);
    if (mixed) s1 = mix_src(a, r1, img1, i, j, CB, cb);
  }
  if (PREC) {
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0, w0 = v0, w1 = v0;
    if (s0 >= 0) {
      const float4* p = reinterpret_cast<const float4*>(src + s0);
      v0 = p[0];
      v1 = p[1];
    }
    if (!KIND && mixed) {
      if (s1 >= 0) {
        const float4* p = reinterpret_cast<const float4*>(src + s1);
        w0 = p[0];
        w1 = p[1];
      }
      v0 = make_float4(mix_blend(lam, v0.x, lam1, w0.x), mix_blend(lam, v0.y, lam1, w0.y),
                       mix_blend(lam, v0.z, lam1, w0.z), mix_blend(lam, v0.w, lam1, w0.w));
      v1 = make_float4(mix_blend(lam, v1.x, lam1, w1.x), mix_blend(lam, v1.y, lam1, w1.y),
                       mix_blend(lam, v1.z, lam1, w1.z), mix_blend(lam, v1.w, lam1, w1.w));
    }
    reinterpret_cast<float4*>(dst)[0] = v0;
    reinterpret_cast<float4*>(dst)[1] = v1;
  } else {
    uint4 v = make_uint4(0u, 0u, 0u, 0u), w = v;
    if (s0 >= 0) v = *reinterpret_cast<const uint4*>(src + s0);
    if (!KIND && mixed) {
      if (s1 >= 0) w = *reinterpret_cast<const uint4*>(src + s1);
      const uint32_t vi[4] = {v.x, v.y, v.z, v.w}, wi[4] = {w.x, w.y, w.z, w.w};
      uint32_t r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = mix_blend(lam, bf2f((uint16_t)(vi[e] & 0xffffu)), lam1, bf2f((uint16_t)(wi[e] & 0xffffu)));
        const float hi = mix_blend(lam, bf2f((uint16_t)(vi[e] >> 16)), lam1, bf2f((uint16_t)(wi[e] >> 16)));
        r[e] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
      }
      v = make_uint4(r[0], r[1], r[2], r[3]);
    }
    *reinterpret_cast<uint4*>(dst) = v;
  }
}

extern "C" {

size_t gt_sizeof_mix_args() { return sizeof(MixArgs); }

// Returns non-zero (nothing launched) on arguments the kernel cannot run: gt_augment's refusals, then the
// mix ranges.
int gt_augment_mix(const void* ap, hipStream_t s) {
  if (!ap) return -1;
  const MixArgs& a = *static_cast<const MixArgs*>(ap);
  if (!a.src || !a.out || !a.gather || !a.st) return -2;
  if (a.Q <= 0 || a.B <= 0 || a.Hp <= 0 || a.Wp <= 0 || a.Cp <= 0 || a.Cp % 8) return -3;
  if (a.Hr <= 0 || a.Wr <= 0 || a.Hr > a.Hp || a.Wr > a.Wp) return -4;
  if (a.shift < 0 || a.shift >= (a.Hr < a.Wr ? a.Hr : a.Wr)) return -5;
  if (a.prec != 0 && a.prec != 1) return -6;
  const long chunks = (long)a.Hp * a.Wp * (a.Cp / 8);
  const long rows = (long)a.Q * a.B;
  const long dmax = a.Wp > a.Cp / 8 ? a.Wp : a.Cp / 8;
  if (chunks * dmax >= (1L << 32) || rows > 0x7fffffffL) return -7;      // FastDiv's range, grid.x
  const long gy = (chunks + MIXA_BLOCK - 1) / MIXA_BLOCK;
  if (gy > 65535) return -7;
  if (a.kind != 0 && a.kind != 1) return -8;
  if (a.alpha < 1 || a.alpha > MIX_MAX_ALPHA) return -9;
  if (a.p24 < 1u || a.p24 > MIX_ONE24) return -10;
  if (!a.valid) return -11;
  if (a.Hr > 32767 || a.Wr > 32767) return -12;                          // mix_box's 32-bit squares
  const dim3 grid((unsigned)rows, (unsigned)gy), block(MIXA_BLOCK);
  if (a.prec) {
    if (a.kind) hipLaunchKernelGGL((augment_mix_kernel<1, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((augment_mix_kernel<1, 0>), grid, block, 0, s, a);
  } else {
    if (a.kind) hipLaunchKernelGGL((augment_mix_kernel<0, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((augment_mix_kernel<0, 0>), grid, block, 0, s, a);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
