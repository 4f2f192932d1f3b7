// Class-conditional Gaussians with a tied covariance in the feature space of fitted Genetic-CNN models on MI355X
// (gfx950) (models/cnn_fitted.py gaussian_fit / mahalanobis, models/cnn_ensemble.py).
//
// The features are those of cnn_neighbors.hip: the hidden rows gt_dense_fwd writes in evaluation mode, kept for the
// request as a feature store [G members][Np rows][Up units] (fp32 or bf16 by the fit), or a flat fp32 [N][ld] array
// of embeddings; both are an NnSrc. Units >= Ur and rows >= N count as zeros whatever the memory holds.
//
//   gt_fs_sums     per-class column sums in fp64, one partial per slice of FS_SLICE_ROWS rows: [S][G][C][Up]
//   gt_fs_center   c = fp32(f - mean[label]) split into three bf16 planes (common.h split8), written FEATURE-MAJOR
//                  [3][G][Up][Np] through an LDS transpose: with rows contiguous both operands of the scatter are
//                  16-byte loads along K straight from global memory
//   gt_fs_scatter  C^T C per member on v_mfma_f32_16x16x32_bf16, six-term order, K = rows: one fp32 partial
//                  [Up][Up] (upper-triangle tiles) per slice of FS_SLICE_ROWS rows
//   gt_fs_reduce   the slices' partials in slice order into fp64 [G][Up][Up]; the last round mirrors the triangle
//   gt_fs_dist     z = f W on the matrix cores with the per-class epilogue d_c = sum_j (z_j - t_cj)^2 fused:
//                  z never goes to memory; writes [G][rows][C]
//
// No atomics, no split of a sum that depends on the launch: a partial sum covers the rows of one slice in row
// order, slices join in slice order, so every result depends on the shapes (N, Up, C) only, never on how the rows
// arrived (batch, chunks) or on how many slices a round of gt_fs_scatter / gt_fs_reduce holds.

#include "common.h"
#include "cnn_nn_src.h"

#define FS_SLICE_ROWS 1024   // rows of one fp32 partial sum (32 k-steps)
#define FS_ROW_PAD 64        // Np is N rounded up to this: the row tile of gt_fs_center
#define FS_MAXC 16
#define FS_TILE 128          // output tile of gt_fs_scatter, 64 x 64 per wave
#define FS_QT 32             // queries per workgroup of gt_fs_dist
#define FS_CT 128            // columns of z per tile of gt_fs_dist: 32 per wave
#define FS_LD 40             // bf16 per query row of a staged plane: 32 features + 8 of padding (80 B)
#define FS_TLD 72            // bf16 per unit of gt_fs_center's transpose tile: 64 rows + 8 of padding (144 B)
#define FS_MAX_UP 8192
#define FS_MAX_STORE_BYTES (1L << 30)
#define FS_MAX_PART_BYTES (1L << 30)

struct FsSumsArgs {
  NnSrc src;                 // rows [0, N) are readable
  const int* label;          // [N] in [0, C)
  double* part;              // [S][G][C][Up], S = ceil(N / FS_SLICE_ROWS)
  int sprec, N, C;           // sprec: 1 fp32 values, 0 bf16
};

struct FsCenterArgs {
  NnSrc src;
  const int* label;
  const float* mean;         // [G][C][Up]
  uint16_t* planes;          // [3][G][Up][Np]
  int sprec, N, Np, C;
};

struct FsScatterArgs {
  const uint16_t* planes;
  float* part;               // [ns][G][Up][Up]: slice s0 + y of the launch at y
  int G, Up, Np, s0, ns;
};

struct FsReduceArgs {
  const float* part;
  double* acc;               // [G][Up][Up]
  int G, Up, ns, first, last;    // first: the accumulator starts at 0; last: mirror the upper triangle
};

struct FsDistArgs {
  NnSrc q;                   // the queries: rows [0, m) of gt_dense_fwd's output
  const uint16_t* wt;        // [3][G][Up j][Up i]: the planes of W^T, zeros in the padding
  const float* wmean;        // [G][C][Up]
  float* out;                // [G][ldo][C]: row r of the launch is row r0 + r
  int sprec, m, C, empty;    // empty: bit c set -> class c has no rows, its distance is +inf
  int r0, ldo;
};

template <int SP>
__device__ __forceinline__ float fs_elem(const NnSrc& s, int row, int g, int u) {
  if (s.flat) return static_cast<const float*>(s.h)[(int64_t)row * s.ld + g * s.Ur + u];
  const int64_t at = ((int64_t)g * s.B + row) * s.Up + u;
  return SP ? static_cast<const float*>(s.h)[at] : bf2f(static_cast<const uint16_t*>(s.h)[at]);
}

// ---------------------------------------------------------------------------------------------------------
// gt_fs_sums. Grid (G * Up / 64, S), 64 threads: a thread owns one (member, unit) column, walks the slice's rows
// in row order and adds into its own [C] fp64 slots in LDS ([class][thread]: no conflicts, no dynamic register
// indexing). The label of a row is wave-uniform.
// ---------------------------------------------------------------------------------------------------------
template <int SP>
__global__ void __launch_bounds__(64) fs_sums_kernel(const FsSumsArgs a) {
  __shared__ double acc[FS_MAXC][64];
  const int tid = threadIdx.x, col = blockIdx.x * 64 + tid;
  const int Up = a.src.Up, g = col / Up, u = col - g * Up;
  for (int c = 0; c < a.C; ++c) acc[c][tid] = 0.0;
  if (g >= a.src.G) return;
  const int r0 = blockIdx.y * FS_SLICE_ROWS, r1 = min(r0 + FS_SLICE_ROWS, a.N);
  if (u < a.src.Ur) {
    for (int r = r0; r < r1; ++r) {
      const int y = a.label[r];
      if (y >= 0 && y < a.C) acc[y][tid] += (double)fs_elem<SP>(a.src, r, g, u);
    }
  }
  for (int c = 0; c < a.C; ++c)
    a.part[(((int64_t)blockIdx.y * a.src.G + g) * a.C + c) * Up + u] = acc[c][tid];
}

// ---------------------------------------------------------------------------------------------------------
// gt_fs_center. Grid (Np / 64, G * Up / 32), 256 threads: a tile of 64 rows x 32 units of one member. Thread t
// reads 8 units of row t / 4, centres and splits them and scatters the three planes into LDS [plane][unit][row];
// then thread t stores, per plane, 8 rows of unit t / 8 with one 16-byte store.
// ---------------------------------------------------------------------------------------------------------
template <int SP>
__global__ void __launch_bounds__(256) fs_center_kernel(const FsCenterArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t sl[3][32 * FS_TLD];
  const int tid = threadIdx.x, Up = a.src.Up;
  const int r0 = blockIdx.x * FS_ROW_PAD, ub = blockIdx.y * 32, g = ub / Up, u0 = ub - g * Up;
  {
    const int rl = tid >> 2, ch = (tid & 3) * 8, row = r0 + rl;
    float f[8];
    if (row < a.N) {
      float mu[8];
      nn_chunk<SP>(a.src, row, (ub + ch) >> 3, f);
      const int y = min(max(a.label[row], 0), a.C - 1);
      load8f(a.mean + ((int64_t)g * a.C + y) * Up + u0 + ch, mu);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = u0 + ch + e < a.src.Ur ? f[e] - mu[e] : 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
    }
    uint4 q[3];
    split8(f, q[0], q[1], q[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const uint32_t w[4] = {q[p].x, q[p].y, q[p].z, q[p].w};
#pragma unroll
      for (int e = 0; e < 8; ++e)
        sl[p][(ch + e) * FS_TLD + rl] = (uint16_t)(e & 1 ? w[e >> 1] >> 16 : w[e >> 1] & 0xffffu);
    }
  }
  __syncthreads();
  const int ul = tid >> 3, rc = (tid & 7) * 8;
  const int64_t plane = (int64_t)a.src.G * Up * a.Np;
#pragma unroll
  for (int p = 0; p < 3; ++p)
    *reinterpret_cast<uint4*>(a.planes + p * plane + (int64_t)(ub + ul) * a.Np + r0 + rc) =
        *reinterpret_cast<const uint4*>(&sl[p][ul * FS_TLD + rc]);
}

// ---------------------------------------------------------------------------------------------------------
// gt_fs_scatter. Grid (upper-triangle tile pairs (ti <= tj), slices, members); a workgroup of 4 waves owns the
// 128 x 128 tile out[i][j], i in tile ti, j in tile tj, wave (wr, wc) its 64 x 64 quarter: four 16-unit A tiles
// (units i) against four 16-unit B tiles (units j), 16 accumulator pairs. K is the row axis: per 32-row k-step
// lane (l16, kq) loads rows kq * 8 .. + 7 of its unit of every tile, one 16-byte load per plane straight from the
// feature-major planes, prefetched one k-step ahead; A[i][k] and B[k][j] have the same fragment layout, so both
// come from the same planes. The leading term a0 b0 accumulates apart from the five small ones and joins after the
// slice's last k-step (as in gt_nn_topk). A wave whose quarter lies outside the matrix or wholly below the
// diagonal leaves at once; units past Up are clamped for the loads and never stored. No LDS, no barrier.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fs_scatter_kernel(const FsScatterArgs a) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4, l16 = lane & 15;
  const int Up = a.Up, T = (Up + FS_TILE - 1) / FS_TILE, g = blockIdx.z;
  int ti = 0, rem = blockIdx.x;
  while (rem >= T - ti) { rem -= T - ti; ++ti; }
  const int tj = ti + rem;
  const int ib = ti * FS_TILE + (wave >> 1) * 64, jb = tj * FS_TILE + (wave & 1) * 64;
  if (ib >= Up || jb >= Up || ib > jb) return;               // wave-uniform
  const int64_t plane = (int64_t)a.G * Up * a.Np;
  const int rb = (a.s0 + blockIdx.y) * FS_SLICE_ROWS, nk = (min(rb + FS_SLICE_ROWS, a.Np) - rb) >> 5;
  const uint16_t* pa[4];
  const uint16_t* pb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    pa[t] = a.planes + ((int64_t)g * Up + min(ib + t * 16 + l16, Up - 1)) * a.Np + rb + kq * 8;
    pb[t] = a.planes + ((int64_t)g * Up + min(jb + t * 16 + l16, Up - 1)) * a.Np + rb + kq * 8;
  }
  auto fetch = [&](int ks, uint4 (*fa)[3], uint4 (*fb)[3]) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[t][p] = *reinterpret_cast<const uint4*>(pa[t] + p * plane + ks * 32);
        fb[t][p] = *reinterpret_cast<const uint4*>(pb[t] + p * plane + ks * 32);
      }
  };
  f32x4_t acc[4][4], lo[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = lo[rt][ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  uint4 fa[4][3], fb[4][3], na[4][3], nb[4][3];
  fetch(0, fa, fb);
  for (int ks = 0; ks < nk; ++ks) {
    if (ks + 1 < nk) fetch(ks + 1, na, nb);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {                       // mfma_np<3>'s terms, smallest first
        lo[rt][ct] = mfma16(fa[rt][2], fb[ct][0], lo[rt][ct]);
        lo[rt][ct] = mfma16(fa[rt][1], fb[ct][1], lo[rt][ct]);
        lo[rt][ct] = mfma16(fa[rt][0], fb[ct][2], lo[rt][ct]);
        lo[rt][ct] = mfma16(fa[rt][1], fb[ct][0], lo[rt][ct]);
        lo[rt][ct] = mfma16(fa[rt][0], fb[ct][1], lo[rt][ct]);
        acc[rt][ct] = mfma16(fa[rt][0], fb[ct][0], acc[rt][ct]);
      }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[t][p] = na[t][p];
        fb[t][p] = nb[t][p];
      }
  }
  float* out = a.part + ((int64_t)blockIdx.y * a.G + g) * Up * Up;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) {                          // D[row kq * 4 + e][col l16]
        const int i = ib + rt * 16 + kq * 4 + e, j = jb + ct * 16 + l16;
        if (i < Up && j < Up) out[(int64_t)i * Up + j] = acc[rt][ct][e] + lo[rt][ct][e];
      }
}

// ---------------------------------------------------------------------------------------------------------
// gt_fs_reduce: one thread per entry (i <= j) of a member's matrix, the round's slices in slice order.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fs_reduce_kernel(const FsReduceArgs a) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x, UU = (int64_t)a.Up * a.Up;
  if (at >= UU) return;
  const int i = (int)(at / a.Up), j = (int)(at - (int64_t)i * a.Up), g = blockIdx.y;
  if (i > j) return;
  double* acc = a.acc + g * UU;
  double s = a.first ? 0.0 : acc[at];
  for (int k = 0; k < a.ns; ++k) s += (double)a.part[((int64_t)k * a.G + g) * UU + at];
  acc[at] = s;
  if (a.last) acc[(int64_t)j * a.Up + i] = s;
}

// ---------------------------------------------------------------------------------------------------------
// gt_fs_dist. Grid (query tiles of 32, members); a workgroup of 4 waves walks the Up columns of z in tiles of
// 128, wave w owning columns 32w .. 32w + 31 of the tile (two 16-row A tiles of W^T) against all 32 queries (two
// 16-column B tiles), k over the member's Up units. The operands move as in gt_nn_topk: the W^T fragments come
// straight from the planes (prefetched one step ahead, across tile ends), the [32 queries][32 units] slab is split
// on the fly by threads 0..127 and double-buffered in LDS, one barrier per k-step. After a tile's last k-step lane
// (l16, kq) holds z_j of queries l16 and 16 + l16 for 8 columns j and adds (z_j - t_cj)^2 for every class c < C
// to registers of its own, every operation rounded separately, columns ascending. After the last tile the 16
// partial sums of a (query, class) -- (wave, kq) in ascending order -- are added through LDS in that order, so a
// row's distances do not depend on where it sits in the launch. LDS: 15 KB of staged planes, 32 KB of partials.
// ---------------------------------------------------------------------------------------------------------
template <int SP>
__global__ void __launch_bounds__(256) fs_dist_kernel(const FsDistArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t sl[2][3][FS_QT * FS_LD];
  __shared__ float red[16][FS_QT][FS_MAXC];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4, l16 = lane & 15;
  const int Up = a.q.Up, Ur = a.q.Ur, C = a.C, g = blockIdx.y;
  const int c0 = blockIdx.x * FS_QT;
  const int nk = Up >> 5, tiles = (Up + FS_CT - 1) / FS_CT;
  const int64_t plane = (int64_t)a.q.G * Up * Up;
  const int si = tid >> 2, sk = (tid & 3) * 8;
  const bool stager = tid < 128;
  const int srow = min(c0 + si, a.m - 1);
  const bool sok = c0 + si < a.m;
  auto stage = [&](int ks, int buf) {
    float f[8];
    nn_chunk<SP>(a.q, srow, (g * Up + ks * 32 + sk) >> 3, f);
    if (!sok) {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
    }
    uint4 q[3];
    split8(f, q[0], q[1], q[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(&sl[buf][p][si * FS_LD + sk]) = q[p];
  };
  // W^T fragments of (tile t, k-step ks): rows (columns of z) t * 128 + 32 wave + 16 rt + l16, clamped to Up - 1
  auto fetch = [&](int t, int ks, uint4 (*fr)[3]) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int j = min(t * FS_CT + wave * 32 + rt * 16 + l16, Up - 1);
      const uint16_t* p = a.wt + ((int64_t)g * Up + j) * Up + ks * 32 + kq * 8;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) fr[rt][pl] = *reinterpret_cast<const uint4*>(p + pl * plane);
    }
  };
  float d[2][FS_MAXC];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int c = 0; c < FS_MAXC; ++c) d[ct][c] = 0.f;
  uint4 af[2][3], an[2][3];
  fetch(0, 0, af);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) an[rt][pl] = af[rt][pl];
  if (stager) stage(0, 0);
  __syncthreads();
  f32x4_t acc[2][2], lo[2][2];
  int cur = 0;
  for (int t = 0; t < tiles; ++t) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = lo[rt][ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nk; ++ks) {
      const bool last = ks + 1 == nk;
      if (!last || t + 1 < tiles) {                          // block-uniform: the next step of the sequence
        fetch(last ? t + 1 : t, last ? 0 : ks + 1, an);
        if (stager) stage(last ? 0 : ks + 1, cur ^ 1);
      }
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        uint4 bf[3];
#pragma unroll
        for (int p = 0; p < 3; ++p)
          bf[p] = *reinterpret_cast<const uint4*>(&sl[cur][p][(ct * 16 + l16) * FS_LD + kq * 8]);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {                     // D[row = column j of z][col = query]
          lo[rt][ct] = mfma16(af[rt][2], bf[0], lo[rt][ct]);
          lo[rt][ct] = mfma16(af[rt][1], bf[1], lo[rt][ct]);
          lo[rt][ct] = mfma16(af[rt][0], bf[2], lo[rt][ct]);
          lo[rt][ct] = mfma16(af[rt][1], bf[0], lo[rt][ct]);
          lo[rt][ct] = mfma16(af[rt][0], bf[1], lo[rt][ct]);
          acc[rt][ct] = mfma16(af[rt][0], bf[0], acc[rt][ct]);
        }
      }
      __syncthreads();             // buffer `cur` is free for the step after next, buffer `cur ^ 1` is complete
      cur ^= 1;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) af[rt][pl] = an[rt][pl];
    }
    // the tile's z entries into this lane's class sums: query ct * 16 + l16, columns ascending
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int j0 = t * FS_CT + wave * 32 + rt * 16 + kq * 4;
      if (j0 < Ur) {                                         // Ur <= Up: the float4 of means below is in bounds
#pragma unroll
        for (int c = 0; c < FS_MAXC; ++c) {
          if (c < C) {
            const float4 t4 = *reinterpret_cast<const float4*>(a.wmean + ((int64_t)g * C + c) * Up + j0);
            const float tc[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)
                const float z = acc[rt][ct][e] + lo[rt][ct][e];
                const float df = z - tc[e];
                if (j0 + e < Ur) d[ct][c] = d[ct][c] + df * df;
              }
          }
        }
      }
    }
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int c = 0; c < FS_MAXC; ++c) red[wave * 4 + kq][ct * 16 + l16][c] = d[ct][c];
  __syncthreads();
  for (int at = tid; at < FS_QT * C; at += 256) {
    const int q = at / C, c = at - q * C;
    float s = red[0][q][c];
    {
#pragma clang fp contract(off)
      for (int p = 1; p < 16; ++p) s = s + red[p][q][c];
    }
    if (c0 + q < a.m)
      a.out[((int64_t)g * a.ldo + a.r0 + c0 + q) * C + c] = (a.empty >> c) & 1 ? INFINITY : s;
  }
}

static bool fs_rows_ok(const NnSrc& s, int sprec, int N, int Np) {
  if (sprec != 0 && sprec != 1) return false;
  if (N < 1 || N > 0x7fffffff - FS_SLICE_ROWS || !nn_src_ok(s, N, sprec) || s.Up > FS_MAX_UP) return false;
  if (Np && Np != (N + FS_ROW_PAD - 1) / FS_ROW_PAD * FS_ROW_PAD) return false;
  return (long)s.G * s.Up * (Np ? Np : N) * 4 <= FS_MAX_STORE_BYTES;
}

extern "C" {

size_t gt_sizeof_fs_sums_args() { return sizeof(FsSumsArgs); }
size_t gt_sizeof_fs_center_args() { return sizeof(FsCenterArgs); }
size_t gt_sizeof_fs_scatter_args() { return sizeof(FsScatterArgs); }
size_t gt_sizeof_fs_reduce_args() { return sizeof(FsReduceArgs); }
size_t gt_sizeof_fs_dist_args() { return sizeof(FsDistArgs); }
int gt_fs_slice_rows() { return FS_SLICE_ROWS; }
int gt_fs_row_pad() { return FS_ROW_PAD; }
int gt_fs_max_classes() { return FS_MAXC; }

// Every launcher returns a negative code (nothing launched) on arguments its kernel cannot run.
int gt_fs_sums(const FsSumsArgs* a, hipStream_t s) {
  if (!a || !a->label || !a->part) return -1;
  if (!fs_rows_ok(a->src, a->sprec, a->N, 0)) return -2;
  if (a->C < 1 || a->C > FS_MAXC) return -3;
  const dim3 grid((unsigned)(a->src.G * a->src.Up / 64 + (a->src.G * a->src.Up % 64 ? 1 : 0)),
                  (unsigned)((a->N + FS_SLICE_ROWS - 1) / FS_SLICE_ROWS));
  if (a->sprec) hipLaunchKernelGGL(fs_sums_kernel<1>, grid, dim3(64), 0, s, *a);
  else hipLaunchKernelGGL(fs_sums_kernel<0>, grid, dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}

int gt_fs_center(const FsCenterArgs* a, hipStream_t s) {
  if (!a || !a->label || !a->mean || !a->planes) return -1;
  if (!fs_rows_ok(a->src, a->sprec, a->N, a->Np)) return -2;
  if (a->C < 1 || a->C > FS_MAXC) return -3;
  const dim3 grid((unsigned)(a->Np / FS_ROW_PAD), (unsigned)(a->src.G * a->src.Up / 32));
  if (a->sprec) hipLaunchKernelGGL(fs_center_kernel<1>, grid, dim3(256), 0, s, *a);
  else hipLaunchKernelGGL(fs_center_kernel<0>, grid, dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

int gt_fs_scatter(const FsScatterArgs* a, hipStream_t s) {
  if (!a || !a->planes || !a->part) return -1;
  if (a->G < 1 || a->Up < 32 || a->Up % 32 || a->Up > FS_MAX_UP || (long)a->G * a->Up > (1L << 20)) return -2;
  if (a->Np < FS_ROW_PAD || a->Np % FS_ROW_PAD || (long)a->G * a->Up * a->Np * 4 > FS_MAX_STORE_BYTES) return -2;
  const int S = (a->Np + FS_SLICE_ROWS - 1) / FS_SLICE_ROWS;
  if (a->ns < 1 || a->ns > 65535 || a->s0 < 0 || a->s0 + a->ns > S || a->G > 65535) return -4;
  if ((long)a->ns * a->G * a->Up * a->Up * 4 > FS_MAX_PART_BYTES) return -5;
  const int T = (a->Up + FS_TILE - 1) / FS_TILE;
  hipLaunchKernelGGL(fs_scatter_kernel, dim3((unsigned)(T * (T + 1) / 2), (unsigned)a->ns, (unsigned)a->G),
                     dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

int gt_fs_reduce(const FsReduceArgs* a, hipStream_t s) {
  if (!a || !a->part || !a->acc) return -1;
  if (a->G < 1 || a->G > 65535 || a->Up < 32 || a->Up % 32 || a->Up > FS_MAX_UP) return -2;
  if (a->ns < 1 || (long)a->ns * a->G * a->Up * a->Up * 4 > FS_MAX_PART_BYTES) return -5;
  const long UU = (long)a->Up * a->Up;
  hipLaunchKernelGGL(fs_reduce_kernel, dim3((unsigned)((UU + 255) / 256), (unsigned)a->G), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

int gt_fs_dist(const FsDistArgs* a, hipStream_t s) {
  if (!a || !a->wt || !a->wmean || !a->out) return -1;
  if (a->sprec != 0 && a->sprec != 1) return -2;
  if (a->m < 1 || !nn_src_ok(a->q, a->m, a->sprec) || a->q.flat || a->q.Up > FS_MAX_UP || a->q.G > 65535) return -2;
  if (a->C < 1 || a->C > FS_MAXC) return -3;
  if (a->r0 < 0 || a->ldo < 1 || (long)a->r0 + a->m > a->ldo) return -4;
  const dim3 grid((unsigned)((a->m + FS_QT - 1) / FS_QT), (unsigned)a->q.G);
  if (a->sprec) hipLaunchKernelGGL(fs_dist_kernel<1>, grid, dim3(256), 0, s, *a);
  else hipLaunchKernelGGL(fs_dist_kernel<0>, grid, dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

}  // extern "C"
