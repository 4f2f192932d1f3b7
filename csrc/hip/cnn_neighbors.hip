// Nearest neighbours in feature space for fitted Genetic-CNN models on MI355X (gfx950)
// (models/cnn_fitted.py neighbors, models/cnn_ensemble.py).
//
// The feature of an image is the hidden row gt_dense_fwd writes in evaluation mode, [G members][B rows][Up units]
// (fp32 or bf16 by prec), real units only, the members' blocks side by side: D = G * Ur features, stored Dp = G * Up
// wide with zeros in the padding. The search is the [m queries] x [N bank rows] x [Dp] product with a fused
// selection of the k <= 16 nearest bank rows of every query:
//
//   l2      d = max((|q|^2 + |b|^2) - 2 q.b, 0)
//   cosine  d = 1 - q.b / (sqrt(|q|^2) sqrt(|b|^2)),   d = 1 when either norm is 0
//
// in ascending (d, bank index) order -- a total order, a tie goes to the lower index.
//
//   gt_nn_bank   appends rows to the resident bank: bf16 planes [NPL][Np][Dp] (the exact three-way split of
//                common.h for an fp32 fit, one plane for a bf16 fit) and every row's squared norm.
//   gt_nn_topk   the product on the matrix cores and the selection; writes [m][S][k] candidates, S bank slices.
//   gt_nn_merge  merges the S sorted lists of every query.
//
// A squared norm is summed in ONE order wherever it is taken (nn_norm): eight partial sums, partial j over the
// 8-feature chunks c = j, j + 8, ... left to right, then ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)). A dot
// product has one k order (members, then units), no split-K and no atomics; the leading term a0 b0 of the
// six-term product accumulates apart from the five small ones and joins after the last k-step (gt_head_mc records
// why). Every multiply and add of the epilogue is rounded separately. So a distance depends on its own query row
// and bank row only: equal bits for any chunking, any position in a tile and any number of slices, and an exact
// duplicate of a bank row ties with the original bit for bit and loses by index. A distance that overflows to +inf
// (or is NaN) enters no list: a query with fewer than k finite distances gets (+inf, NN_NOIDX) in the places left.

#include "common.h"
#include "cnn_nn_src.h"

#define NN_MAXK 16
#define NN_MAXS 64
#define NN_QT 32             // queries per workgroup
#define NN_BT 128            // bank rows per tile: 32 per wave
#define NN_LD 40             // bf16 per query row of a staged plane: 32 features + 8 of padding (80 B)
#define NN_LISTS 512         // selection lists per workgroup: 16 per query, two per lane
#define NN_NOIDX 0x7fffffff  // index of an empty list entry (distance +inf): sorts after every real pair
#define NN_MAX_PLANE_BYTES (1L << 30)

struct NnBankArgs {
  NnSrc src;                 // src.B rows are readable; row r of the launch is bank row n0 + r
  uint16_t* planes;          // [NPL][Np][G * Up] bf16
  float* norm;               // [Np] squared norms
  int prec;                  // of the fit: 1 three planes, 0 one plane
  int sprec;                 // of the source values: 1 fp32, 0 bf16 (flat sources are fp32)
  int m, rows;               // rows [0, m) are copied, rows [m, rows) are written as zeros (the bank's tail)
  int n0, N, Np;
};

struct NnTopkArgs {
  NnSrc q;                   // the queries: rows [0, m) of gt_dense_fwd's output
  const uint16_t* planes;
  const float* bnorm;
  float* cand_d;             // [m][S][k]
  int* cand_i;               // [m][S][k]
  int prec, m, N, Np, k, S, metric;     // metric 0 l2, 1 cosine
};

struct NnMergeArgs {
  const float* cand_d;
  const int* cand_i;
  float* out_d;              // [m][k]
  int* out_i;                // [m][k]
  int m, S, k;
};

__device__ __forceinline__ float nn_sq8(float s, const float* f) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 8; ++e) s = s + f[e] * f[e];
  return s;
}

// the eight partial sums of eight neighbouring lanes -> the norm, in every one of them
__device__ __forceinline__ float nn_norm(float p) {
#pragma clang fp contract(off)
  p = p + __shfl_xor(p, 1);
  p = p + __shfl_xor(p, 2);
  p = p + __shfl_xor(p, 4);
  return p;
}

// ---------------------------------------------------------------------------------------------------------
// gt_nn_bank: 32 rows per workgroup, 8 lanes per row; lane j splits and stores the chunks j, j + 8, ...
// ---------------------------------------------------------------------------------------------------------
template <int NPL, int SP>
__global__ void __launch_bounds__(256) nn_bank_kernel(const NnBankArgs a) {
  const int r = blockIdx.x * 32 + (threadIdx.x >> 3), j = threadIdx.x & 7;
  if (r >= a.rows) return;                                   // whole groups of 8 lanes leave together
  const int Dp = a.src.G * a.src.Up;
  const int64_t plane = (int64_t)a.Np * Dp;
  uint16_t* dst = a.planes + (int64_t)(a.n0 + r) * Dp;
  const bool real = r < a.m;
  float s = 0.f;
  for (int c = j; c < (Dp >> 3); c += 8) {
    float f[8];
    if (real) {
      nn_chunk<SP>(a.src, r, c, f);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
    }
    if (NPL == 1) {
      const uint4 p0 = pack8(f);
      unpack8(p0, f);                                        // the norm is that of the stored values
      *reinterpret_cast<uint4*>(dst + c * 8) = p0;
    } else {
      uint4 q[3];
      split8(f, q[0], q[1], q[2]);
#pragma unroll
      for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(dst + p * plane + c * 8) = q[p];
    }
    s = nn_sq8(s, f);
  }
  s = nn_norm(s);
  if (j == 0) a.norm[a.n0 + r] = s;
}

// ---------------------------------------------------------------------------------------------------------
// Merging sorted lists, one list per lane of a group of W lanes: k rounds, each a lexicographic minimum of the
// lists' heads over the group (xor butterfly), the owner of the minimum moves on. Lane 0 of a group writes.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool nn_less(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

template <int W>
__device__ __forceinline__ void nn_merge_lists(const float* d, const int* i, int stride, bool have, int k, float* od,
                                               int* oi, bool writer) {
  int head = 0;
  float cd = have ? d[0] : INFINITY;
  int ci = have ? i[0] : NN_NOIDX;
  for (int r = 0; r < k; ++r) {
    float bd = cd;
    int bi = ci;
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
      const float xd = __shfl_xor(bd, off);
      const int xi = __shfl_xor(bi, off);
      if (nn_less(xd, xi, bd, bi)) { bd = xd; bi = xi; }
    }
    if (writer) { od[r] = bd; oi[r] = bi; }
    if (have && cd == bd && ci == bi) {
      ++head;
      cd = head < k ? d[(int64_t)head * stride] : INFINITY;
      ci = head < k ? i[(int64_t)head * stride] : NN_NOIDX;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// gt_nn_topk. Grid (query tiles of 32, S bank slices); a workgroup of 4 waves walks its slice in tiles of 128
// bank rows, wave w owning rows 32w .. 32w + 31 of the tile (two 16-row A tiles) against all 32 queries (two
// 16-column B tiles): four 16x16 accumulator pairs. Per 32-feature k-step:
//   A  lane (l16, kq) loads features kq * 8 .. + 7 of its two bank rows straight from the planes (16-byte
//      loads, prefetched one step ahead, across tile ends too): no wave shares a bank row inside a tile;
//   B  the [32 queries][32 features] slab is what the four waves share: threads 0..127 read 8 features each from
//      gt_dense_fwd's output (member ks / (Up / 32), units (ks % (Up / 32)) * 32 ..), split them and store the
//      planes into LDS, double-buffered over the whole (tile, k-step) sequence, one barrier per step.
// After a tile's last k-step lane (l16, kq) holds, for queries l16 and 16 + l16, the dot products with 8 bank
// rows in ascending order. It forms the distances and feeds them to two selection lists of its own in LDS
// (k sorted pairs each, [entry][list] so that a wave's lanes fall on distinct banks): 16 lists per query, each
// fed in ascending bank index, so "insert when d < the list's worst, behind every entry <= d" is the lexicographic
// order and costs one compare per distance once the lists have filled. No distance tile goes through LDS and the
// selection needs no barrier. After the slice the 16 lists of a query merge (nn_merge_lists) into [m][S][k].
// LDS: 15 KB of staged planes, 128 B of norms, 4 KB x k of lists (20 KB at k = 5, 64 KB at k = 16).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void nn_insert(float* ld, int* li, int L, int k, float d, int idx, float& worst) {
  int j = k - 1;
  while (j > 0 && ld[(j - 1) * NN_LISTS + L] > d) {
    ld[j * NN_LISTS + L] = ld[(j - 1) * NN_LISTS + L];
    li[j * NN_LISTS + L] = li[(j - 1) * NN_LISTS + L];
    --j;
  }
  ld[j * NN_LISTS + L] = d;
  li[j * NN_LISTS + L] = idx;
  worst = ld[(k - 1) * NN_LISTS + L];
}

template <int NPL>
__global__ void __launch_bounds__(256) nn_topk_kernel(const NnTopkArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t sl[2][NPL][NN_QT * NN_LD];
  __shared__ float qn[NN_QT];
  extern __shared__ __attribute__((aligned(16))) unsigned char nn_smem[];
  float* ld = reinterpret_cast<float*>(nn_smem);             // [k][NN_LISTS]
  int* li = reinterpret_cast<int*>(ld + a.k * NN_LISTS);     // [k][NN_LISTS]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4, l16 = lane & 15;
  const int k = a.k, Up = a.q.Up, Dp = a.q.G * Up;
  const int c0 = blockIdx.x * NN_QT;
  const int nku = Up >> 5, nk = Dp >> 5;
  // this slice's tiles
  const int tiles = a.Np / NN_BT, tps = (tiles + a.S - 1) / a.S;
  const int t0 = blockIdx.y * tps, t1 = min(t0 + tps, tiles);
  const int64_t plane = (int64_t)a.Np * Dp;

  for (int e = tid; e < k * NN_LISTS; e += 256) {
    ld[e] = INFINITY;
    li[e] = NN_NOIDX;
  }
  {                                                          // query norms: 8 lanes per query, nn_norm's order
    const int qi = tid >> 3, j = tid & 7;
    const int row = min(c0 + qi, a.m - 1);
    float s = 0.f;
    for (int c = j; c < (Dp >> 3); c += 8) {
      float f[8];
      nn_chunk<(NPL == 3)>(a.q, row, c, f);
      s = nn_sq8(s, f);
    }
    s = nn_norm(s);
    if (j == 0) qn[qi] = s;
  }
  // staging role of threads 0..127: query si of the tile, features sk .. sk + 7 of the k-step
  const int si = tid >> 2, sk = (tid & 3) * 8;
  const bool stager = tid < 128;
  const int srow = min(c0 + si, a.m - 1);
  const bool sok = c0 + si < a.m;
  auto stage = [&](int ks, int buf) {
    const int g = ks / nku, u = (ks - g * nku) * 32 + sk;
    float f[8];
    nn_chunk<(NPL == 3)>(a.q, srow, (g * Up + u) >> 3, f);
    if (!sok) {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
    }
    if (NPL == 1) {
      *reinterpret_cast<uint4*>(&sl[buf][0][si * NN_LD + sk]) = pack8(f);    // exact: the values are bf16
    } else {
      uint4 q[3];
      split8(f, q[0], q[1], q[2]);
#pragma unroll
      for (int p = 0; p < NPL; ++p) *reinterpret_cast<uint4*>(&sl[buf][p][si * NN_LD + sk]) = q[p];
    }
  };
  // bank fragments of (tile t, k-step ks): rows t * 128 + 32 wave + 16 rt + l16 < Np, the planes hold them
  auto fetch = [&](int t, int ks, uint4 (*fr)[NPL]) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const uint16_t* p = a.planes + (int64_t)(t * NN_BT + wave * 32 + rt * 16 + l16) * Dp + ks * 32 + kq * 8;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) fr[rt][pl] = *reinterpret_cast<const uint4*>(p + pl * plane);
    }
  };

  float worst[2] = {INFINITY, INFINITY};
  if (t0 < t1) {                                             // block-uniform
    uint4 af[2][NPL], an[2][NPL];
    fetch(t0, 0, af);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) an[rt][pl] = af[rt][pl];
    if (stager) stage(0, 0);
    __syncthreads();                                         // buffer 0, the norms and the empty lists
    f32x4_t acc[2][2], lo[2][2];
    int cur = 0;
    for (int t = t0; t < t1; ++t) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = lo[rt][ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < nk; ++ks) {
        const bool last = ks + 1 == nk;
        if (!last || t + 1 < t1) {                           // block-uniform: the next step of the sequence
          fetch(last ? t + 1 : t, last ? 0 : ks + 1, an);
          if (stager) stage(last ? 0 : ks + 1, cur ^ 1);
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          uint4 bf[NPL];
#pragma unroll
          for (int p = 0; p < NPL; ++p)
            bf[p] = *reinterpret_cast<const uint4*>(&sl[cur][p][(ct * 16 + l16) * NN_LD + kq * 8]);
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {                   // D[row = bank row][col = query]
            if (NPL == 1) {
              acc[rt][ct] = mfma16(af[rt][0], bf[0], acc[rt][ct]);
            } else {                                         // mfma_np<3>'s terms, smallest first
              lo[rt][ct] = mfma16(af[rt][NPL - 1], bf[0], lo[rt][ct]);
              lo[rt][ct] = mfma16(af[rt][NPL / 2], bf[NPL / 2], lo[rt][ct]);
              lo[rt][ct] = mfma16(af[rt][0], bf[NPL - 1], lo[rt][ct]);
              lo[rt][ct] = mfma16(af[rt][NPL / 2], bf[0], lo[rt][ct]);
              lo[rt][ct] = mfma16(af[rt][0], bf[NPL / 2], lo[rt][ct]);
              acc[rt][ct] = mfma16(af[rt][0], bf[0], acc[rt][ct]);
            }
          }
        }
        __syncthreads();           // buffer `cur` is free for the step after next, buffer `cur ^ 1` is complete
        cur ^= 1;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) af[rt][pl] = an[rt][pl];
      }
      // the tile's distances into this lane's lists: query ct * 16 + l16, bank rows ascending
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float q2 = qn[ct * 16 + l16];
        const int L = ct * 256 + tid;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          const int b0 = t * NN_BT + wave * 32 + rt * 16 + kq * 4;
          const float4 b2 = *reinterpret_cast<const float4*>(a.bnorm + b0);
          const float bn[4] = {b2.x, b2.y, b2.z, b2.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float d;
            {
#pragma clang fp contract(off)
              const float dot = NPL == 1 ? acc[rt][ct][i] : acc[rt][ct][i] + lo[rt][ct][i];
              if (a.metric == 0) {
                const float n2 = q2 + bn[i];
                d = fmaxf(n2 - 2.f * dot, 0.f);
              } else {
                const float den = sqrtf(q2) * sqrtf(bn[i]);
                d = (q2 == 0.f || bn[i] == 0.f) ? 1.f : 1.f - dot / den;
              }
            }
            if (b0 + i >= a.N) d = INFINITY;                 // the bank's tail never enters a list
            if (d < worst[ct]) nn_insert(ld, li, L, k, d, b0 + i, worst[ct]);
          }
        }
      }
    }
  }
  __syncthreads();                 // every list is final (and, for an empty slice, initialised)
  // 16 lanes per query, one list each: list (wave', kq') of query (ct, l16') is ct * 256 + 64 wave' + 16 kq' + l16'
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int gq = tid >> 4, sub = tid & 15;
    const int query = c0 + ct * 16 + gq;
    const int L = ct * 256 + (sub >> 2) * 64 + (sub & 3) * 16 + gq;
    const bool ok = query < a.m;
    const int64_t o = ((int64_t)min(query, a.m - 1) * a.S + blockIdx.y) * k;
    nn_merge_lists<16>(ld + L, li + L, NN_LISTS, true, k, a.cand_d + o, a.cand_i + o, ok && sub == 0);
  }
}

// ---------------------------------------------------------------------------------------------------------
// gt_nn_merge: one wave per query, lane s holds slice s's list; four queries per workgroup.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) nn_merge_kernel(const NnMergeArgs a) {
  const int query = blockIdx.x * 4 + (threadIdx.x >> 6), s = threadIdx.x & 63;
  if (query >= a.m) return;                                  // a whole wave
  const bool have = s < a.S;
  const int64_t at = ((int64_t)query * a.S + (have ? s : 0)) * a.k;
  nn_merge_lists<64>(a.cand_d + at, a.cand_i + at, 1, have, a.k, a.out_d + (int64_t)query * a.k,
                     a.out_i + (int64_t)query * a.k, s == 0);
}

static bool nn_bank_ok(int prec, int N, int Np, long Dp) {
  if (prec != 0 && prec != 1) return false;
  if (N < 1 || N > 0x7fffffff - NN_BT || Np != (N + NN_BT - 1) / NN_BT * NN_BT) return false;
  return (long)Np * Dp * 2 * (prec ? 3 : 1) <= NN_MAX_PLANE_BYTES;
}

extern "C" {

size_t gt_sizeof_nn_bank_args() { return sizeof(NnBankArgs); }
size_t gt_sizeof_nn_topk_args() { return sizeof(NnTopkArgs); }
size_t gt_sizeof_nn_merge_args() { return sizeof(NnMergeArgs); }
int gt_nn_max_k() { return NN_MAXK; }
int gt_nn_max_slices() { return NN_MAXS; }
int gt_nn_bank_tile() { return NN_BT; }

// Every launcher returns a negative code (nothing launched) on arguments its kernel cannot run.
int gt_nn_bank(const NnBankArgs* a, hipStream_t s) {
  if (!a || !a->planes || !a->norm) return -1;
  if (a->sprec != 0 && a->sprec != 1) return -2;
  if (a->m < 0 || a->rows < 1 || a->m > a->rows) return -3;
  if (!nn_src_ok(a->src, a->m > 0 ? a->m : 1, a->sprec)) return -2;
  if (!nn_bank_ok(a->prec, a->N, a->Np, (long)a->src.G * a->src.Up)) return -4;
  if (a->prec == 1 && a->sprec == 0) return -2;              // an fp32 fit has fp32 features
  if (a->n0 < 0 || (long)a->n0 + a->m > a->N || (long)a->n0 + a->rows > a->Np) return -3;
  const dim3 grid((unsigned)((a->rows + 31) / 32));
  if (a->prec) hipLaunchKernelGGL((nn_bank_kernel<3, 1>), grid, dim3(256), 0, s, *a);
  else if (a->sprec) hipLaunchKernelGGL((nn_bank_kernel<1, 1>), grid, dim3(256), 0, s, *a);
  else hipLaunchKernelGGL((nn_bank_kernel<1, 0>), grid, dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

// dynamic LDS of gt_nn_topk at k: the selection lists
size_t gt_nn_topk_lds(int k) { return (size_t)k * NN_LISTS * 8; }

int gt_nn_topk(const NnTopkArgs* a, hipStream_t s) {
  if (!a || !a->planes || !a->bnorm || !a->cand_d || !a->cand_i) return -1;
  if (a->prec != 0 && a->prec != 1) return -2;
  if (a->m < 1 || !nn_src_ok(a->q, a->m, a->prec) || a->q.flat) return -2;
  if (!nn_bank_ok(a->prec, a->N, a->Np, (long)a->q.G * a->q.Up)) return -4;
  if (a->k < 1 || a->k > NN_MAXK || a->k > a->N) return -5;
  if (a->S < 1 || a->S > NN_MAXS) return -6;
  if (a->metric != 0 && a->metric != 1) return -7;
  const size_t lds = gt_nn_topk_lds(a->k);
  const bool big = lds > 48 * 1024;                          // with the static 15.5 KB: past the 64 KiB default
  const dim3 grid((unsigned)((a->m + NN_QT - 1) / NN_QT), (unsigned)a->S);
  if (a->prec) {
    if (big && hipFuncSetAttribute(reinterpret_cast<const void*>(nn_topk_kernel<3>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return -8;
    hipLaunchKernelGGL(nn_topk_kernel<3>, grid, dim3(256), lds, s, *a);
  } else {
    if (big && hipFuncSetAttribute(reinterpret_cast<const void*>(nn_topk_kernel<1>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return -8;
    hipLaunchKernelGGL(nn_topk_kernel<1>, grid, dim3(256), lds, s, *a);
  }
  return (int)hipGetLastError();
}

int gt_nn_merge(const NnMergeArgs* a, hipStream_t s) {
  if (!a || !a->cand_d || !a->cand_i || !a->out_d || !a->out_i) return -1;
  if (a->m < 1) return -2;
  if (a->k < 1 || a->k > NN_MAXK) return -5;
  if (a->S < 1 || a->S > NN_MAXS) return -6;
  hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)((a->m + 3) / 4)), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

}  // extern "C"
