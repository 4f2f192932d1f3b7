// SHAP interaction values (Booster.predict(pred_interactions=True)) on MI355X, bit-identical to the CPU predictor
// (csrc/gbdt/engine.cpp gbdt_predict_interactions). The definition, the per-leaf pair arithmetic and the finishing
// step are csrc/gbdt/shap_interactions.h, on the element tables of csrc/gbdt/shap_tables.h; the latter switches
// fp contraction off for this whole translation unit. Nothing here divides. Plain HIP only: no inline assembly,
// no atomics.
//
// Kernel contract: grid = (row blocks, K, S). Every accumulator (row, class, i, j) has exactly one owning thread,
// which performs its additions in the header's order (the class's trees in round order, leaves by compact node
// index, pairs in element order). No atomics, no cross-thread reduction of a Phi.
//
// Where the accumulators live: in global memory, [class][i][j][row] (phi_i in the slot (i, i)), K F^2 8 bytes
// per row, each read-modify-written by its owner only. All lanes of a wave work on the same leaf and pair at the
// same time, hence on the same (i, j) of 64 consecutive rows: one contiguous 512-byte access. Chunking rule:
// rows go through the device in chunks of min(chunk_rows, n, 256 MB / (K (F + 1)^2 8), 2^20) rows, so that the
// output chunk [rows][K][F + 1][F + 1] stays within 256 MB: 30,812 rows at F = 32, 508 at F = 256. The row stride
// of the accumulators is the chunk rounded up to 8 rows (64-byte segments) where the chunk holds a whole wave and
// the padded buffer still fits 256 MB, else the chunk itself. A single row beyond 256 MB (F = 8200 is 538 MB)
// is refused with -4.
//
// Parallelism beyond rows: the feature-axis split S = grid z. Accumulator (i, j) only ever receives pairs whose
// first feature is i, so block z = s owns the first indices i with i mod S == s (S a power of two) and the phi_i
// of those features. A thread skips every leaf that has none of its features (no extend, no row reads); for the
// others it repeats the extend and computes the pairs that touch one of its features -- in the header's one
// order, the earlier element unwound first, so both owners of a pair get the same bits -- and keeps its half.
// S is the smallest power of two that gives the launch SI_FILL = 1024 workgroups, at most SI_MAXSPLIT = 256 and
// at most F: 1 from 128 K rows on, 8 at 20,000 rows, one owner per feature at 500 rows of 256 features. The
// kernel is bound by latency (dependent LDS weights, the row reads, one global read-modify-write per term), so
// it wants many resident waves more than it minds repeated extends: 20,000 x 32 runs in 381 ms at S = 8 against
// 817 ms at S = 1, 500 x 256 in 37 ms at S = 256 against 963 ms at S = 1 (profiles/gbdt_shap_interactions.txt).
//
// LDS: SI_T = 128 threads, so that a few hundred rows already make several workgroups. Two weight columns,
// [k][thread] as in gbdt_shap.hip (conflict-free), sized by the forest's longest path: max_m + 1 doubles of w and
// max_m of w2 per thread, 13 KB at depth 6 and 33 KB at the limit of 16. With the 16 KB table chunk a workgroup
// needs 29 KB (5 per CU, 10 waves) at depth 6 and 49 KB (3 per CU) at the limit. Rows are read from global
// memory at every F: a leaf reads 2 m floats of its row beside O(m^3) LDS arithmetic, and staged rows would
// take the LDS of a resident workgroup.
//
// Table chunks: built as for gbdt_shap.hip (gbdt_shap_host.h), with a budget of 16 KB (a depth-6 tree is at most
// 13 KB): whole trees pass through LDS; a tree whose tables alone exceed the budget is read from global memory.
//
// Output: inter_diag_kernel finishes the diagonal in place (one thread per (row, class, i), the header's
// shap_interaction_diagonal); inter_transpose_kernel writes [row][class][F + 1][F + 1] through LDS tiles with the
// bias corner and the zero last row and column.
//
// SH_MAXM = 16 unique features on a path is the kernel's limit; beyond it the entry point returns -3.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <vector>

#include "../gbdt/shap_interactions.h"
#include "gbdt_shap_host.h"

namespace {

using gbdt::ShapElem;
using gbdt::ShapLeaf;
using shap_host::Buffers;
using shap_host::SChunk;

#define SI_T 128
#define SI_TABLE_BYTES (16 * 1024)  // table chunk
#define SI_FILL 1024                // workgroups the split aims at: 4 per CU
#define SI_MAXSPLIT 256
#define SI_BUFFER_BYTES ((size_t)256 << 20)
#define SI_MAXCHUNK (1 << 20)       // rows: the transpose puts 32-row tiles on grid z

struct WeightColumn {               // w[k] of this thread: LDS [k][thread]
  double* p; int stride;
  __device__ __forceinline__ double& operator[](int k) const { return p[k * stride]; }
};

// acc: this thread's (class, row) corner of [K][F][F][stride]; it owns first indices f with (f & smask) == s
template <class LeafPtr, class ElemPtr>
__device__ __forceinline__ void run_leaves(LeafPtr lb, ElemPtr eb, int nleaf, int elem0, const float* row,
                                           const double* __restrict__ inv, WeightColumn w, WeightColumn w2,
                                           int smask, int s, double* acc, size_t F, size_t stride) {
  for (int l = 0; l < nleaf; ++l) {
    const ShapLeaf lf = lb[l];
    gbdt::shap_leaf_interactions(
        eb + (lf.e0 - elem0), lf.m, lf.value, row, inv, w, w2, [smask, s](int f) { return (f & smask) == s; },
        [acc, F, stride](int f, double term) { acc[((size_t)f * F + f) * stride] += term; },
        [acc, F, stride](int a, int b, double term) { acc[((size_t)a * F + b) * stride] += term; });
  }
}

// acc [K][F][F][stride] (zeroed), row i of the upload at [..][i]. grid (row blocks, K, S).
__global__ void __launch_bounds__(SI_T) inter_kernel(const float* __restrict__ X, int n, int F,
                                                     const ShapLeaf* __restrict__ leaves,
                                                     const ShapElem* __restrict__ elems,
                                                     const SChunk* __restrict__ chunks,
                                                     const int* __restrict__ cstart, const double* __restrict__ inv,
                                                     int max_m, double* __restrict__ acc, size_t stride) {
  extern __shared__ double si_sm[];
  double* tab = si_sm;
  const int c = blockIdx.y, s = blockIdx.z, smask = gridDim.z - 1, tid = threadIdx.x;
  double* wts = si_sm + SI_TABLE_BYTES / 8;
  const long i0 = (long)blockIdx.x * SI_T;
  const int rows = (int)min((long)SI_T, (long)n - i0);
  const bool active = tid < rows;
  const size_t i = (size_t)i0 + tid;
  const float* grow = X + i * F;
  const WeightColumn w{wts + tid, SI_T}, w2{wts + (max_m + 1) * SI_T + tid, SI_T};
  double* my = acc + (size_t)c * F * F * stride + i;
  for (int ci = cstart[c]; ci < cstart[c + 1]; ++ci) {
    const SChunk ch = chunks[ci];
    __syncthreads();                 // the previous chunk's leaves are done (first pass: nothing to wait for)
    if (ch.lds) {
      const uint64_t* se = reinterpret_cast<const uint64_t*>(elems + ch.elem0);      // records as 8-byte words
      const uint64_t* sl = reinterpret_cast<const uint64_t*>(leaves + ch.leaf0);
      uint64_t* dst = reinterpret_cast<uint64_t*>(tab);
      const int ne = ch.nelem * 4, nl = ch.nleaf * 2;
      for (int v = tid; v < ne; v += SI_T) dst[v] = se[v];
      for (int v = tid; v < nl; v += SI_T) dst[ne + v] = sl[v];
    }
    __syncthreads();                 // the chunk is staged
    if (!active) continue;
    if (ch.lds) {
      const ShapElem* eb = reinterpret_cast<const ShapElem*>(tab);
      const ShapLeaf* lb = reinterpret_cast<const ShapLeaf*>(tab + ch.nelem * 4);
      run_leaves(lb, eb, ch.nleaf, ch.elem0, grow, inv, w, w2, smask, s, my, (size_t)F, stride);
    } else {
      run_leaves(leaves + ch.leaf0, elems + ch.elem0, ch.nleaf, ch.elem0, grow, inv, w, w2, smask, s, my,
                 (size_t)F, stride);
    }
  }
}

// Phi[i][i] = phi_i - the rest of row i, in place. grid (row blocks, F, K), one thread per (row, class, i).
__global__ void __launch_bounds__(256) inter_diag_kernel(double* __restrict__ acc, size_t stride, int n, int F) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y, c = blockIdx.z;
  if (r >= n) return;
  double* row = acc + ((size_t)c * F + i) * F * stride + r;
  row[(size_t)i * stride] = gbdt::shap_interaction_diagonal(F, i, [row, stride](int j) { return row[(size_t)j * stride]; });
}

// acc [K][F][F][stride] -> out [n][K][F + 1][F + 1]; [F][F] = bias[class], the rest of row and column F zero.
// grid (K (F + 1): class and i, j tiles, row tiles), 32 x 8.
__global__ void __launch_bounds__(256) inter_transpose_kernel(const double* __restrict__ acc, size_t stride, int n,
                                                              int F, int K, const double* __restrict__ bias,
                                                              double* __restrict__ out) {
  __shared__ double tile[32][33];
  const int F1 = F + 1, c = blockIdx.x / F1, i = blockIdx.x - c * F1, tx = threadIdx.x, ty = threadIdx.y;
  const int j0 = blockIdx.y * 32;
  const long r0 = (long)blockIdx.z * 32;
  for (int q = ty; q < 32; q += 8) {
    const int j = j0 + q;
    const long r = r0 + tx;
    double v = 0.0;
    if (i < F && j < F) {
      if (r < n) v = acc[(((size_t)c * F + i) * F + j) * stride + r];
    } else if (i == F && j == F) {
      v = bias[c];
    }
    tile[q][tx] = v;
  }
  __syncthreads();
  for (int q = ty; q < 32; q += 8) {
    const long r = r0 + q;
    const int j = j0 + tx;
    if (r < n && j <= F) out[(((size_t)r * K + c) * F1 + i) * F1 + j] = tile[tx][q];
  }
}

struct Plan { int chunk, split; };

// 0, or -4 when one row's output exceeds the per-buffer bound
int make_plan(int n, int F, int K, int chunk_rows, int split, Plan& p) {
  const size_t out_row = sizeof(double) * (size_t)K * ((size_t)F + 1) * ((size_t)F + 1);
  if (out_row > SI_BUFFER_BYTES) return -4;
  p.chunk = (int)std::min<size_t>(std::min(std::min(chunk_rows, n), SI_MAXCHUNK), SI_BUFFER_BYTES / out_row);
  if (split <= 0) {
    const long blocks = (long)((p.chunk + SI_T - 1) / SI_T) * K;
    split = 1;
    while (blocks * split < SI_FILL) split *= 2;
  }
  p.split = 1;
  while (p.split * 2 <= std::min(std::min(split, SI_MAXSPLIT), F)) p.split *= 2;
  return 0;
}

}  // namespace

extern "C" {

// The most unique features on one root-to-leaf path the kernel handles.
int gbdt_shap_inter_hip_limit() { return SH_MAXM; }

// What a call with these sizes does -- for tests and tools: plan[0] the rows per device chunk, plan[1] the
// feature-axis split S. Returns 0, -1 bad arguments, -4 one row's output exceeds 256 MB.
int gbdt_shap_inter_hip_plan(int n, int F, int K, int chunk_rows, int* plan) {
  if (n <= 0 || F <= 0 || K <= 0 || K > 65535 || chunk_rows <= 0 || plan == nullptr) return -1;
  Plan p;
  if (const int rc = make_plan(n, F, K, chunk_rows, 0, p)) return rc;
  plan[0] = p.chunk;
  plan[1] = p.split;
  return 0;
}

// SHAP interaction values of n raw rows X_h [n][F] (host) with the first ntrees trees (a multiple of K) of a
// compact forest with node covers: out [n][K][F + 1][F + 1] fp64. split: the feature-axis split S, rounded down
// to a power of two within [1, min(256, F)]; 0 chooses it (the header's rule). out_ms (may be null): [0] kernel
// milliseconds, [1] milliseconds including the table build, uploads and read-backs. Returns 0, -1 bad
// arguments, -2 malformed forest, -3 a path with more than gbdt_shap_inter_hip_limit() unique features,
// -4 one row's output exceeds 256 MB, -100 - hipError.
int gbdt_shap_inter_hip_split(const float* X_h, int n, int F, const long long* offsets, const int* feature,
                              const float* threshold, const int* left, const double* value, const double* cover,
                              int ntrees, int K, double base, int chunk_rows, int split, double* out,
                              double* out_ms) {
  if (n < 0 || F <= 0 || K <= 0 || K > 65535 || ntrees < 0 || ntrees % K || chunk_rows <= 0 || split < 0 ||
      cover == nullptr || out == nullptr)
    return -1;
  if (n == 0) return 0;
  const auto t_start = std::chrono::steady_clock::now();
  Plan plan;
  if (const int rc = make_plan(n, F, K, chunk_rows, split, plan)) return rc;
  gbdt::ShapTables tb;
  if (const int rc = gbdt::shap_build(F, offsets, feature, threshold, left, value, cover, ntrees, K, base, tb)) return rc;
  if (tb.max_m > SH_MAXM) return -3;
  std::vector<SChunk> chunks;
  std::vector<int> cstart;
  shap_host::shap_chunks(tb, ntrees, K, SI_TABLE_BYTES, chunks, cstart);

  // the weight columns of the forest's longest path: max_m + 1 of w, max_m of w2
  const size_t lds = (size_t)SI_TABLE_BYTES + (size_t)(2 * tb.max_m + 1) * 8 * SI_T;
  static_assert(3 * (SI_TABLE_BYTES + (2 * SH_MAXM + 1) * 8 * SI_T) <= SH_LDS_TOTAL, "three workgroups per CU at least");
  SHC(hipFuncSetAttribute((const void*)inter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int chunk = plan.chunk;
  const size_t out_row = sizeof(double) * (size_t)K * ((size_t)F + 1) * ((size_t)F + 1);
  const size_t acc_row = sizeof(double) * (size_t)K * F * F, padded = ((size_t)chunk + 7) / 8 * 8;
  const size_t stride = chunk >= 64 && acc_row * padded <= SI_BUFFER_BYTES ? padded : (size_t)chunk;
  const size_t acc_bytes = acc_row * stride;

  Buffers b;
  ShapLeaf* d_leaves; ShapElem* d_elems; SChunk* d_chunks; int* d_cstart; double *d_inv, *d_bias, *d_acc, *d_out;
  float* d_X;
  SHC(b.alloc(d_leaves, sizeof(ShapLeaf) * tb.leaves.size()));
  SHC(b.alloc(d_elems, sizeof(ShapElem) * tb.elems.size()));
  SHC(b.alloc(d_chunks, sizeof(SChunk) * chunks.size()));
  SHC(b.alloc(d_cstart, sizeof(int) * cstart.size()));
  SHC(b.alloc(d_inv, sizeof(double) * tb.inv.size()));
  SHC(b.alloc(d_bias, sizeof(double) * K));
  SHC(b.alloc(d_X, sizeof(float) * (size_t)chunk * F));
  SHC(b.alloc(d_acc, acc_bytes));
  SHC(b.alloc(d_out, out_row * chunk));
  SHC(hipEventCreate(&b.ev[0]));
  SHC(hipEventCreate(&b.ev[1]));
  if (!tb.leaves.empty()) SHC(hipMemcpy(d_leaves, tb.leaves.data(), sizeof(ShapLeaf) * tb.leaves.size(), hipMemcpyHostToDevice));
  if (!tb.elems.empty()) SHC(hipMemcpy(d_elems, tb.elems.data(), sizeof(ShapElem) * tb.elems.size(), hipMemcpyHostToDevice));
  if (!chunks.empty()) SHC(hipMemcpy(d_chunks, chunks.data(), sizeof(SChunk) * chunks.size(), hipMemcpyHostToDevice));
  SHC(hipMemcpy(d_cstart, cstart.data(), sizeof(int) * cstart.size(), hipMemcpyHostToDevice));
  SHC(hipMemcpy(d_inv, tb.inv.data(), sizeof(double) * tb.inv.size(), hipMemcpyHostToDevice));
  SHC(hipMemcpy(d_bias, tb.bias.data(), sizeof(double) * K, hipMemcpyHostToDevice));
  double kernel_ms = 0.0;
  for (long r0 = 0; r0 < n; r0 += chunk) {
    const int m = (int)std::min<long>(chunk, n - r0);
    SHC(hipMemcpy(d_X, X_h + (size_t)r0 * F, sizeof(float) * (size_t)m * F, hipMemcpyHostToDevice));
    SHC(hipEventRecord(b.ev[0], 0));
    SHC(hipMemsetAsync(d_acc, 0, acc_bytes, 0));
    hipLaunchKernelGGL(inter_kernel, dim3((m + SI_T - 1) / SI_T, K, plan.split), dim3(SI_T), lds, 0, d_X, m, F,
                       d_leaves, d_elems, d_chunks, d_cstart, d_inv, tb.max_m, d_acc, stride);
    SHC(hipGetLastError());
    hipLaunchKernelGGL(inter_diag_kernel, dim3((m + 255) / 256, F, K), dim3(256), 0, 0, d_acc, stride, m, F);
    SHC(hipGetLastError());
    hipLaunchKernelGGL(inter_transpose_kernel, dim3(K * (F + 1), (F + 1 + 31) / 32, (m + 31) / 32), dim3(32, 8), 0, 0,
                       d_acc, stride, m, F, K, d_bias, d_out);
    SHC(hipGetLastError());
    SHC(hipEventRecord(b.ev[1], 0));
    SHC(hipMemcpy(out + (size_t)r0 * (out_row / sizeof(double)), d_out, out_row * m, hipMemcpyDeviceToHost));
    float ms = 0.f;
    SHC(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
    kernel_ms += ms;
  }
  if (out_ms) {
    out_ms[0] = kernel_ms;
    out_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  }
  return 0;
}

int gbdt_shap_inter_hip(const float* X_h, int n, int F, const long long* offsets, const int* feature,
                        const float* threshold, const int* left, const double* value, const double* cover, int ntrees,
                        int K, double base, int chunk_rows, double* out, double* out_ms) {
  return gbdt_shap_inter_hip_split(X_h, n, F, offsets, feature, threshold, left, value, cover, ntrees, K, base,
                                   chunk_rows, 0, out, out_ms);
}

}  // extern "C"
