// SHAP contributions (Booster.predict(pred_contribs=True)) on MI355X, bit-identical to the CPU predictor
// (csrc/gbdt/engine.cpp gbdt_predict_contribs). The definition, the host-built per-leaf element tables and the
// per-leaf arithmetic are csrc/gbdt/shap_tables.h, shared with the CPU library; that header switches fp
// contraction off (#pragma clang fp contract(off)) for this whole translation unit, so the device code has no
// fused multiply-add where the CPU build (no FMA) has a multiply and an add. shap_leaf divides nowhere.
//
// Kernel contract: grid = (row blocks, K). A thread owns ONE (row, class) and performs that pair's additions in
// the header's order (the class's trees in round order, leaves by compact node index, elements by first
// appearance). No atomics, no cross-thread reduction of a phi.
//
// Where the phi accumulators live: in global memory, in a scratch buffer laid out [class][feature][row], each
// read-modify-written by its owning thread only. All lanes of a wave work on the same leaf and element at the
// same time, hence on the same feature of 64 consecutive rows: with the row index innermost every such
// read-modify-write is one contiguous 512-byte access. A second kernel transposes the buffer through LDS tiles
// into the output layout [row][class][F + 1] and writes the bias column. (LDS accumulators would need
// 8 (F + 1) bytes per thread, 2 KB at F = 256, beside the staged rows; one layout serves every F.)
//
// Staging, as in gbdt_predict.hip: the host lays the tables out class-major; they pass through LDS in chunks of
// whole trees of at most SH_TABLE_BYTES (16-byte leaf records, 32-byte element records); a tree whose tables
// alone exceed the budget (depth 12) is read from global memory. The block's 256 rows are staged in LDS as
// floats with the odd dword stride F + 1 while the block then still needs no more than half of the CU's LDS,
// so that two blocks (8 waves) share a CU; otherwise (F above 13) they are read from global memory. Occupancy
// decides here, not the row reads: at F = 256 a block that stages its rows holds 64 of them, one wave per CU,
// and ran 4.3 times slower than 256-thread blocks reading rows from global memory (profiles/gbdt_shap.txt).
//
// Path weights: m + 1 doubles per thread, indexed at run time, so they live in LDS as [k][thread] (consecutive
// lanes read consecutive 8-byte words: conflict-free), not in a private array that would go to scratch.
// SH_MAXM = 16 unique features on a path is the kernel's limit (the GPU engine grows depth 12 at most); beyond
// it the entry point returns -3 and Python raises.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <vector>

#include "../gbdt/shap_tables.h"
#include "gbdt_shap_host.h"

namespace {

using gbdt::ShapElem;
using gbdt::ShapLeaf;
using shap_host::Buffers;
using shap_host::SChunk;

#define SH_T 256

struct WeightColumn {               // w[k] of this thread: LDS [k][thread]
  double* p; int stride;
  __device__ __forceinline__ double& operator[](int k) const { return p[k * stride]; }
};

template <class LeafPtr, class ElemPtr, class Row>
__device__ __forceinline__ void run_leaves(LeafPtr lb, ElemPtr eb, int nleaf, int elem0, Row row,
                                           const double* __restrict__ inv, WeightColumn w, double* acc,
                                           size_t stride) {
  for (int l = 0; l < nleaf; ++l) {
    const ShapLeaf lf = lb[l];
    gbdt::shap_leaf(eb + (lf.e0 - elem0), lf.m, lf.value, row, inv, w,
                    [acc, stride](int f, double term) { acc[(size_t)f * stride] += term; });
  }
}

// LROWS: the block's rows are staged in LDS. acc [K][F][stride] (zeroed), row i of the upload at [..][i].
template <bool LROWS>
__global__ void __launch_bounds__(SH_T) shap_kernel(const float* __restrict__ X, int n, int F,
                                                    const ShapLeaf* __restrict__ leaves,
                                                    const ShapElem* __restrict__ elems,
                                                    const SChunk* __restrict__ chunks,
                                                    const int* __restrict__ cstart, const double* __restrict__ inv,
                                                    double* __restrict__ acc, size_t stride) {
  extern __shared__ double sh_sm[];
  double* tab = sh_sm;
  const int c = blockIdx.y, tid = threadIdx.x, R = blockDim.x, rs = F + 1;
  double* wts = sh_sm + SH_TABLE_BYTES / 8;
  float* lrow = reinterpret_cast<float*>(wts + (SH_MAXM + 1) * R);
  const long i0 = (long)blockIdx.x * R;
  const int rows = (int)min((long)R, (long)n - i0);
  if (LROWS) {
    const float* src = X + (size_t)i0 * F;
    for (int v = tid; v < rows * F; v += R) {
      const int r = v / F;
      lrow[r * rs + (v - r * F)] = src[v];
    }
  }
  const bool active = tid < rows;
  const size_t i = (size_t)i0 + tid;
  const float* grow = X + i * F;
  const float* srow = lrow + tid * rs;
  const WeightColumn w{wts + tid, R};
  double* my = acc + (size_t)c * F * stride + i;
  for (int ci = cstart[c]; ci < cstart[c + 1]; ++ci) {
    const SChunk ch = chunks[ci];
    __syncthreads();                 // the previous chunk's leaves are done (first pass: nothing to wait for)
    if (ch.lds) {
      const uint64_t* se = reinterpret_cast<const uint64_t*>(elems + ch.elem0);      // records as 8-byte words
      const uint64_t* sl = reinterpret_cast<const uint64_t*>(leaves + ch.leaf0);
      uint64_t* dst = reinterpret_cast<uint64_t*>(tab);
      const int ne = ch.nelem * 4, nl = ch.nleaf * 2;
      for (int v = tid; v < ne; v += R) dst[v] = se[v];
      for (int v = tid; v < nl; v += R) dst[ne + v] = sl[v];
    }
    __syncthreads();                 // the chunk (and, first pass, the rows) are staged
    if (!active) continue;
    if (ch.lds) {
      const ShapElem* eb = reinterpret_cast<const ShapElem*>(tab);
      const ShapLeaf* lb = reinterpret_cast<const ShapLeaf*>(tab + ch.nelem * 4);
      if (LROWS) run_leaves(lb, eb, ch.nleaf, ch.elem0, srow, inv, w, my, stride);
      else run_leaves(lb, eb, ch.nleaf, ch.elem0, grow, inv, w, my, stride);
    } else {
      if (LROWS) run_leaves(leaves + ch.leaf0, elems + ch.elem0, ch.nleaf, ch.elem0, srow, inv, w, my, stride);
      else run_leaves(leaves + ch.leaf0, elems + ch.elem0, ch.nleaf, ch.elem0, grow, inv, w, my, stride);
    }
  }
}

// acc [K][F][stride] -> out [n][K][F + 1], column F = bias[class]. grid (row tiles, feature tiles, K), 32 x 8.
__global__ void __launch_bounds__(256) shap_transpose_kernel(const double* __restrict__ acc, size_t stride, int n,
                                                             int F, int K, const double* __restrict__ bias,
                                                             double* __restrict__ out) {
  __shared__ double tile[32][33];
  const int c = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y;
  const long i0 = (long)blockIdx.x * 32;
  const int f0 = blockIdx.y * 32;
  for (int q = ty; q < 32; q += 8) {
    const int f = f0 + q;
    const long i = i0 + tx;
    double v = 0.0;
    if (i < n && f < F) v = acc[((size_t)c * F + f) * stride + i];
    else if (f == F) v = bias[c];
    tile[q][tx] = v;
  }
  __syncthreads();
  for (int q = ty; q < 32; q += 8) {
    const long i = i0 + q;
    const int f = f0 + tx;
    if (i < n && f <= F) out[((size_t)i * K + c) * ((size_t)F + 1) + f] = tile[tx][q];
  }
}

}  // namespace

extern "C" {

// The most unique features on one root-to-leaf path the kernel handles.
int gbdt_shap_hip_limit() { return SH_MAXM; }

// Rows the kernel stages per block for F features (0: rows are read from global memory) -- for tests and tools.
int gbdt_shap_hip_rows(int F) {
  const long need = SH_TABLE_BYTES + SH_T * ((SH_MAXM + 1) * 8l + 4l * ((long)F + 1));
  return need <= SH_LDS_TOTAL / 2 ? SH_T : 0;
}

// SHAP contributions of n raw rows X_h [n][F] (host) with the first ntrees trees (a multiple of K) of a compact
// forest with node covers: out [n][K][F + 1] fp64, the bias in the last column. Rows go to the device in chunks
// of at most chunk_rows, bounded also by 256 MB per device buffer. out_ms (may be null): [0] kernel
// milliseconds, [1] milliseconds including the table build, uploads and read-backs. Returns 0, -1 bad
// arguments, -2 malformed forest, -3 a path with more than gbdt_shap_hip_limit() unique features,
// -100 - hipError.
int gbdt_shap_hip(const float* X_h, int n, int F, const long long* offsets, const int* feature,
                  const float* threshold, const int* left, const double* value, const double* cover, int ntrees,
                  int K, double base, int chunk_rows, double* out, double* out_ms) {
  if (n < 0 || F <= 0 || K <= 0 || ntrees < 0 || ntrees % K || chunk_rows <= 0 || cover == nullptr || out == nullptr)
    return -1;
  if (n == 0) return 0;
  const auto t_start = std::chrono::steady_clock::now();
  gbdt::ShapTables tb;
  if (const int rc = gbdt::shap_build(F, offsets, feature, threshold, left, value, cover, ntrees, K, base, tb)) return rc;
  if (tb.max_m > SH_MAXM) return -3;
  std::vector<SChunk> chunks;
  std::vector<int> cstart;
  shap_host::shap_chunks(tb, ntrees, K, SH_TABLE_BYTES, chunks, cstart);

  const int R = gbdt_shap_hip_rows(F), T = SH_T;
  const size_t lds = (size_t)SH_TABLE_BYTES + (size_t)(SH_MAXM + 1) * 8 * T + (R > 0 ? (size_t)R * (F + 1) * 4 : 0);
  const void* kern = R > 0 ? (const void*)shap_kernel<true> : (const void*)shap_kernel<false>;
  SHC(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // device buffers of at most 256 MB each: the output row is K (F + 1) doubles
  const size_t out_row = sizeof(double) * (size_t)K * ((size_t)F + 1);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min(chunk_rows, n), ((size_t)256 << 20) / out_row));
  const size_t stride = ((size_t)chunk + 63) / 64 * 64;

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
  SHC(b.alloc(d_acc, sizeof(double) * (size_t)K * F * stride));
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
    SHC(hipMemsetAsync(d_acc, 0, sizeof(double) * (size_t)K * F * stride, 0));
    const dim3 grid((m + T - 1) / T, K);
    if (R > 0) hipLaunchKernelGGL(shap_kernel<true>, grid, dim3(T), lds, 0, d_X, m, F, d_leaves, d_elems, d_chunks, d_cstart, d_inv, d_acc, stride);
    else hipLaunchKernelGGL(shap_kernel<false>, grid, dim3(T), lds, 0, d_X, m, F, d_leaves, d_elems, d_chunks, d_cstart, d_inv, d_acc, stride);
    SHC(hipGetLastError());
    hipLaunchKernelGGL(shap_transpose_kernel, dim3((m + 31) / 32, (F + 1 + 31) / 32, K), dim3(32, 8), 0, 0, d_acc, stride, m, F, K, d_bias, d_out);
    SHC(hipGetLastError());
    SHC(hipEventRecord(b.ev[1], 0));
    SHC(hipMemcpy(out + (size_t)r0 * K * ((size_t)F + 1), d_out, out_row * m, hipMemcpyDeviceToHost));
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

}  // extern "C"
