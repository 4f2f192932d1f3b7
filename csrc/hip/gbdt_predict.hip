// GBDT forest prediction on MI355X for a fitted Booster (gentun_amd/models/booster.py): raw float rows, float
// thresholds, fp64 margins that are bit-identical to the CPU predictor (csrc/gbdt/engine.cpp gbdt_predict).
//
// Rule (the Booster's): a row goes left when !(x[feature] > threshold); the margin of (row, class) is the base
// margin plus the leaf values of the class's trees, added one tree at a time in round order in fp64.
//
// Kernel contract: grid = (row blocks, K). A thread owns ONE (row, class) and adds that class's trees in round
// order into one fp64 register, which is what makes the sum equal to the CPU's to the bit: a row's trees are never
// split over threads and there are no atomics.
//
// The host lays the forest out class-major (class c's trees of rounds 0, 1, ... are consecutive), so a block
// stages only its own class's trees. They pass through LDS in consecutive chunks of at most PF_NODES nodes
// (12-byte node records (feature, threshold, left) + 8-byte values); a tree that alone exceeds the budget
// (depth 12: up to 8191 nodes) is walked from global memory. The block's rows are staged in LDS as floats with
// the odd dword stride F + 1: the lanes of a wave look up the same feature of consecutive rows when they sit in
// the same tree node, and ds_read_b32 banks are (address / 4) % 32, so an odd stride spreads those lookups over
// distinct banks (gbdt_hist.hip's predict_kernel does the same with Fs / 4 + 1 for its byte rows). A block holds
// as many rows (a multiple of 64, at most 256, one per thread) as the 160 KB of a gfx950 CU leave beside the tree
// chunk; when not even 64 fit (F above ~540) the rows are read from global memory instead.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <vector>

namespace {

#define PF_LDS_TOTAL (160 * 1024)   // gfx950: LDS per CU = the most one workgroup can ask for
#define PF_NODES 1228               // tree chunk: 1228 x (12 + 8) B = 24,560 B
#define PF_T 256

struct PNode { int f; float t; int l; };              // f < 0: leaf; right child = l + 1 (tree-local)
struct PChunk { int first, count, node0, lds; };      // trees [first, first + count) of the class-major list

// leaf of one row in the tree whose nodes start at nd[0]
template <class RowPtr, class NodePtr>
__device__ __forceinline__ int walk_tree(RowPtr row, NodePtr nd) {
  int j = 0;
  PNode k = nd[0];
  while (k.f >= 0) {
    j = !(row[k.f] > k.t) ? k.l : k.l + 1;
    k = nd[j];
  }
  return j;
}

// LEAF: write tree-local leaf indices [n][T] instead of margins [n][K]. LROWS: the block's rows are staged in LDS.
template <bool LEAF, bool LROWS>
__global__ void __launch_bounds__(PF_T) predict_forest_kernel(const float* __restrict__ X, int n, int F,
                                                              const PNode* __restrict__ nodes,
                                                              const double* __restrict__ value,
                                                              const int* __restrict__ toff,
                                                              const PChunk* __restrict__ chunks,
                                                              const int* __restrict__ cstart, int K, int rounds,
                                                              double base, double* __restrict__ out_margin,
                                                              int* __restrict__ out_leaf) {
  extern __shared__ double pf_sm[];
  double* lval = pf_sm;
  PNode* lnode = reinterpret_cast<PNode*>(lval + PF_NODES);
  float* lrow = reinterpret_cast<float*>(lnode + PF_NODES);
  const int c = blockIdx.y, tid = threadIdx.x, R = blockDim.x, rs = F + 1;
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
  double acc = base;
  for (int ci = cstart[c]; ci < cstart[c + 1]; ++ci) {
    const PChunk ch = chunks[ci];
    __syncthreads();                 // the previous chunk's walks are done (first pass: nothing to wait for)
    if (ch.lds) {
      const int nn = toff[ch.first + ch.count] - ch.node0;
      for (int v = tid; v < nn; v += R) {
        lnode[v] = nodes[ch.node0 + v];
        lval[v] = value[ch.node0 + v];
      }
    }
    __syncthreads();                 // the chunk (and, first pass, the rows) are staged
    if (!active) continue;
    for (int u = ch.first; u < ch.first + ch.count; ++u) {
      const int o = toff[u];
      int j;
      if (ch.lds) j = LROWS ? walk_tree(srow, lnode + (o - ch.node0)) : walk_tree(grow, lnode + (o - ch.node0));
      else j = LROWS ? walk_tree(srow, nodes + o) : walk_tree(grow, nodes + o);
      if (LEAF) out_leaf[i * ((size_t)rounds * K) + (size_t)(u - c * rounds) * K + c] = j;
      else acc += ch.lds ? lval[o - ch.node0 + j] : value[o + j];
    }
  }
  if (!LEAF && active) out_margin[i * K + c] = acc;
}

struct Buffers {
  std::vector<void*> dev;
  hipEvent_t ev[2] = {nullptr, nullptr};
  template <class T> hipError_t alloc(T*& p, size_t bytes) {
    const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 4));
    if (e == hipSuccess) dev.push_back(p);
    return e;
  }
  Buffers() = default; Buffers(const Buffers&) = delete;
  ~Buffers() {
    for (void* p : dev) (void)hipFree(p);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};

#define PHC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -100 - (int)e_; } while (0)

}  // namespace

extern "C" {

// Rows the kernel stages per block for F features (0: rows are read from global memory) -- for tests and tools.
int gbdt_predict_hip_rows(int F) {
  const long fit = ((long)PF_LDS_TOTAL - (long)PF_NODES * 20) / (4l * ((long)F + 1));
  return fit < 64 ? 0 : (int)std::min<long>(PF_T, fit / 64 * 64);
}

// Predict n raw rows X_h [n][F] (host) with the first ntrees trees (a multiple of K) of a compact forest (tree t:
// round t / K, class t % K). Rows go to the device in chunks of at most chunk_rows. Exactly one of out_margin
// (fp64 [n][K]) and out_leaf (int32 [n][ntrees]) is given. out_ms (may be null): [0] kernel milliseconds,
// [1] milliseconds including uploads and read-backs. Returns 0, -1 bad arguments, -2 malformed forest,
// -100 - hipError.
int gbdt_predict_hip(const float* X_h, int n, int F, const long long* offsets, const int* feature,
                     const float* threshold, const int* left, const double* value, int ntrees, int K, double base,
                     int chunk_rows, double* out_margin, int* out_leaf, double* out_ms) {
  if (n < 0 || F <= 0 || K <= 0 || ntrees < 0 || ntrees % K || chunk_rows <= 0 || (out_margin == nullptr) == (out_leaf == nullptr))
    return -1;
  if (n == 0) return 0;
  const int rounds = ntrees / K;
  if (offsets[ntrees] >= (1ll << 31)) return -2;
  // class-major forest + chunk lists; the walk must stay inside each tree whatever the file held
  std::vector<PNode> nodes;
  std::vector<double> vals;
  std::vector<int> toff(ntrees + 1, 0), cstart(K + 1, 0);
  std::vector<PChunk> chunks;
  nodes.reserve((size_t)offsets[ntrees]);
  vals.reserve((size_t)offsets[ntrees]);
  for (int c = 0; c < K; ++c) {
    cstart[c] = (int)chunks.size();
    PChunk cur{c * rounds, 0, (int)nodes.size(), 1};
    int cur_nodes = 0;
    for (int r = 0; r < rounds; ++r) {
      const int t = r * K + c, u = c * rounds + r;
      const long long o = offsets[t], sz = offsets[t + 1] - o;
      if (sz < 1) return -2;
      for (long long j = 0; j < sz; ++j) {
        if (feature[o + j] >= F) return -2;
        if (feature[o + j] >= 0 && (left[o + j] <= j || (long long)left[o + j] + 1 >= sz)) return -2;
        nodes.push_back(PNode{feature[o + j], threshold[o + j], left[o + j]});
        vals.push_back(value[o + j]);
      }
      toff[u] = (int)nodes.size() - (int)sz;
      const bool big = sz > PF_NODES;
      if (cur.count > 0 && (big || cur_nodes + sz > PF_NODES)) {
        chunks.push_back(cur);
        cur = PChunk{u, 0, toff[u], 1};
        cur_nodes = 0;
      }
      cur.count += 1; cur_nodes += (int)sz;
      if (big) {                       // alone in its chunk, walked from global memory
        cur.lds = 0;
        chunks.push_back(cur);
        cur = PChunk{u + 1, 0, (int)nodes.size(), 1};
        cur_nodes = 0;
      }
    }
    if (cur.count > 0) chunks.push_back(cur);
  }
  cstart[K] = (int)chunks.size();
  toff[ntrees] = (int)nodes.size();

  const bool leaf = out_leaf != nullptr;
  const int R = gbdt_predict_hip_rows(F);
  const int T = R > 0 ? R : PF_T;
  const size_t lds = (size_t)PF_NODES * 20 + (R > 0 ? (size_t)R * (F + 1) * 4 : 0);
  const void* kern = leaf ? (R > 0 ? (const void*)predict_forest_kernel<true, true> : (const void*)predict_forest_kernel<true, false>)
                          : (R > 0 ? (const void*)predict_forest_kernel<false, true> : (const void*)predict_forest_kernel<false, false>);
  if (lds > 65536) PHC(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const size_t out_row = leaf ? sizeof(int) * (size_t)ntrees : sizeof(double) * (size_t)K;
  // device buffers of at most 256 MB each
  const size_t per_row = std::max(sizeof(float) * (size_t)F, std::max<size_t>(out_row, 1));
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min(chunk_rows, n), ((size_t)256 << 20) / per_row));

  Buffers b;
  PNode* d_nodes; double *d_val, *d_margin = nullptr; int *d_toff, *d_cstart, *d_leaf = nullptr; PChunk* d_chunks;
  float* d_X;
  PHC(b.alloc(d_nodes, sizeof(PNode) * nodes.size()));
  PHC(b.alloc(d_val, sizeof(double) * vals.size()));
  PHC(b.alloc(d_toff, sizeof(int) * toff.size()));
  PHC(b.alloc(d_cstart, sizeof(int) * cstart.size()));
  PHC(b.alloc(d_chunks, sizeof(PChunk) * chunks.size()));
  PHC(b.alloc(d_X, sizeof(float) * (size_t)chunk * F));
  if (leaf) PHC(b.alloc(d_leaf, out_row * chunk)); else PHC(b.alloc(d_margin, out_row * chunk));
  PHC(hipEventCreate(&b.ev[0]));
  PHC(hipEventCreate(&b.ev[1]));
  const auto t_start = std::chrono::steady_clock::now();
  if (!nodes.empty()) {
    PHC(hipMemcpy(d_nodes, nodes.data(), sizeof(PNode) * nodes.size(), hipMemcpyHostToDevice));
    PHC(hipMemcpy(d_val, vals.data(), sizeof(double) * vals.size(), hipMemcpyHostToDevice));
  }
  PHC(hipMemcpy(d_toff, toff.data(), sizeof(int) * toff.size(), hipMemcpyHostToDevice));
  PHC(hipMemcpy(d_cstart, cstart.data(), sizeof(int) * cstart.size(), hipMemcpyHostToDevice));
  if (!chunks.empty()) PHC(hipMemcpy(d_chunks, chunks.data(), sizeof(PChunk) * chunks.size(), hipMemcpyHostToDevice));
  double kernel_ms = 0.0;
  for (long r0 = 0; r0 < n; r0 += chunk) {
    const int m = (int)std::min<long>(chunk, n - r0);
    PHC(hipMemcpy(d_X, X_h + (size_t)r0 * F, sizeof(float) * (size_t)m * F, hipMemcpyHostToDevice));
    const dim3 grid((m + T - 1) / T, K);
    PHC(hipEventRecord(b.ev[0], 0));
    if (leaf) {
      if (R > 0) hipLaunchKernelGGL((predict_forest_kernel<true, true>), grid, dim3(T), lds, 0, d_X, m, F, d_nodes, d_val, d_toff, d_chunks, d_cstart, K, rounds, base, d_margin, d_leaf);
      else hipLaunchKernelGGL((predict_forest_kernel<true, false>), grid, dim3(T), lds, 0, d_X, m, F, d_nodes, d_val, d_toff, d_chunks, d_cstart, K, rounds, base, d_margin, d_leaf);
    } else {
      if (R > 0) hipLaunchKernelGGL((predict_forest_kernel<false, true>), grid, dim3(T), lds, 0, d_X, m, F, d_nodes, d_val, d_toff, d_chunks, d_cstart, K, rounds, base, d_margin, d_leaf);
      else hipLaunchKernelGGL((predict_forest_kernel<false, false>), grid, dim3(T), lds, 0, d_X, m, F, d_nodes, d_val, d_toff, d_chunks, d_cstart, K, rounds, base, d_margin, d_leaf);
    }
    PHC(hipGetLastError());
    PHC(hipEventRecord(b.ev[1], 0));
    if (leaf) PHC(hipMemcpy(out_leaf + (size_t)r0 * ntrees, d_leaf, out_row * m, hipMemcpyDeviceToHost));
    else PHC(hipMemcpy(out_margin + (size_t)r0 * K, d_margin, out_row * m, hipMemcpyDeviceToHost));
    float ms = 0.f;
    PHC(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
    kernel_ms += ms;
  }
  if (out_ms) {
    out_ms[0] = kernel_ms;
    out_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  }
  return 0;
}

}  // extern "C"
