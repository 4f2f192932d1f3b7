// Host side that the two SHAP translation units share (gbdt_shap.hip: contributions; gbdt_shap_inter.hip:
// interaction values): the table chunks a block stages in LDS, and the owner of a call's device buffers.

#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../gbdt/shap_tables.h"

#define SH_LDS_TOTAL (160 * 1024)   // gfx950: LDS per CU
#define SH_TABLE_BYTES (32 * 1024)  // table chunk of gbdt_shap.hip
#define SH_MAXM 16                  // unique features on a path

static_assert(sizeof(gbdt::ShapElem) == 32 && sizeof(gbdt::ShapLeaf) == 16, "table records are staged as 8-byte words");

namespace shap_host {

struct SChunk { int leaf0, nleaf, elem0, nelem, lds; };   // leaves / elements of consecutive trees of one class

// The class-major tree list of tb cut into chunks of whole trees of at most budget bytes (lds = 1); a tree
// whose tables alone exceed the budget is alone in its chunk and read from global memory (lds = 0).
// cstart [K + 1]: the chunks of class c are [cstart[c], cstart[c + 1]).
inline void shap_chunks(const gbdt::ShapTables& tb, int ntrees, int K, size_t budget, std::vector<SChunk>& chunks,
                        std::vector<int>& cstart) {
  using gbdt::ShapElem;
  using gbdt::ShapLeaf;
  const int rounds = ntrees / K;
  // first element of every tree of the class-major list (a tree's leaves and elements are consecutive)
  std::vector<int> tree_e0(ntrees + 1, (int)tb.elems.size());
  for (int u = ntrees - 1; u >= 0; --u)
    tree_e0[u] = tb.leaf_off[u] < tb.leaf_off[u + 1] ? tb.leaves[tb.leaf_off[u]].e0 : tree_e0[u + 1];
  chunks.clear();
  cstart.assign(K + 1, 0);
  for (int c = 0; c < K; ++c) {
    cstart[c] = (int)chunks.size();
    SChunk cur{tb.leaf_off[c * rounds], 0, tree_e0[c * rounds], 0, 1};
    for (int u = c * rounds; u < (c + 1) * rounds; ++u) {
      const int nl = tb.leaf_off[u + 1] - tb.leaf_off[u], ne = tree_e0[u + 1] - tree_e0[u];
      const size_t bytes = (size_t)nl * sizeof(ShapLeaf) + (size_t)ne * sizeof(ShapElem);
      const bool big = bytes > budget;
      const size_t have = (size_t)cur.nleaf * sizeof(ShapLeaf) + (size_t)cur.nelem * sizeof(ShapElem);
      if (cur.nleaf > 0 && (big || have + bytes > budget)) {
        chunks.push_back(cur);
        cur = SChunk{tb.leaf_off[u], 0, tree_e0[u], 0, 1};
      }
      cur.nleaf += nl; cur.nelem += ne;
      if (big) {                       // alone in its chunk, read from global memory
        cur.lds = 0;
        chunks.push_back(cur);
        cur = SChunk{tb.leaf_off[u + 1], 0, tree_e0[u + 1], 0, 1};
      }
    }
    if (cur.nleaf > 0) chunks.push_back(cur);
  }
  cstart[K] = (int)chunks.size();
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

}  // namespace shap_host

#define SHC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return -100 - (int)e_; } while (0)
