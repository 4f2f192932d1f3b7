// Native histogram GBDT engine with xgboost-style k-fold cross-validation.
//
// Replaces the XGBoost 0.72 `DMatrix` + `xgb.cv` call of the reference
// (gentun/models/xgboost_models.py:28-37):
//   * G1 quantise: per feature <= 256 bins (exact unique values when they fit,
//     so small fixtures such as Iris / wine split exactly like exact-greedy);
//   * G2 grad/hess per objective (reg:linear|squarederror, reg:logistic,
//     binary:logistic|logitraw with scale_pos_weight, multi:softmax|softprob);
//   * G3 histograms with the subtraction trick (build the smaller child);
//   * G4 best split with lambda, alpha (L1 soft threshold), gamma,
//     min_child_weight, max_delta_step (xgboost's CalcGain/CalcWeight math);
//   * G5 partition, G6 leaf update (eta), G7 subsample / colsample_bytree /
//     colsample_bylevel, G8 metrics (rmse, mae, logloss, error, auc, merror,
//     mlogloss) per fold, mean/std over folds, early stopping on the mean
//     test value of the last metric; history truncated to the best round.
//
// Folds advance in lock-step (one boosting round of every fold, then the
// early-stopping check), each fold on its own thread. Deterministic: all
// sampling comes from a splitmix64 stream keyed by (seed, fold, round, class).
// What the MI355X engine (csrc/hip/gbdt_hist.hip) shares with this one: cv_protocol.h.
//
// gbdt_train fits the final model with the same tree-growing step (one fold, no test rows) and hands out its
// trees with float thresholds and their node statistics (cover, gain: gbdt_forest_stats); gbdt_predict scores
// raw rows with them, gbdt_predict_contribs explains them (shap_tables.h, shared with csrc/hip/gbdt_shap.hip;
// gentun_amd/models/booster.py), gbdt_predict_interactions by pairs of features (shap_interactions.h, shared
// with csrc/hip/gbdt_shap_inter.hip).

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <thread>
#include <vector>

#include "cv_protocol.h"
#include "shap_tables.h"
#include "shap_interactions.h"

namespace {

using namespace gbdt;

constexpr int kMaxBin = 256;

struct Quantized {
  int n = 0, F = 0;
  std::vector<uint8_t> bins;            // row-major [n][F]
  std::vector<int> nbins;               // per feature
  std::vector<std::vector<float>> upper;   // per feature: bin b holds values <= upper[b] (gbdt_train's thresholds)
};

// One feature column -> bins (exact: <= kMaxBin distinct values keep one bin
// each, otherwise kMaxBin equal-count quantile cuts). Writes bin b of row i
// at out[i * stride] (out may be null: cuts only) and hands out the bins' upper bounds.
static int quantize_column(const float* X, int n, int F, int f, uint8_t* out, size_t stride,
                           std::vector<float>& col, std::vector<float>& sorted, std::vector<float>& upper) {
  for (int i = 0; i < n; ++i) {
    float v = X[(size_t)i * F + f];
    col[i] = std::isnan(v) ? -std::numeric_limits<float>::infinity() : v;
  }
  sorted = col;
  std::sort(sorted.begin(), sorted.end());
  std::vector<float> uniq;
  uniq.reserve(256);
  for (int i = 0; i < n; ++i)
    if (uniq.empty() || sorted[i] != uniq.back()) {
      uniq.push_back(sorted[i]);
      if ((int)uniq.size() > kMaxBin) break;
    }
  upper.clear();                      // bin b holds values <= upper[b]
  if ((int)uniq.size() <= kMaxBin) {
    upper = uniq;
  } else {
    // quantile cuts: kMaxBin bins of ~equal counts
    upper.reserve(kMaxBin);
    for (int b = 1; b <= kMaxBin; ++b) {
      size_t idx = std::min<size_t>((size_t)n - 1, (size_t)((double)b * n / kMaxBin) - (b == kMaxBin ? 1 : 0));
      float v = sorted[idx];
      if (upper.empty() || v > upper.back()) upper.push_back(v);
    }
    upper.back() = sorted[n - 1];
  }
  for (int i = 0; out != nullptr && i < n; ++i) {
    int b = (int)(std::lower_bound(upper.begin(), upper.end(), col[i]) - upper.begin());
    if (b >= (int)upper.size()) b = (int)upper.size() - 1;
    out[(size_t)i * stride] = (uint8_t)b;
  }
  return (int)upper.size();
}

// Columns are independent: one thread per stripe of features (the per-column
// sort dominates: ~n log n per feature). feature_major: bins[f][n] (the GPU
// histogram layout) instead of bins[n][F].
// uppers (optional): F vectors that receive every feature's upper bounds; bins may be null with it (cuts only).
static void quantize_into(const float* X, int n, int F, uint8_t* bins, int* nbins, bool feature_major,
                          std::vector<float>* uppers = nullptr) {
  int nt = (int)std::max(1u, std::thread::hardware_concurrency());
  nt = std::min(nt, std::max(1, F));
  auto work = [&](int t) {
    std::vector<float> col(n), sorted, upper;
    for (int f = t; f < F; f += nt) {
      uint8_t* out = bins == nullptr ? nullptr : (feature_major ? bins + (size_t)f * n : bins + f);
      nbins[f] = quantize_column(X, n, F, f, out, feature_major ? 1 : (size_t)F, col, sorted, upper);
      if (uppers) uppers[f] = upper;
    }
  };
  if (nt == 1 || (size_t)n * F < (1u << 16)) {
    nt = 1;
    work(0);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
  for (auto& x : th) x.join();
}

Quantized quantize(const float* X, int n, int F) {
  Quantized q;
  q.n = n; q.F = F;
  q.bins.resize((size_t)n * F);
  q.nbins.resize(F);
  q.upper.resize(F);
  quantize_into(X, n, F, q.bins.data(), q.nbins.data(), false, q.upper.data());
  return q;
}

struct Node {
  int feature = -1, split_bin = -1, left = -1, right = -1;
  double value = 0.0;
  double cover = 0.0, gain = 0.0;   // hessian sum of the node's (sampled) rows; loss change of its split, 0 for leaves
};

struct GH { double g, h; };

struct Tree {
  std::vector<Node> nodes;
  double predict(const uint8_t* row) const {
    int k = 0;
    while (nodes[k].left >= 0) k = (row[nodes[k].feature] <= nodes[k].split_bin) ? nodes[k].left : nodes[k].right;
    return nodes[k].value;
  }
};

struct SplitResult {
  double gain = 0.0; int feature = -1, bin = -1; double GL = 0, HL = 0;
};

// Build one tree on rows `rows` (indices into the dataset) with grad/hess `gh`
// and the tree's draws `draws` (cv_protocol.h draw_tree).
Tree build_tree(const Quantized& q, const std::vector<GH>& gh, std::vector<int>& rows, const Params& p,
                const TreeDraws& draws) {
  const int F = q.F;
  const int max_depth = std::max(0, (int)p.max_depth);
  Tree tree;
  const std::vector<int>& feats = draws.feats;
  struct Work { int node; int begin, end; std::vector<GH> hist; double G, H; };
  auto build_hist = [&](int b, int e, std::vector<GH>& hist) {
    hist.assign((size_t)F * kMaxBin, GH{0.0, 0.0});
    for (int r = b; r < e; ++r) {
      const int i = rows[r];
      const uint8_t* row = &q.bins[(size_t)i * F];
      const GH v = gh[i];
      for (int f : feats) { GH& c = hist[(size_t)f * kMaxBin + row[f]]; c.g += v.g; c.h += v.h; }
    }
  };
  std::vector<Work> level;
  {
    Work root;
    root.node = 0; root.begin = 0; root.end = (int)rows.size();
    tree.nodes.emplace_back();
    build_hist(root.begin, root.end, root.hist);
    double G = 0, H = 0;
    for (int r = root.begin; r < root.end; ++r) { G += gh[rows[r]].g; H += gh[rows[r]].h; }
    root.G = G; root.H = H;
    level.push_back(std::move(root));
  }
  for (int depth = 0; depth <= max_depth && !level.empty(); ++depth) {
    std::vector<Work> next;
    const std::vector<int> lfeats = level_features(feats, draws.level_key, depth, p);   // colsample_bylevel
    for (Work& w : level) {
      Node& nd = tree.nodes[w.node];
      nd.value = calc_weight(p, w.G, w.H) * p.eta;
      nd.cover = w.H;
      if (depth == max_depth || w.end - w.begin < 2) continue;
      const double parent_gain = calc_gain(p, w.G, w.H);
      SplitResult best;
      for (int f : lfeats) {
        const GH* hf = &w.hist[(size_t)f * kMaxBin];
        double GL = 0, HL = 0;
        for (int b = 0; b + 1 < q.nbins[f]; ++b) {
          GL += hf[b].g; HL += hf[b].h;
          const double GR = w.G - GL, HR = w.H - HL;
          if (HL < p.min_child_weight || HR < p.min_child_weight || HL <= 0.0 || HR <= 0.0) continue;
          const double chg = calc_gain(p, GL, HL) + calc_gain(p, GR, HR) - parent_gain;
          if (chg > best.gain + 1e-12 || (best.feature < 0 && chg > 1e-12)) {
            best.gain = chg; best.feature = f; best.bin = b; best.GL = GL; best.HL = HL;
          }
        }
      }
      if (best.feature < 0 || best.gain < p.gamma || best.gain <= 1e-12) continue;
      // partition rows[w.begin, w.end) stably: left (bin <= split) first
      const int f = best.feature, sb = best.bin;
      auto mid_it = std::stable_partition(rows.begin() + w.begin, rows.begin() + w.end,
                                          [&](int i) { return q.bins[(size_t)i * F + f] <= sb; });
      const int mid = (int)(mid_it - rows.begin());
      const int li = (int)tree.nodes.size();
      tree.nodes.emplace_back();
      tree.nodes.emplace_back();
      Node& pn = tree.nodes[w.node];
      pn.feature = f; pn.split_bin = sb; pn.left = li; pn.right = li + 1;
      pn.gain = best.gain;
      Work L, R;
      L.node = li; L.begin = w.begin; L.end = mid; L.G = best.GL; L.H = best.HL;
      R.node = li + 1; R.begin = mid; R.end = w.end; R.G = w.G - best.GL; R.H = w.H - best.HL;
      if (depth + 1 < max_depth) {
        // subtraction trick: build the smaller child, derive the larger
        Work& small = (L.end - L.begin <= R.end - R.begin) ? L : R;
        Work& large = (&small == &L) ? R : L;
        build_hist(small.begin, small.end, small.hist);
        large.hist = std::move(w.hist);
        for (size_t k = 0; k < large.hist.size(); ++k) {
          large.hist[k].g -= small.hist[k].g; large.hist[k].h -= small.hist[k].h;
        }
      }
      next.push_back(std::move(L));
      next.push_back(std::move(R));
    }
    level = std::move(next);
  }
  return tree;
}

inline double sigmoid(double x) { return 1.0 / (1.0 + std::exp(-x)); }

struct FoldState {
  std::vector<int> train, test;
  std::vector<double> margin;   // [n * K]
};

double auc_score(const std::vector<double>& s, const std::vector<double>& y) {
  const size_t n = s.size();
  std::vector<size_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return s[a] < s[b]; });
  double npos = 0, nneg = 0, rank_sum = 0;
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j + 1 < n && s[idx[j + 1]] == s[idx[i]]) ++j;
    const double avg_rank = 0.5 * (i + j) + 1.0;
    for (size_t k = i; k <= j; ++k) if (y[idx[k]] > 0.5) { rank_sum += avg_rank; npos += 1; } else nneg += 1;
    i = j + 1;
  }
  return auc_from_rank_sum(rank_sum, npos, nneg);
}

double eval_metric(int metric, int obj, int K, const std::vector<int>& rows, const std::vector<double>& margin,
                   const float* y) {
  const double n = (double)std::max<size_t>(1, rows.size());
  const double eps = 1e-15;
  switch (metric) {
    case M_RMSE: case M_MAE: {
      double acc = 0;
      for (int i : rows) {
        double pred = margin[(size_t)i * K];
        if (obj == OBJ_LOGISTIC || obj == OBJ_BINARY_LOGISTIC) pred = sigmoid(pred);
        const double d = pred - y[i];
        acc += metric == M_RMSE ? d * d : std::fabs(d);
      }
      return metric == M_RMSE ? std::sqrt(acc / n) : acc / n;
    }
    case M_LOGLOSS: {
      double acc = 0;
      for (int i : rows) {
        double pr = std::min(1 - eps, std::max(eps, sigmoid(margin[(size_t)i * K])));
        acc += -(y[i] * std::log(pr) + (1 - y[i]) * std::log(1 - pr));
      }
      return acc / n;
    }
    case M_ERROR: {
      double acc = 0;
      for (int i : rows) {
        const double pr = (obj == OBJ_BINARY_LOGITRAW) ? margin[(size_t)i * K] : sigmoid(margin[(size_t)i * K]);
        const double thr = (obj == OBJ_BINARY_LOGITRAW) ? 0.0 : 0.5;
        acc += ((pr > thr) ? 1.0 : 0.0) != (y[i] > 0.5 ? 1.0 : 0.0);
      }
      return acc / n;
    }
    case M_AUC: {
      std::vector<double> s, yy;
      for (int i : rows) { s.push_back(margin[(size_t)i * K]); yy.push_back(y[i]); }
      return auc_score(s, yy);
    }
    case M_MERROR: case M_MLOGLOSS: {
      double acc = 0;
      for (int i : rows) {
        const double* m = &margin[(size_t)i * K];
        int arg = 0;
        double mx = m[0];
        for (int k = 1; k < K; ++k) if (m[k] > mx) { mx = m[k]; arg = k; }
        if (metric == M_MERROR) { acc += (arg != (int)y[i]); continue; }
        double z = 0;
        for (int k = 0; k < K; ++k) z += std::exp(m[k] - mx);
        const int c = (int)y[i];
        const double pr = std::max(eps, std::exp(m[c] - mx) / z);
        acc += -std::log(pr);
      }
      return acc / n;
    }
  }
  return 0.0;
}

// One class tree of one booster (gbdt_cv: class c of a fold's round; gbdt_train: of the final model's round):
// the tree's draws from its stream, gradients of the training rows at the current margins, the row sample,
// the tree, and its leaf values added to the margins of every row.
Tree grow_class_tree(const Quantized& q, const float* y, const std::vector<int>& train, std::vector<double>& margin,
                     const Params& p, int objective, int K, int c, uint64_t fold_round) {
  const int n = q.n, F = q.F;
  const bool multi = (objective == OBJ_MULTI_SOFTMAX || objective == OBJ_MULTI_SOFTPROB);
  Rng rng(class_stream(fold_round, c));
  const TreeDraws draws = draw_tree(rng, p, F);
  std::vector<GH> gh(n, GH{0.0, 0.0});
  for (int i : train) {
    const double* m = &margin[(size_t)i * K];
    double g, h;
    if (objective == OBJ_SQUARED) { g = m[0] - y[i]; h = 1.0; }
    else if (!multi) {
      const double pr = sigmoid(m[0]);
      g = pr - y[i]; h = std::max(pr * (1 - pr), 1e-16);
      if (y[i] > 0.5 && objective != OBJ_LOGISTIC) { g *= p.scale_pos_weight; h *= p.scale_pos_weight; }
    } else {
      double mx = m[0];
      for (int j = 1; j < K; ++j) mx = std::max(mx, m[j]);
      double z = 0;
      for (int j = 0; j < K; ++j) z += std::exp(m[j] - mx);
      const double pr = std::exp(m[c] - mx) / z;
      g = pr - ((int)y[i] == c ? 1.0 : 0.0); h = std::max(2.0 * pr * (1 - pr), 1e-16);
    }
    gh[i] = GH{g, h};
  }
  std::vector<int> rows;
  rows.reserve(train.size());
  if (p.subsample < 1.0) {
    // the GPU path (csrc/hip/gbdt_hist.hip root_rows_kernel) samples the same rows in parallel
    for (int i : train) if (row_uniform(draws.row_key, (uint64_t)i) < p.subsample) rows.push_back(i);
  } else {
    rows = train;
  }
  Tree t = build_tree(q, gh, rows, p, draws);
  for (int i = 0; i < n; ++i) margin[(size_t)i * K + c] += t.predict(&q.bins[(size_t)i * F]);
  return t;
}

// A fitted model's trees in the compact layout of gentun_amd/models/booster.py: tree t's nodes are
// [offsets[t], offsets[t + 1]), numbered in level order (build_tree's creation order), right child = left + 1.
struct Forest {
  std::vector<long long> offsets{0};
  std::vector<int> feature, split_bin, left;
  std::vector<float> threshold;
  std::vector<double> value, cover, gain;
  void add(const Tree& t, const Quantized& q) {
    for (const Node& nd : t.nodes) {
      const bool leaf = nd.left < 0;
      feature.push_back(leaf ? -1 : nd.feature);
      split_bin.push_back(leaf ? -1 : nd.split_bin);
      left.push_back(leaf ? -1 : nd.left);
      threshold.push_back(leaf ? 0.f : q.upper[nd.feature][nd.split_bin]);
      value.push_back(nd.value);
      cover.push_back(nd.cover);
      gain.push_back(leaf ? 0.0 : nd.gain);
    }
    offsets.push_back((long long)feature.size());
  }
};

}  // namespace

extern "C" {

#ifndef GT_SRC_HASH
#define GT_SRC_HASH "unhashed"
#endif
// content hash of the sources this library was compiled from (tools/build_native.py)
const char* gt_build_hash() { return GT_SRC_HASH; }

// params: eta, min_child_weight, max_depth, gamma, max_delta_step, subsample,
//         colsample_bytree, colsample_bylevel, lambda, alpha, scale_pos_weight, base_score
// out_hist: [num_boost_round][n_metrics][4] = train-mean, train-std, test-mean, test-std
// returns the number of rows of history kept (best round + 1), or <0 on error.
int gbdt_cv(const float* X, int n, int F, const float* y, const int* fold_of, int nfold, const double* params,
            int objective, int num_class, const int* metrics, int n_metrics, int num_boost_round,
            int early_stopping_rounds, unsigned long long seed, int nthreads, double* out_hist) {
  if (n <= 0 || F <= 0 || nfold <= 0 || n_metrics <= 0) return -1;
  Params p;
  std::memcpy(&p, params, sizeof(Params));
  const bool multi = (objective == OBJ_MULTI_SOFTMAX || objective == OBJ_MULTI_SOFTPROB);
  const int K = multi ? std::max(2, num_class) : 1;
  Quantized q = quantize(X, n, F);
  std::vector<FoldState> folds(nfold);
  for (int k = 0; k < nfold; ++k) {
    for (int i = 0; i < n; ++i) (fold_of[i] == k ? folds[k].test : folds[k].train).push_back(i);
    folds[k].margin.assign((size_t)n * K, base_margin(objective, p.base_score));
  }
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  EarlyStop stop(metrics[n_metrics - 1], early_stopping_rounds);     // the last metric decides
  int rounds_done = 0;
  std::vector<double> train_vals((size_t)n_metrics * nfold), test_vals((size_t)n_metrics * nfold);   // [metric][fold]

  auto round_fold = [&](int k, int round) {
    FoldState& fs = folds[k];
    const uint64_t fold_round = fold_round_seed(seed, k, round);
    for (int c = 0; c < K; ++c) grow_class_tree(q, y, fs.train, fs.margin, p, objective, K, c, fold_round);
    for (int m = 0; m < n_metrics; ++m) {
      train_vals[(size_t)m * nfold + k] = eval_metric(metrics[m], objective, K, fs.train, fs.margin, y);
      test_vals[(size_t)m * nfold + k] = eval_metric(metrics[m], objective, K, fs.test, fs.margin, y);
    }
  };

  for (int round = 0; round < num_boost_round; ++round) {
    if (nthreads > 1 && nfold > 1) {
      std::vector<std::thread> th;
      std::atomic<int> next{0};
      const int nt = std::min(nthreads, nfold);
      for (int t = 0; t < nt; ++t)
        th.emplace_back([&]() { for (int k; (k = next.fetch_add(1)) < nfold;) round_fold(k, round); });
      for (auto& t : th) t.join();
    } else {
      for (int k = 0; k < nfold; ++k) round_fold(k, round);
    }
    for (int m = 0; m < n_metrics; ++m)
      write_fold_stats(&train_vals[(size_t)m * nfold], &test_vals[(size_t)m * nfold], nfold,
                       &out_hist[((size_t)round * n_metrics + m) * 4]);
    rounds_done = round + 1;
    if (stop.update(round, out_hist[((size_t)round * n_metrics + (n_metrics - 1)) * 4 + 2])) break;
  }
  return stop.kept_rows(rounds_done);
}

// Fit the final model: the cv protocol with one fold (index 0) and no test rows, every row a training row, so
// the streams are fold_round_seed(seed, 0, round). out_hist [num_boost_round][n_metrics]: the train metrics;
// out_margin (may be null) [n][K]: the final fp64 margins. *out_forest receives a handle for
// gbdt_forest_size / gbdt_forest_copy / gbdt_forest_free. Returns the number of rounds, or < 0 on error.
int gbdt_train(const float* X, int n, int F, const float* y, const double* params, int objective, int num_class,
               const int* metrics, int n_metrics, int num_boost_round, unsigned long long seed, double* out_hist,
               double* out_margin, void** out_forest) {
  if (n <= 0 || F <= 0 || n_metrics <= 0 || num_boost_round < 0 || out_forest == nullptr) return -1;
  Params p;
  std::memcpy(&p, params, sizeof(Params));
  const bool multi = (objective == OBJ_MULTI_SOFTMAX || objective == OBJ_MULTI_SOFTPROB);
  const int K = multi ? std::max(2, num_class) : 1;
  const Quantized q = quantize(X, n, F);
  std::vector<int> train(n);
  std::iota(train.begin(), train.end(), 0);
  std::vector<double> margin((size_t)n * K, base_margin(objective, p.base_score));
  Forest* forest = new Forest();
  for (int round = 0; round < num_boost_round; ++round) {
    const uint64_t fold_round = fold_round_seed(seed, 0, round);
    for (int c = 0; c < K; ++c) forest->add(grow_class_tree(q, y, train, margin, p, objective, K, c, fold_round), q);
    for (int m = 0; m < n_metrics; ++m)
      out_hist[(size_t)round * n_metrics + m] = eval_metric(metrics[m], objective, K, train, margin, y);
  }
  if (out_margin) std::memcpy(out_margin, margin.data(), sizeof(double) * margin.size());
  *out_forest = forest;
  return num_boost_round;
}

// sizes[0] = trees, sizes[1] = nodes
int gbdt_forest_size(const void* forest, long long* sizes) {
  const Forest* f = static_cast<const Forest*>(forest);
  sizes[0] = (long long)f->offsets.size() - 1;
  sizes[1] = (long long)f->feature.size();
  return 0;
}

int gbdt_forest_copy(const void* forest, long long* offsets, int* feature, float* threshold, int* split_bin, int* left,
                     double* value) {
  const Forest* f = static_cast<const Forest*>(forest);
  const size_t N = f->feature.size();
  std::memcpy(offsets, f->offsets.data(), sizeof(long long) * f->offsets.size());
  if (N == 0) return 0;
  std::memcpy(feature, f->feature.data(), sizeof(int) * N);
  std::memcpy(threshold, f->threshold.data(), sizeof(float) * N);
  std::memcpy(split_bin, f->split_bin.data(), sizeof(int) * N);
  std::memcpy(left, f->left.data(), sizeof(int) * N);
  std::memcpy(value, f->value.data(), sizeof(double) * N);
  return 0;
}

// The node statistics of the same forest, in gbdt_forest_copy's node order: cover (the hessian sum of the rows
// the engine had in the node) and gain (the loss change of the node's split, 0 for leaves).
int gbdt_forest_stats(const void* forest, double* cover, double* gain) {
  const Forest* f = static_cast<const Forest*>(forest);
  const size_t N = f->feature.size();
  if (N == 0) return 0;
  std::memcpy(cover, f->cover.data(), sizeof(double) * N);
  std::memcpy(gain, f->gain.data(), sizeof(double) * N);
  return 0;
}

void gbdt_forest_free(void* forest) { delete static_cast<Forest*>(forest); }

// Predict on raw float rows with a compact forest (tree t: round t / K, class t % K; the first ntrees trees).
// A row goes left when !(x[feature] > threshold) (NaN goes left, as in training); the margin of (row, class) is
// base plus that class's leaf values, added one tree at a time in tree order in fp64. Rows are split over
// nthreads; every (row, class) is summed by one thread in the same order, so the result does not depend on the
// thread count. out_margin [n][K] and out_leaf [n][ntrees] (tree-local leaf indices) may each be null.
int gbdt_predict(const float* X, int n, int F, const long long* offsets, const int* feature, const float* threshold,
                 const int* left, const double* value, int ntrees, int K, double base, int nthreads,
                 double* out_margin, int* out_leaf) {
  if (n < 0 || F <= 0 || K <= 0 || ntrees < 0) return -1;
  for (int t = 0; t < ntrees; ++t)            // a corrupt file must not walk out of bounds
    for (long long j = offsets[t]; j < offsets[t + 1]; ++j) {
      const long long sz = offsets[t + 1] - offsets[t];
      if (feature[j] >= F) return -2;
      if (feature[j] >= 0 && (left[j] <= j - offsets[t] || left[j] + 1 >= sz)) return -2;
    }
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  nthreads = std::max(1, std::min(nthreads, n / 256));
  auto work = [&](int i0, int i1) {
    for (int i = i0; i < i1; ++i) {
      const float* row = X + (size_t)i * F;
      if (out_margin)
        for (int c = 0; c < K; ++c) out_margin[(size_t)i * K + c] = base;
      for (int t = 0; t < ntrees; ++t) {
        const long long o = offsets[t];
        int j = 0;
        while (feature[o + j] >= 0) j = !(row[feature[o + j]] > threshold[o + j]) ? left[o + j] : left[o + j] + 1;
        if (out_margin) out_margin[(size_t)i * K + t % K] += value[o + j];
        if (out_leaf) out_leaf[(size_t)i * ntrees + t] = j;
      }
    }
  };
  if (nthreads == 1) {
    work(0, n);
    return 0;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; ++t)
    th.emplace_back(work, (int)((long long)n * t / nthreads), (int)((long long)n * (t + 1) / nthreads));
  for (auto& x : th) x.join();
  return 0;
}

// SHAP contributions of raw float rows (csrc/gbdt/shap_tables.h has the definition and the shared arithmetic):
// out [n][K][F + 1] fp64, the last column the bias. The forest checks of gbdt_predict plus the cover checks
// (-2), at most 64 unique features on a path (-3). Rows are split over nthreads; every (row, class) is
// computed by one thread in the header's order, so the result does not depend on the thread count.
int gbdt_predict_contribs(const float* X, int n, int F, const long long* offsets, const int* feature,
                          const float* threshold, const int* left, const double* value, const double* cover,
                          int ntrees, int K, double base, int nthreads, double* out) {
  if (n < 0 || F <= 0 || K <= 0 || ntrees < 0 || ntrees % K || cover == nullptr || out == nullptr) return -1;
  ShapTables tb;
  if (const int rc = shap_build(F, offsets, feature, threshold, left, value, cover, ntrees, K, base, tb)) return rc;
  const int rounds = ntrees / K;
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  nthreads = std::max(1, std::min(nthreads, n / 16));
  auto work = [&](int i0, int i1) {
    double w[kShapMaxPath + 1];
    for (int i = i0; i < i1; ++i) {
      const float* row = X + (size_t)i * F;
      for (int c = 0; c < K; ++c) {
        double* phi = out + ((size_t)i * K + c) * ((size_t)F + 1);
        std::fill(phi, phi + F, 0.0);
        phi[F] = tb.bias[c];
        for (int l = tb.leaf_off[c * rounds]; l < tb.leaf_off[(c + 1) * rounds]; ++l) {
          const ShapLeaf& lf = tb.leaves[l];
          shap_leaf(tb.elems.data() + lf.e0, lf.m, lf.value, row, tb.inv.data(), w,
                    [phi](int f, double term) { phi[f] += term; });
        }
      }
    }
  };
  if (nthreads == 1) {
    work(0, n);
    return 0;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; ++t)
    th.emplace_back(work, (int)((long long)n * t / nthreads), (int)((long long)n * (t + 1) / nthreads));
  for (auto& x : th) x.join();
  return 0;
}

// SHAP interaction values of raw float rows (csrc/gbdt/shap_interactions.h has the definition and the shared
// arithmetic): out [n][K][F + 1][F + 1] fp64. Arguments, checks and return codes of gbdt_predict_contribs. A
// (row, class) matrix is accumulated in place by one thread in the header's order -- phi_i on the diagonal, the
// pairs off it -- and finished there, so the result does not depend on the thread count.
int gbdt_predict_interactions(const float* X, int n, int F, const long long* offsets, const int* feature,
                              const float* threshold, const int* left, const double* value, const double* cover,
                              int ntrees, int K, double base, int nthreads, double* out) {
  if (n < 0 || F <= 0 || K <= 0 || ntrees < 0 || ntrees % K || cover == nullptr || out == nullptr) return -1;
  ShapTables tb;
  if (const int rc = shap_build(F, offsets, feature, threshold, left, value, cover, ntrees, K, base, tb)) return rc;
  const int rounds = ntrees / K;
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  nthreads = std::max(1, std::min(nthreads, n / 4));
  const size_t F1 = (size_t)F + 1;
  auto work = [&](int i0, int i1) {
    double w[kShapMaxPath + 1], w2[kShapMaxPath];
    for (int i = i0; i < i1; ++i) {
      const float* row = X + (size_t)i * F;
      for (int c = 0; c < K; ++c) {
        double* phi = out + ((size_t)i * K + c) * F1 * F1;
        std::fill(phi, phi + F1 * F1, 0.0);
        for (int l = tb.leaf_off[c * rounds]; l < tb.leaf_off[(c + 1) * rounds]; ++l) {
          const ShapLeaf& lf = tb.leaves[l];
          shap_leaf_interactions(tb.elems.data() + lf.e0, lf.m, lf.value, row, tb.inv.data(), w, w2,
                                 [](int) { return true; },
                                 [phi, F1](int f, double term) { phi[(size_t)f * F1 + f] += term; },
                                 [phi, F1](int a, int b, double term) { phi[(size_t)a * F1 + b] += term; });
        }
        for (int f = 0; f < F; ++f) {
          const double* r = phi + (size_t)f * F1;
          phi[(size_t)f * F1 + f] = shap_interaction_diagonal(F, f, [r](int j) { return r[j]; });
        }
        phi[F1 * F1 - 1] = tb.bias[c];
      }
    }
  };
  if (nthreads == 1) {
    work(0, n);
    return 0;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; ++t)
    th.emplace_back(work, (int)((long long)n * t / nthreads), (int)((long long)n * (t + 1) / nthreads));
  for (auto& x : th) x.join();
  return 0;
}

// Per-feature upper bounds of the quantiser's bins: nbins_out [F], upper_out [F][256] (the first nbins[f] of
// feature f's row are set). bin = min(lower_bound(upper, v with NaN -> -inf), nbins - 1).
int gbdt_cuts(const float* X, int n, int F, int* nbins_out, float* upper_out) {
  if (n <= 0 || F <= 0) return -1;
  std::vector<std::vector<float>> up(F);
  quantize_into(X, n, F, nullptr, nbins_out, false, up.data());
  for (int f = 0; f < F; ++f) std::copy(up[f].begin(), up[f].end(), upper_out + (size_t)f * kMaxBin);
  return 0;
}

// Quantise only (exposed for the HIP path and tests): bins out [n][F], nbins out [F].
int gbdt_quantize(const float* X, int n, int F, uint8_t* bins_out, int* nbins_out) {
  quantize_into(X, n, F, bins_out, nbins_out, false);
  return 0;
}

// Feature-major bins [F][n] for the GPU histogram path.
int gbdt_quantize_fm(const float* X, int n, int F, uint8_t* bins_out, int* nbins_out) {
  quantize_into(X, n, F, bins_out, nbins_out, true);
  return 0;
}

}  // extern "C"
