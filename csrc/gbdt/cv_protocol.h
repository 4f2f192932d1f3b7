// What the two GBDT engines (csrc/gbdt/engine.cpp on the CPU, csrc/hip/gbdt_hist.hip on MI355X) must agree
// on to the bit: the C ABI's codes and parameter block, the random streams and the order every tree draws
// from them, the base margin, the fold statistics, early stopping and xgboost's gain / weight math.
// Plain C++17, no HIP: GBDT_HD marks what the kernels call as well.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#ifdef __HIPCC__
#define GBDT_HD __host__ __device__ __forceinline__
#else
#define GBDT_HD inline
#endif

namespace gbdt {

enum Objective { OBJ_SQUARED = 0, OBJ_LOGISTIC = 1, OBJ_BINARY_LOGISTIC = 2, OBJ_BINARY_LOGITRAW = 3,
                 OBJ_MULTI_SOFTMAX = 4, OBJ_MULTI_SOFTPROB = 5 };
enum Metric { M_RMSE = 0, M_MAE = 1, M_LOGLOSS = 2, M_ERROR = 3, M_AUC = 4, M_MERROR = 5, M_MLOGLOSS = 6 };

// the 12 doubles of the C ABI, in order
struct Params {
  double eta, min_child_weight, max_depth, gamma, max_delta_step, subsample, colsample_bytree,
      colsample_bylevel, lambda, alpha, scale_pos_weight, base_score;
};

GBDT_HD uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { s = splitmix(s); return s; }
};

// counter-based Bernoulli per row: row i of a tree is kept when row_uniform(row key, i) < subsample
GBDT_HD double row_uniform(uint64_t key, uint64_t row) {
  return (splitmix(key ^ splitmix(row)) >> 11) * (1.0 / 9007199254740992.0);
}

// one stream per tree (class c of fold k, round) with a fixed number of draws that do not depend on the
// data, so the GPU engine derives a whole round's draws before its first launch
inline uint64_t fold_round_seed(uint64_t seed, int k, int round) {
  return splitmix(seed ^ splitmix((uint64_t)k * 1000003ull + (uint64_t)round * 7919ull + 17));
}
inline uint64_t class_stream(uint64_t fold_round, int c) {
  return c == 0 ? fold_round : splitmix(fold_round ^ splitmix((uint64_t)c * 0x51ED27ull + 3));
}

// colsample_bytree: the tree's features, ascending
inline std::vector<int> tree_features(Rng& rng, const Params& p, int F) {
  std::vector<int> feats(F);
  std::iota(feats.begin(), feats.end(), 0);
  if (p.colsample_bytree < 1.0) {
    const int k = std::max(1, (int)std::floor(p.colsample_bytree * F + 1e-9));
    for (int i = 0; i < F; ++i) std::swap(feats[i], feats[i + (int)(rng.next() % (uint64_t)(F - i))]);
    feats.resize(k);
    std::sort(feats.begin(), feats.end());
  }
  return feats;
}

// colsample_bylevel: the features of level `depth` in scan order. Every level shuffles with its own stream
// keyed by the tree's level key, so the tree stream's draw count does not depend on how deep the tree grows.
inline std::vector<int> level_features(const std::vector<int>& tree_feats, uint64_t level_key, int depth,
                                       const Params& p) {
  std::vector<int> lf = tree_feats;
  if (p.colsample_bylevel < 1.0 && lf.size() > 1) {
    const int m = (int)lf.size();
    const int k = std::max(1, (int)std::floor(p.colsample_bylevel * m + 1e-9));
    Rng lrng(splitmix(level_key ^ splitmix((uint64_t)depth + 1)));
    for (int i = 0; i < m; ++i) std::swap(lf[i], lf[i + (int)(lrng.next() % (uint64_t)(m - i))]);
    lf.resize(k);
  }
  return lf;
}

// THE draw order of one tree's stream: the row key (only if subsample < 1), the tree features, the level
// key (only if colsample_bylevel < 1)
struct TreeDraws { uint64_t row_key, level_key; std::vector<int> feats; };
inline TreeDraws draw_tree(Rng& rng, const Params& p, int F) {
  TreeDraws t;
  t.row_key = p.subsample < 1.0 ? rng.next() : 0ull;
  t.feats = tree_features(rng, p, F);
  t.level_key = p.colsample_bylevel < 1.0 ? rng.next() : 0ull;
  return t;
}

// logit of base_score for the logistic objectives only
inline double base_margin(int objective, double base_score) {
  if (objective != OBJ_LOGISTIC && objective != OBJ_BINARY_LOGISTIC) return base_score;
  const double b = std::min(1 - 1e-7, std::max(1e-7, base_score));
  return std::log(b / (1 - b));
}
inline bool higher_better(int metric) { return metric == M_AUC; }

// rank_sum: tie-averaged 1-based ranks of the positives among all rows
inline double auc_from_rank_sum(double rank_sum, double n_pos, double n_neg) {
  if (n_pos == 0 || n_neg <= 0) return 0.5;
  return (rank_sum - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg);
}

// out4 = train mean, train std, test mean, test std over the folds (population std)
inline void write_fold_stats(const double* train, const double* test, int nfold, double* out4) {
  double trm = 0, tem = 0, trs = 0, tes = 0;
  for (int k = 0; k < nfold; ++k) { trm += train[k]; tem += test[k]; }
  trm /= nfold; tem /= nfold;
  for (int k = 0; k < nfold; ++k) {
    const double a = train[k] - trm, b = test[k] - tem;
    trs += a * a; tes += b * b;
  }
  out4[0] = trm; out4[1] = std::sqrt(trs / nfold); out4[2] = tem; out4[3] = std::sqrt(tes / nfold);
}

// early stopping on the mean test value of the last metric; a tie does not move the best round
struct EarlyStop {
  bool higher; int patience, best_round = 0; double best_score;
  EarlyStop(int last_metric, int early_stopping_rounds)
      : higher(higher_better(last_metric)), patience(early_stopping_rounds), best_score(higher ? -INFINITY : INFINITY) {}
  bool update(int round, double score) {             // true: stop after this round
    if (higher ? score > best_score : score < best_score) { best_score = score; best_round = round; }
    return patience > 0 && round - best_round >= patience;
  }
  int kept_rows(int rounds_done) const { return patience > 0 ? best_round + 1 : rounds_done; }
};

// xgboost's CalcWeight / CalcGain; P: Params or the kernels' DevParams (same field names)
GBDT_HD double threshold_l1(double g, double alpha) {
  return g > alpha ? g - alpha : (g < -alpha ? g + alpha : 0.0);
}
template <class P> GBDT_HD double calc_weight(const P& p, double G, double H) {
  if (H < p.min_child_weight || H <= 0.0) return 0.0;
  double w = -threshold_l1(G, p.alpha) / (H + p.lambda);
  if (p.max_delta_step != 0.0 && std::fabs(w) > p.max_delta_step) w = std::copysign(p.max_delta_step, w);
  return w;
}
template <class P> GBDT_HD double calc_gain(const P& p, double G, double H) {
  if (H < p.min_child_weight || H <= 0.0) return 0.0;
  if (p.max_delta_step == 0.0) {
    const double t = threshold_l1(G, p.alpha);
    return t * t / (H + p.lambda);
  }
  const double w = calc_weight(p, G, H);
  const double ret = -(2.0 * G * w + (H + p.lambda) * w * w);
  return p.alpha == 0.0 ? ret : ret + p.alpha * std::fabs(w);
}

}  // namespace gbdt
