// Stand-alone driver of the C++ GBDT engine for host sanitizer builds
// (the reference has no race detection or sanitizers; its
// xgb.cv is an opaque library call, gentun/models/xgboost_models.py:28-37).
//
// Built by tests/test_sanitizers.py together with engine.cpp under
//   -fsanitize=address,undefined   (heap / stack bounds, UB in the split math)
//   -fsanitize=thread              (the multi-threaded histogram / quantiser)
// and run without Python in the process, so every report is the engine's.
// It walks the code paths the GA reaches: every objective family, every
// metric, row / column sampling, L1 / max_delta_step / gamma, early stopping,
// tiny folds (empty leaves) and both quantiser layouts. Then it checks
// cv_protocol.h, what the CPU and the GPU engine share, directly.

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "cv_protocol.h"

extern "C" {
int gbdt_cv(const float* X, int n, int F, const float* y, const int* fold_of, int nfold, const double* params,
            int objective, int num_class, const int* metrics, int n_metrics, int num_boost_round,
            int early_stopping_rounds, unsigned long long seed, int nthreads, double* out_hist);
int gbdt_quantize(const float* X, int n, int F, uint8_t* bins_out, int* nbins_out);
int gbdt_quantize_fm(const float* X, int n, int F, uint8_t* bins_out, int* nbins_out);
int gbdt_train(const float* X, int n, int F, const float* y, const double* params, int objective, int num_class,
               const int* metrics, int n_metrics, int num_boost_round, unsigned long long seed, double* out_hist,
               double* out_margin, void** out_forest);
int gbdt_forest_size(const void* forest, long long* sizes);
int gbdt_forest_copy(const void* forest, long long* offsets, int* feature, float* threshold, int* split_bin, int* left,
                     double* value);
void gbdt_forest_free(void* forest);
int gbdt_predict(const float* X, int n, int F, const long long* offsets, const int* feature, const float* threshold,
                 const int* left, const double* value, int ntrees, int K, double base, int nthreads,
                 double* out_margin, int* out_leaf);
int gbdt_cuts(const float* X, int n, int F, int* nbins_out, float* upper_out);
int gbdt_forest_stats(const void* forest, double* cover, double* gain);
int gbdt_predict_contribs(const float* X, int n, int F, const long long* offsets, const int* feature,
                          const float* threshold, const int* left, const double* value, const double* cover,
                          int ntrees, int K, double base, int nthreads, double* out);
}

namespace {

int failures = 0;

void check(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAIL: %s\n", what);
    ++failures;
  }
}

struct Data {
  int n, F;
  std::vector<float> X, y;
  std::vector<int> fold_of;
};

// kind 0: regression, 1: binary, 2: 3-class
Data make(int n, int F, int kind, int nfold, unsigned seed) {
  std::mt19937 g(seed);
  std::normal_distribution<float> nd(0.f, 1.f);
  Data d{n, F, std::vector<float>(size_t(n) * F), std::vector<float>(n), std::vector<int>(n)};
  for (int i = 0; i < n; ++i) {
    for (int f = 0; f < F; ++f) {
      float v = nd(g);
      if (f % 3 == 2) v = float(int(v * 2.f));      // few distinct values
      d.X[size_t(i) * F + f] = v;
    }
    const float* r = &d.X[size_t(i) * F];
    float s = r[0] - 0.5f * r[1] + 0.25f * r[F - 1] + 0.1f * nd(g);
    d.y[i] = kind == 0 ? s : kind == 1 ? float(s > 0.f) : float(s < -0.5f ? 0 : s < 0.5f ? 1 : 2);
    d.fold_of[i] = i % nfold;
  }
  return d;
}

//           eta  mcw  depth gamma mds  sub  cs_t cs_l lambda alpha spw  base
double P_default[12] = {0.3, 1, 6, 0, 0, 1, 1, 1, 1, 0, 1, 0.5};

int run(const Data& d, int nfold, const double* p, int obj, int ncls, std::vector<int> metrics, int rounds,
        int es, int threads) {
  std::vector<double> hist(size_t(rounds) * metrics.size() * 4, -1.0);
  int kept = gbdt_cv(d.X.data(), d.n, d.F, d.y.data(), d.fold_of.data(), nfold, p, obj, ncls, metrics.data(),
                     int(metrics.size()), rounds, es, 1234ull, threads, hist.data());
  check(kept > 0 && kept <= rounds, "gbdt_cv kept rows");
  for (int r = 0; r < kept; ++r)
    for (size_t j = 0; j < metrics.size() * 4; ++j) check(std::isfinite(hist[r * metrics.size() * 4 + j]), "finite");
  return kept;
}

bool subset(const std::vector<int>& a, const std::vector<int>& of) {
  for (int v : a)
    if (std::find(of.begin(), of.end(), v) == of.end()) return false;
  return true;
}

// the sampling draws: F = 7, colsample_bytree 0.6 -> 4 features, colsample_bylevel 0.5 -> 2 of them per level
void protocol_sampling() {
  using namespace gbdt;
  Params p;
  std::memcpy(&p, P_default, sizeof p);
  p.colsample_bytree = 0.6; p.colsample_bylevel = 0.5;
  const int F = 7;
  Rng a(42), b(42);
  const std::vector<int> ta = tree_features(a, p, F), tb = tree_features(b, p, F);
  const uint64_t ka = a.next(), kb = b.next();
  check(ta == tb && ka == kb, "same seed, same tree features and level key");
  check((int)ta.size() == std::max(1, (int)std::floor(0.6 * F + 1e-9)) && ta.size() == 4, "tree list size");
  check(std::is_sorted(ta.begin(), ta.end()) && std::adjacent_find(ta.begin(), ta.end()) == ta.end() &&
            ta.front() >= 0 && ta.back() < F, "tree list: distinct features, ascending");
  for (int d = 0; d <= 3; ++d) {
    const std::vector<int> la = level_features(ta, ka, d, p);
    check((int)la.size() == std::max(1, (int)std::floor(0.5 * ta.size() + 1e-9)) && la.size() == 2, "level list size");
    check(subset(la, ta) && la[0] != la[1], "level list is a subset of the tree list");
    check(la == level_features(tb, kb, d, p), "same seed, same level list");
  }
  p.colsample_bylevel = 1.0;
  check(level_features(ta, 0, 2, p) == ta, "no level sampling: the tree list");
  p.colsample_bylevel = 0.5;
  // the row key is the stream's first draw, and only with subsample < 1
  Rng r0(42), r1(42);
  const TreeDraws t0 = draw_tree(r0, p, F);
  p.subsample = 0.7;
  const TreeDraws t1 = draw_tree(r1, p, F);
  check(t0.row_key == 0 && t0.feats == ta && t0.level_key == ka, "draw_tree without subsample: features, then level key");
  check(t1.row_key != 0 && (t1.feats != t0.feats || t1.level_key != t0.level_key), "the row key draw shifts the stream");
  const double u = row_uniform(t1.row_key, 5);
  check(u >= 0.0 && u < 1.0 && u == row_uniform(t1.row_key, 5) && u != row_uniform(t1.row_key, 6), "row_uniform");
}

void protocol_stats_and_stopping() {
  using namespace gbdt;
  const double tr[3] = {1.0, 2.0, 3.0}, te[3] = {0.5, 0.5, 2.0};
  double o[4];
  write_fold_stats(tr, te, 3, o);      // population std: sqrt(2 / 3), sqrt((0.25 + 0.25 + 1) / 3)
  check(o[0] == 2.0 && std::fabs(o[1] - std::sqrt(2.0 / 3.0)) < 1e-15, "train mean / std");
  check(o[2] == 1.0 && std::fabs(o[3] - std::sqrt(0.5)) < 1e-15, "test mean / std");
  {
    EarlyStop s(M_RMSE, 2);           // best at round 1; the tie at round 3 does not move it
    const double v[5] = {1.0, 0.8, 0.9, 0.8, 0.7};
    int r = 0;
    while (r < 5 && !s.update(r, v[r])) ++r;
    check(r == 3 && s.kept_rows(r + 1) == 2, "early stopping, lower is better");
  }
  {
    EarlyStop s(M_AUC, 2);            // auc is maximised
    const double v[5] = {0.6, 0.7, 0.7, 0.65, 0.9};
    int r = 0;
    while (r < 5 && !s.update(r, v[r])) ++r;
    check(r == 3 && s.kept_rows(r + 1) == 2, "early stopping, auc");
  }
  {
    EarlyStop s(M_RMSE, 0);           // off: every round is kept
    bool stopped = false;
    for (int r = 0; r < 5; ++r) stopped = stopped || s.update(r, 5.0 - r + (r == 2 ? 9.0 : 0.0));
    check(!stopped && s.kept_rows(5) == 5, "early stopping off");
  }
  check(higher_better(M_AUC) && !higher_better(M_LOGLOSS), "higher_better");
  check(auc_from_rank_sum(7.0, 2, 2) == 1.0 && auc_from_rank_sum(3.0, 2, 2) == 0.0, "auc from rank sum");
  check(auc_from_rank_sum(3.0, 2, 0) == 0.5 && auc_from_rank_sum(0.0, 0, 4) == 0.5, "auc with one class");
  for (int obj = 0; obj <= 5; ++obj) {
    const bool logit = obj == OBJ_LOGISTIC || obj == OBJ_BINARY_LOGISTIC;
    check(base_margin(obj, 0.3) == (logit ? std::log(0.3 / 0.7) : 0.3), "base margin");
    check(base_margin(obj, 0.0) == (logit ? std::log(1e-7 / (1 - 1e-7)) : 0.0), "base score clamped from below");
    check(base_margin(obj, 1.0) == (logit ? std::log((1 - 1e-7) / (1 - (1 - 1e-7))) : 1.0), "base score clamped from above");
  }
}

// gbdt_train -> compact forest -> gbdt_predict: the final margins of the training run, whatever the thread
// count; ntree_limit; leaf indices inside their trees; thresholds = the cuts at the split bins.
void train_predict(const Data& d, const double* p, int obj, int ncls, int metric, int rounds) {
  const int K = ncls > 0 ? ncls : 1;
  std::vector<double> hist(rounds, -1.0), margin(size_t(d.n) * K);
  void* forest = nullptr;
  check(gbdt_train(d.X.data(), d.n, d.F, d.y.data(), p, obj, ncls, &metric, 1, rounds, 99ull, hist.data(),
                   margin.data(), &forest) == rounds && forest != nullptr, "gbdt_train rc");
  if (forest == nullptr) return;
  for (double v : hist) check(std::isfinite(v), "train metric finite");
  long long sz[2];
  gbdt_forest_size(forest, sz);
  check(sz[0] == (long long)rounds * K && sz[1] >= sz[0], "forest size");
  const size_t T = size_t(sz[0]), N = size_t(sz[1]);
  std::vector<long long> off(T + 1);
  std::vector<int> feat(N), sbin(N), left(N);
  std::vector<float> thr(N);
  std::vector<double> val(N);
  gbdt_forest_copy(forest, off.data(), feat.data(), thr.data(), sbin.data(), left.data(), val.data());
  std::vector<double> cover(N), gain(N);
  check(gbdt_forest_stats(forest, cover.data(), gain.data()) == 0, "gbdt_forest_stats rc");
  gbdt_forest_free(forest);
  check(off[0] == 0 && off[T] == (long long)N, "forest offsets");
  if (p[2] == 0) check(N == T, "depth 0: one leaf per tree");
  std::vector<int> nb(d.F);
  std::vector<float> upper(size_t(d.F) * 256);
  check(gbdt_cuts(d.X.data(), d.n, d.F, nb.data(), upper.data()) == 0, "gbdt_cuts rc");
  for (size_t j = 0; j < N; ++j)
    if (feat[j] >= 0) {
      check(feat[j] < d.F && sbin[j] >= 0 && sbin[j] + 1 < nb[feat[j]], "split bin below the last bin");
      check(thr[j] == upper[size_t(feat[j]) * 256 + sbin[j]], "threshold = upper[split_bin]");
    }
  const double base = gbdt::base_margin(obj, p[11]);
  std::vector<double> m1(margin.size()), m4(margin.size());
  check(gbdt_predict(d.X.data(), d.n, d.F, off.data(), feat.data(), thr.data(), left.data(), val.data(), int(T), K, base,
                     1, m1.data(), nullptr) == 0, "gbdt_predict rc");
  check(gbdt_predict(d.X.data(), d.n, d.F, off.data(), feat.data(), thr.data(), left.data(), val.data(), int(T), K, base,
                     4, m4.data(), nullptr) == 0, "gbdt_predict rc, 4 threads");
  check(std::memcmp(m1.data(), margin.data(), sizeof(double) * margin.size()) == 0, "predict = training margins");
  check(std::memcmp(m1.data(), m4.data(), sizeof(double) * margin.size()) == 0, "predict does not depend on threads");
  // ntree_limit: the first round only, margins and leaves together
  std::vector<int> leaf(size_t(d.n) * K);
  check(gbdt_predict(d.X.data(), d.n, d.F, off.data(), feat.data(), thr.data(), left.data(), val.data(), K, K, base, 3,
                     m4.data(), leaf.data()) == 0, "gbdt_predict rc, one round");
  bool ok = true;
  for (int i = 0; i < d.n; ++i)
    for (int c = 0; c < K; ++c) {
      const int j = leaf[size_t(i) * K + c];
      ok = ok && j >= 0 && j < off[c + 1] - off[c] && feat[off[c] + j] < 0 && m4[size_t(i) * K + c] == base + val[off[c] + j];
    }
  check(ok, "one round: margin = base + the leaf's value");
  // rows the model never saw: NaN, infinities, out of range
  std::vector<float> odd(size_t(4) * d.F, NAN);
  for (int f = 0; f < d.F; ++f) { odd[d.F + f] = INFINITY; odd[2 * d.F + f] = -INFINITY; odd[3 * d.F + f] = 1e30f; }
  std::vector<double> mo(size_t(4) * K);
  check(gbdt_predict(odd.data(), 4, d.F, off.data(), feat.data(), thr.data(), left.data(), val.data(), int(T), K, base, 2,
                     mo.data(), nullptr) == 0, "gbdt_predict rc, odd rows");
  for (double v : mo) check(std::isfinite(v), "odd rows: finite margins");
  // node statistics and SHAP contributions: they add up to the margin, whatever the thread count
  double leaf_sum = std::fabs(base);
  long long first_split = -1, first_split_tree = 0;
  for (size_t t = 0; t < T; ++t)
    for (long long j = off[t]; j < off[t + 1]; ++j) {
      check(cover[j] > 0.0 && std::isfinite(cover[j]), "cover positive");
      check(feat[j] >= 0 ? gain[j] > 0.0 : gain[j] == 0.0, "gain: positive at splits, 0 at leaves");
      if (feat[j] < 0) { leaf_sum += std::fabs(val[j]); continue; }
      const long long l = off[t] + left[j];
      check(cover[j] >= cover[l] && cover[j] >= cover[l + 1], "children's covers below the parent's");
      if (first_split < 0) { first_split = j; first_split_tree = (long long)t; }
    }
  const size_t W = size_t(d.F) + 1;
  std::vector<double> c1(size_t(d.n) * K * W, -1.0), c4(c1.size(), -2.0), co(size_t(4) * K * W);
  check(gbdt_predict_contribs(d.X.data(), d.n, d.F, off.data(), feat.data(), thr.data(), left.data(), val.data(),
                              cover.data(), int(T), K, base, 1, c1.data()) == 0, "gbdt_predict_contribs rc");
  check(gbdt_predict_contribs(d.X.data(), d.n, d.F, off.data(), feat.data(), thr.data(), left.data(), val.data(),
                              cover.data(), int(T), K, base, 4, c4.data()) == 0, "gbdt_predict_contribs rc, 4 threads");
  check(std::memcmp(c1.data(), c4.data(), sizeof(double) * c1.size()) == 0, "contribs do not depend on threads");
  check(gbdt_predict_contribs(odd.data(), 4, d.F, off.data(), feat.data(), thr.data(), left.data(), val.data(),
                              cover.data(), int(T), K, base, 2, co.data()) == 0, "gbdt_predict_contribs rc, odd rows");
  ok = true;
  for (int i = 0; i < d.n + 4; ++i)
    for (int c = 0; c < K; ++c) {
      const double* phi = i < d.n ? &c1[(size_t(i) * K + c) * W] : &co[(size_t(i - d.n) * K + c) * W];
      double sum = 0.0;
      for (size_t f = 0; f < W; ++f) sum += phi[f];
      const double m = i < d.n ? m1[size_t(i) * K + c] : mo[size_t(i - d.n) * K + c];
      ok = ok && std::fabs(sum - m) <= 1e-12 * leaf_sum;
    }
  check(ok, "contribs add up to the margin");
  if (first_split >= 0) {              // a zero children's cover sum is a malformed forest
    std::vector<double> bad(cover);
    const long long l = off[first_split_tree] + left[first_split];
    bad[l] = bad[l + 1] = 0.0;
    check(gbdt_predict_contribs(d.X.data(), 4, d.F, off.data(), feat.data(), thr.data(), left.data(), val.data(),
                                bad.data(), int(T), K, base, 1, co.data()) == -2, "zero cover sum: malformed forest");
  }
}

}  // namespace

int main() {
  protocol_sampling();
  protocol_stats_and_stopping();
  // the final model: regression with sampling and a NaN column, multi-class, binary, depth 0
  {
    Data d = make(2500, 7, 0, 1, 6);
    for (int i = 0; i < d.n; ++i) d.X[size_t(i) * d.F + 3] = NAN;
    double p[12];
    std::memcpy(p, P_default, sizeof p);
    p[2] = 5; p[5] = 0.7; p[6] = 0.7; p[7] = 0.6;
    train_predict(d, p, 0, 0, 0, 4);
    p[2] = 0;
    train_predict(d, p, 0, 0, 0, 2);
    Data m = make(1500, 5, 2, 1, 7);
    train_predict(m, P_default, 5, 3, 6, 3);
    Data b = make(1200, 6, 1, 1, 8);
    train_predict(b, P_default, 2, 0, 2, 3);
  }
  // quantiser, both layouts
  {
    Data d = make(5000, 13, 0, 5, 1);
    std::vector<uint8_t> b(size_t(d.n) * d.F), bfm(size_t(d.n) * d.F);
    std::vector<int> nb(d.F), nbfm(d.F);
    check(gbdt_quantize(d.X.data(), d.n, d.F, b.data(), nb.data()) == 0, "quantize rc");
    check(gbdt_quantize_fm(d.X.data(), d.n, d.F, bfm.data(), nbfm.data()) == 0, "quantize_fm rc");
    for (int f = 0; f < d.F; ++f) {
      check(nb[f] == nbfm[f] && nb[f] >= 1 && nb[f] <= 256, "bin counts");
      for (int i = 0; i < d.n; i += 97) check(b[size_t(i) * d.F + f] == bfm[size_t(f) * d.n + i], "layouts agree");
    }
  }
  // regression: sampling, L1, gamma, max_delta_step, early stopping, threads
  {
    Data d = make(3000, 9, 0, 5, 2);
    double p[12];
    std::memcpy(p, P_default, sizeof p);
    p[0] = 0.1; p[2] = 8; p[3] = 0.05; p[4] = 2; p[5] = 0.7; p[6] = 0.6; p[7] = 0.5; p[9] = 0.5;
    run(d, 5, p, 0, 0, {0, 1}, 200, 10, 4);
    run(d, 5, P_default, 1, 0, {0}, 20, 0, 1);        // reg:logistic on unscaled targets still finite
  }
  // binary: weights, logloss / error / auc
  {
    Data d = make(2000, 6, 1, 3, 3);
    double p[12];
    std::memcpy(p, P_default, sizeof p);
    p[10] = 3.0; p[1] = 0; p[8] = 0.1;
    run(d, 3, p, 2, 0, {2, 3, 4}, 50, 5, 3);
    run(d, 3, p, 3, 0, {2}, 10, 0, 2);                 // logitraw
  }
  // multiclass softprob / softmax
  {
    Data d = make(1500, 5, 2, 4, 4);
    run(d, 4, P_default, 5, 3, {5, 6}, 30, 5, 4);
    run(d, 4, P_default, 4, 3, {5}, 10, 0, 1);
  }
  // tiny data: folds of 2-3 rows, deep trees, empty children
  {
    Data d = make(7, 3, 0, 3, 5);
    double p[12];
    std::memcpy(p, P_default, sizeof p);
    p[1] = 0; p[2] = 10; p[8] = 0.0;
    run(d, 3, p, 0, 0, {0}, 5, 0, 8);
  }
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("selftest ok\n");
  return 0;
}
