// Stand-alone driver of gbdt_predict_interactions for host sanitizer builds. Built by
// tests/test_gbdt_interactions_sanitizers.py together with engine.cpp under -fsanitize=address,undefined and
// -fsanitize=thread and run without Python in the process.
//
// A small synthetic forest (2 classes x 3 rounds of full depth-4 trees over 7 features, so paths repeat features
// and elements merge; random positive covers), training-like rows plus NaN / infinite ones. Checked: 1 and 4
// threads give the same bytes; every matrix is symmetric to the bit; its rows add up to the contributions and
// all of it to the margin; the corner is the contributions' bias; the last row and column are otherwise 0.
// Then the ownership rule the GPU kernel relies on (shap_interactions.h): callers that own the first indices
// i mod S == s, for every s, together produce the bytes of a caller that owns everything.

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "shap_interactions.h"

extern "C" {
int gbdt_predict(const float* X, int n, int F, const long long* offsets, const int* feature, const float* threshold,
                 const int* left, const double* value, int ntrees, int K, double base, int nthreads,
                 double* out_margin, int* out_leaf);
int gbdt_predict_contribs(const float* X, int n, int F, const long long* offsets, const int* feature,
                          const float* threshold, const int* left, const double* value, const double* cover,
                          int ntrees, int K, double base, int nthreads, double* out);
int gbdt_predict_interactions(const float* X, int n, int F, const long long* offsets, const int* feature,
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

}  // namespace

int main() {
  const int F = 7, K = 2, rounds = 3, T = K * rounds, depth = 4, n = 96;
  const int nn = (2 << depth) - 1, inner = (1 << depth) - 1;
  const double base = 0.25;
  std::mt19937 g(11);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<double> ud(0.5, 9.0);
  std::vector<long long> off(T + 1);
  std::vector<int> feat(size_t(T) * nn, -1), left(size_t(T) * nn, -1);
  std::vector<float> thr(size_t(T) * nn, 0.f);
  std::vector<double> val(size_t(T) * nn), cover(size_t(T) * nn);
  double leaf_sum = std::fabs(base);
  for (int t = 0; t <= T; ++t) off[t] = (long long)t * nn;
  for (int t = 0; t < T; ++t)
    for (int j = 0; j < nn; ++j) {
      const size_t q = size_t(t) * nn + j;
      if (j < inner) {
        feat[q] = int(g() % F);
        left[q] = 2 * j + 1;
        thr[q] = nd(g);
      } else {
        leaf_sum += std::fabs(val[q] = 0.1 * nd(g));
      }
      cover[q] = ud(g);
    }
  std::vector<float> X(size_t(n) * F);
  for (float& v : X) v = 1.5f * nd(g);
  for (int f = 0; f < F; ++f) {        // the last four rows: NaN, +inf, -inf, out of range
    X[size_t(n - 4) * F + f] = NAN;
    X[size_t(n - 3) * F + f] = INFINITY;
    X[size_t(n - 2) * F + f] = -INFINITY;
    X[size_t(n - 1) * F + f] = 1e30f;
  }
  X[size_t(n - 5) * F + 2] = NAN;

  const size_t W = size_t(F) + 1, M = W * W;
  std::vector<double> p1(size_t(n) * K * M, -1.0), p4(p1.size(), -2.0), contribs(size_t(n) * K * W), margin(size_t(n) * K);
  check(gbdt_predict_interactions(X.data(), n, F, off.data(), feat.data(), thr.data(), left.data(), val.data(),
                                  cover.data(), T, K, base, 1, p1.data()) == 0, "gbdt_predict_interactions rc");
  check(gbdt_predict_interactions(X.data(), n, F, off.data(), feat.data(), thr.data(), left.data(), val.data(),
                                  cover.data(), T, K, base, 4, p4.data()) == 0, "gbdt_predict_interactions rc, 4 threads");
  check(std::memcmp(p1.data(), p4.data(), sizeof(double) * p1.size()) == 0, "interactions do not depend on threads");
  check(gbdt_predict_contribs(X.data(), n, F, off.data(), feat.data(), thr.data(), left.data(), val.data(), cover.data(),
                              T, K, base, 2, contribs.data()) == 0, "gbdt_predict_contribs rc");
  check(gbdt_predict(X.data(), n, F, off.data(), feat.data(), thr.data(), left.data(), val.data(), T, K, base, 1,
                     margin.data(), nullptr) == 0, "gbdt_predict rc");
  const double bound = 1e-12 * leaf_sum;
  bool symmetric = true, rows_add_up = true, all_adds_up = true, corner = true, border = true, some = false;
  for (size_t rc = 0; rc < size_t(n) * K; ++rc) {
    const double* phi = &p1[rc * M];
    double all = 0.0;
    for (size_t i = 0; i < W; ++i) {
      double sum = 0.0;
      for (size_t j = 0; j < W; ++j) {
        symmetric = symmetric && std::memcmp(&phi[i * W + j], &phi[j * W + i], sizeof(double)) == 0;
        sum += phi[i * W + j];
        if (i != j && phi[i * W + j] != 0.0) some = true;
        if ((i == size_t(F)) != (j == size_t(F))) border = border && phi[i * W + j] == 0.0;
      }
      rows_add_up = rows_add_up && std::fabs(sum - contribs[rc * W + i]) <= bound;
      all += sum;
    }
    all_adds_up = all_adds_up && std::fabs(all - margin[rc]) <= bound;
    corner = corner && std::memcmp(&phi[M - 1], &contribs[rc * W + F], sizeof(double)) == 0;
  }
  check(symmetric, "symmetric to the bit");
  check(rows_add_up, "rows add up to the contributions");
  check(all_adds_up, "the matrix adds up to the margin");
  check(corner, "the corner is the contributions' bias");
  check(border, "the last row and column are otherwise 0");
  check(some, "some interaction is not 0");
  check(gbdt_predict_interactions(X.data(), n, F, off.data(), feat.data(), thr.data(), left.data(), val.data(),
                                  cover.data(), T + 1, K, base, 1, p4.data()) == -1, "trees not a multiple of K");

  // ownership by first index: S callers, each keeping its share, make the same bytes as one caller
  gbdt::ShapTables tb;
  check(gbdt::shap_build(F, off.data(), feat.data(), thr.data(), left.data(), val.data(), cover.data(), T, K, base, tb) == 0,
        "shap_build rc");
  double w[gbdt::kShapMaxPath + 1], w2[gbdt::kShapMaxPath];
  for (int S : {1, 2, 4}) {
    bool same = true;
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < K; ++c) {
        std::vector<double> acc(M, 0.0);
        double* a = acc.data();
        for (int s = 0; s < S; ++s)
          for (int l = tb.leaf_off[c * rounds]; l < tb.leaf_off[(c + 1) * rounds]; ++l) {
            const gbdt::ShapLeaf& lf = tb.leaves[l];
            gbdt::shap_leaf_interactions(
                tb.elems.data() + lf.e0, lf.m, lf.value, &X[size_t(i) * F], tb.inv.data(), w, w2,
                [S, s](int f) { return (f & (S - 1)) == s; }, [a, W](int f, double t) { a[f * W + f] += t; },
                [a, W](int x, int y, double t) { a[x * W + y] += t; });
          }
        for (int f = 0; f < F; ++f) {
          const double* r = a + f * W;
          a[f * W + f] = gbdt::shap_interaction_diagonal(F, f, [r](int j) { return r[j]; });
        }
        a[M - 1] = tb.bias[c];
        same = same && std::memcmp(a, &p1[(size_t(i) * K + c) * M], sizeof(double) * M) == 0;
      }
    check(same, "owners by first index make the predictor's bytes");
  }

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("selftest ok\n");
  return 0;
}
