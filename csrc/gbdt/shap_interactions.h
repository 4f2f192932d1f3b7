// What the two SHAP interaction predictors share (CPU: engine.cpp gbdt_predict_interactions; MI355X:
// csrc/hip/gbdt_shap_inter.hip): the per-leaf pair arithmetic and the finishing step, __host__ __device__, on
// the element tables of shap_tables.h. That header comes first, so its fp contract(off) pragma covers this one.
//
// Definition (Booster.predict(pred_interactions=True)): Phi fp64 [F + 1][F + 1] per (row, class), under the value
// function v(S) = sum_t v_t(x, S) of shap_tables.h (cover-weighted, "NaN satisfies left edges only").
//   i != j:  Phi[i][j] = Phi[j][i] = half the Shapley interaction index of features i and j,
//            sum over S in N \ {i, j} of |S|! (F - |S| - 2)! / (2 (F - 1)!) (v(S+ij) - v(S+i) - v(S+j) + v(S));
//   Phi[i][i] = phi_i - sum_{j != i} Phi[i][j], phi_i the pred_contribs value: every row sums to the contribution;
//   Phi[F][F] = the pred_contribs bias, bit for bit; the rest of the last row and column is exactly 0.
// This is xgboost's layout and meaning.
//
// Computed form. A leaf with m merged elements is the game value prod_{S} o prod_{rest} z; features off its path
// are dummies, so for two of its elements a != b
//   Phi[f_a][f_b] += value / 2 (o_a - z_a) (o_b - z_b)
//                    sum_{S in U \ {a, b}} |S|! (m - |S| - 2)! / (m - 1)!  prod_{s in S} o_s  prod_{s not in S} z_s.
// The sum needs no subsets: from the m + 1 path weights w that shap_leaf's extend leaves behind, unwind a into m
// weights w2 (o_a = 1: w2[j] = next (m + 1) / (j + 1), next = w[j] - w2[j] z_a (m - j) / (m + 1), from
// next = w[m]; o_a = 0: w2[j] = w[j] (m + 1) / (z_a (m - j))), then unwind-and-sum b on w2 exactly as shap_leaf
// does on w, with m - 1 in place of m. O(m) per pair, O(m^3) per leaf, a second column of m weights.
// An element with o = 0 and z = 0 zeroes the leaf (shap_leaf's dead rule). Nothing divides: inv[] and rz.
//
// Every unordered pair is computed ONCE, the earlier element (first appearance on the path) unwound first, and the
// same double goes to [f_a][f_b] and [f_b][f_a]: the matrix is symmetric to the bit. A caller that owns only
// some first indices i (the GPU kernel splits them over threads) computes the pairs that touch its features, in
// this same order, and drops the half it does not own; a leaf with none of its features costs it nothing.
//
// Order of additions: one accumulator per (row, class, i, j); a class's trees in round order, a tree's leaves in
// increasing compact node index, a leaf's pairs in element order (a leaf adds to an accumulator at most once).
// phi_i is accumulated by shap_leaf itself in the same pass, in its own order. One finishing step,
// shap_interaction_diagonal, then sets Phi[i][i] = phi_i - (off-diagonal entries of row i added up in increasing j).

#pragma once

#include "shap_tables.h"

namespace gbdt {

// One leaf for one row. e, m, value, row, inv, w as in shap_leaf; w2: m more weights. owns(f): whether the
// caller holds the accumulators whose first index is feature f. add_phi(f, term): phi[f] += term;
// add_pair(i, j, term): Phi[i][j] += term, called for owned i only.
template <class ElemPtr, class Row, class Weights, class Weights2, class Owns, class AddPhi, class AddPair>
SHAP_HD inline void shap_leaf_interactions(ElemPtr e, int m, double value, Row row, const double* inv, Weights w,
                                           Weights2 w2, Owns owns, AddPhi add_phi, AddPair add_pair) {
  uint64_t mine = 0;
  for (int u = 0; u < m; ++u)
    if (owns(e[u].f)) mine |= 1ull << u;
  if (!mine) return;                   // no feature of this leaf is the caller's (or m == 0): nothing to add
  shap_leaf(e, m, value, row, inv, w, [&](int f, double term) { if (owns(f)) add_phi(f, term); });
  if (m < 2) return;
  uint64_t ones = 0;
  for (int u = 0; u < m; ++u) {
    if (shap_follows(e[u], row[e[u].f])) ones |= 1ull << u;
    else if (!(e[u].z > 0.0)) return;  // dead, as in shap_leaf
  }
  // shap_leaf has left the extended weights of the m elements in w[0..m]
  const double half = value * 0.5;
  const double m1 = (double)(m + 1), rm1 = inv[m + 1], m0 = (double)m, rm0 = inv[m];
  for (int a = 0; a + 1 < m; ++a) {
    if (!(mine >> a)) break;           // neither a nor any later element is owned
    const bool own_a = (mine >> a) & 1, oa = (ones >> a) & 1;
    const double za = e[a].z;
    if (oa) {
      double next = w[m];
      for (int j = m - 1; j >= 0; --j) {
        const double tmp = next * m1 * inv[j + 1];
        w2[j] = tmp;
        next = w[j] - tmp * za * (double)(m - j) * rm1;
      }
    } else {
      const double rz = e[a].rz;
      for (int j = m - 1; j >= 0; --j) w2[j] = w[j] * rz * m1 * inv[m - j];
    }
    const double ca = half * ((oa ? 1.0 : 0.0) - za);
    for (int b = a + 1; b < m; ++b) {
      const bool own_b = (mine >> b) & 1;
      if (!own_a && !own_b) continue;
      const double zb = e[b].z;
      const bool ob = (ones >> b) & 1;
      double total = 0.0;
      if (ob) {
        double next = w2[m - 1];
        for (int j = m - 2; j >= 0; --j) {
          const double tmp = next * m0 * inv[j + 1];
          total = total + tmp;
          next = w2[j] - tmp * zb * (double)(m - 1 - j) * rm0;
        }
      } else {
        const double rz = e[b].rz;
        for (int j = m - 2; j >= 0; --j) total = total + w2[j] * rz * m0 * inv[m - 1 - j];
      }
      const double term = ca * ((ob ? 1.0 : 0.0) - zb) * total;
      if (own_a) add_pair(e[a].f, e[b].f, term);
      if (own_b) add_pair(e[b].f, e[a].f, term);
    }
  }
}

// The finishing step of row i of one (row, class): get(j) reads the accumulator (i, j), which holds phi_i for
// j == i. Returns Phi[i][i].
template <class Get>
SHAP_HD inline double shap_interaction_diagonal(int F, int i, Get get) {
  double s = 0.0;
  for (int j = 0; j < F; ++j)
    if (j != i) s = s + get(j);
  return get(i) - s;
}

}  // namespace gbdt
