// Comb-table plan of a proving key: the group size k and the table kind of each of its five MSMs
// (A, B1, K, Z in G1; B2 in G2) within a byte budget.  Host only, so that the search is tested
// without a GPU (tests/native/comb_plan_check.cpp, tests/test_native_comb_plan.py).
//
// A comb MSM over n bases at group size k executes one mixed addition per (group, window, proof),
// ceil(n / k) groups.  Subset-sum tables hold 2^k entries per group and need 254 windows; sign-
// pattern tables hold 2^(k-1) and need 255.  Relative cost of one mixed addition, measured on MI355X
// (Arbo-160 key, ns per (group, window) at 1024 proofs): G1 subset-sum 61.1, G1 sign-pattern 62.8
// (the per-lane negation), G2 subset-sum 171.6, G2 sign-pattern 178.5.
//
// The quotient MSM (Z) is dense: every group varies over the batch in every proof.  The four wire
// MSMs execute only the groups whose scalars vary (the others are summed once per batch): 8 - 16 %
// of them on census paths, all of them in the worst case.  So the cost of a plan weighs the wire
// MSMs by phi in [0, 1]:
//   cost(phi) = sum_i w_i c_i ceil(n_i / k_i),   w = 1 for Z, phi for A, B1, K and B2.
// comb_plan_search minimises cost(phi) over the plans that fit the budget and whose worst-case cost,
// cost(1), stays within `guard` of the cost of the equal-k plan (one k for the four G1 MSMs, one
// for B2: comb_plan_equal, the planner before there was one k per MSM).  It also takes no more
// bytes than the equal-k plan: the steps of that plan are coarse and often leave HBM free, which a
// caller may count on for a second key or a wider batch.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zk {

constexpr int COMB_PLAN_MSMS = 5;
enum { COMB_MSM_A = 0, COMB_MSM_B1 = 1, COMB_MSM_K = 2, COMB_MSM_Z = 3, COMB_MSM_B2 = 4 };
constexpr int COMB_PLAN_MIN_K = 8;
constexpr int COMB_PLAN_MAX_K_SIGNED = 21;     // the digit kernels are instantiated for these
constexpr int COMB_PLAN_MAX_K_UNSIGNED = 20;
constexpr double COMB_PLAN_PHI = 0.5;          // the break-even of the useful move
constexpr double COMB_PLAN_GUARD = 0.02;       // worst-case cost over the equal-k plan's

struct CombPlan {
  int k[COMB_PLAN_MSMS];
  bool sg[COMB_PLAN_MSMS];
  bool fits;   // false: no comb plan fits the budget (k, sg are then the narrowest plan's)
};

inline bool comb_msm_is_g2(int i) { return i == COMB_MSM_B2; }
inline double comb_groups(size_t n, int k) { return (double)((n + (size_t)k - 1) / (size_t)k); }
// cost of the additions of one group over all its windows
inline double comb_group_cost(bool g2, bool sg) {
  return g2 ? (sg ? 255 * 178.5 : 254 * 171.6) : (sg ? 255 * 62.8 : 254 * 61.1);
}
inline double comb_table_bytes(size_t n, bool g2, int k, bool sg) {
  return comb_groups(n, k) * (double)((uint64_t)1 << (k - (sg ? 1 : 0))) * (g2 ? 128.0 : 64.0);
}
inline double comb_plan_bytes(const size_t n[COMB_PLAN_MSMS], const CombPlan& p) {
  double b = 0;
  for (int i = 0; i < COMB_PLAN_MSMS; i++) b += comb_table_bytes(n[i], comb_msm_is_g2(i), p.k[i], p.sg[i]);
  return b;
}
inline double comb_plan_cost(const size_t n[COMB_PLAN_MSMS], const CombPlan& p, double phi) {
  double c = 0;
  for (int i = 0; i < COMB_PLAN_MSMS; i++)
    c += (i == COMB_MSM_Z ? 1.0 : phi) * comb_group_cost(comb_msm_is_g2(i), p.sg[i]) *
         comb_groups(n[i], p.k[i]);
  return c;
}

// One k and one table kind per group: n1 G1 bases, n2 G2 bases, minimising the estimated accumulate
// time with every group executed.  allow_signed = false: witnesses of bits / small integers
// (zkmi_pk_desc.sparse_witness): only subset-sum tables skip their zero digits (measured on the
// Keccak address circuit: 172 ms with them, 280 ms with sign patterns, for 5 % more additions on
// paper).  Nothing fits: k = 8.
inline void comb_plan_equal(size_t n1, size_t n2, double usable_bytes, int* k1, int* k2, bool* sg1,
                            bool* sg2, bool allow_signed) {
  double best = 1e300;
  *k1 = *k2 = COMB_PLAN_MIN_K;
  *sg1 = *sg2 = allow_signed;
  for (int s1 = 0; s1 < (allow_signed ? 2 : 1); s1++)
    for (int s2 = 0; s2 < (allow_signed ? 2 : 1); s2++)
      for (int a = COMB_PLAN_MIN_K; a <= (s1 ? COMB_PLAN_MAX_K_SIGNED : COMB_PLAN_MAX_K_UNSIGNED); a++)
        for (int b = COMB_PLAN_MIN_K; b <= (s2 ? COMB_PLAN_MAX_K_SIGNED : COMB_PLAN_MAX_K_UNSIGNED); b++) {
          const double bytes = comb_table_bytes(n1, false, a, s1 != 0) + comb_table_bytes(n2, true, b, s2 != 0);
          if (bytes > usable_bytes) continue;
          const double cost = comb_groups(n1, a) * comb_group_cost(false, s1 != 0) +
                              comb_groups(n2, b) * comb_group_cost(true, s2 != 0);
          if (cost < best) {
            best = cost;
            *k1 = a;
            *k2 = b;
            *sg1 = s1 != 0;
            *sg2 = s2 != 0;
          }
        }
}

// The equal-k plan of a key as a CombPlan (the four G1 MSMs planned as one set of bases)
inline CombPlan comb_plan_equal5(const size_t n[COMB_PLAN_MSMS], double usable_bytes,
                                 bool allow_signed) {
  int k1, k2;
  bool s1, s2;
  comb_plan_equal(n[0] + n[1] + n[2] + n[3], n[4], usable_bytes, &k1, &k2, &s1, &s2, allow_signed);
  CombPlan p;
  for (int i = 0; i < COMB_PLAN_MSMS; i++) {
    p.k[i] = comb_msm_is_g2(i) ? k2 : k1;
    p.sg[i] = comb_msm_is_g2(i) ? s2 : s1;
  }
  p.fits = comb_plan_bytes(n, p) <= usable_bytes;
  return p;
}

// The plan of least cost(phi) whose tables fit usable_bytes and the bytes of the equal-k plan, and
// whose cost(1) is at most (1 + guard) times that plan's.  An MSM without bases keeps the equal-k plan's k.
// When no plan qualifies (not even the narrowest tables fit), the equal-k plan is returned with
// fits = false.
// Ties go to the fewer bytes.
inline CombPlan comb_plan_search(const size_t n[COMB_PLAN_MSMS], double usable_bytes,
                                 bool allow_signed, double phi = COMB_PLAN_PHI,
                                 double guard = COMB_PLAN_GUARD) {
  const CombPlan ref = comb_plan_equal5(n, usable_bytes, allow_signed);
  const double worst_max = (1.0 + guard) * comb_plan_cost(n, ref, 1.0);
  if (ref.fits && comb_plan_bytes(n, ref) < usable_bytes) usable_bytes = comb_plan_bytes(n, ref);
  // per MSM: the (k, kind) choices no other choice beats in both bytes and cost, bytes ascending
  struct Opt {
    int k;
    bool sg;
    double bytes, cost;   // cost unweighted
  };
  constexpr int MAX_OPTS = 2 * (COMB_PLAN_MAX_K_SIGNED - COMB_PLAN_MIN_K + 1);
  Opt opts[COMB_PLAN_MSMS][MAX_OPTS];
  int n_opts[COMB_PLAN_MSMS];
  for (int i = 0; i < COMB_PLAN_MSMS; i++) {
    const bool g2 = comb_msm_is_g2(i);
    n_opts[i] = 0;
    if (n[i] == 0) {
      opts[i][n_opts[i]++] = {ref.k[i], ref.sg[i], 0.0, 0.0};
      continue;
    }
    Opt all[MAX_OPTS];
    int m = 0;
    for (int s = 0; s < (allow_signed ? 2 : 1); s++)
      for (int k = COMB_PLAN_MIN_K; k <= (s ? COMB_PLAN_MAX_K_SIGNED : COMB_PLAN_MAX_K_UNSIGNED); k++)
        all[m++] = {k, s != 0, comb_table_bytes(n[i], g2, k, s != 0),
                    comb_group_cost(g2, s != 0) * comb_groups(n[i], k)};
    for (int a = 1; a < m; a++)   // insertion sort: bytes, then cost
      for (int b = a; b > 0 && (all[b].bytes < all[b - 1].bytes ||
                                (all[b].bytes == all[b - 1].bytes && all[b].cost < all[b - 1].cost));
           b--) {
        const Opt t = all[b];
        all[b] = all[b - 1];
        all[b - 1] = t;
      }
    double least = 1e300;
    for (int a = 0; a < m; a++)
      if (all[a].cost < least) {
        least = all[a].cost;
        opts[i][n_opts[i]++] = all[a];
      }
  }
  CombPlan best = ref;
  double best_cost = 1e300, best_bytes = 1e300;
  int c[COMB_PLAN_MSMS];
  double bytes[COMB_PLAN_MSMS + 1], cost[COMB_PLAN_MSMS + 1], worst[COMB_PLAN_MSMS + 1];
  bytes[0] = cost[0] = worst[0] = 0;
  // depth-first over the choices; the lists ascend in bytes, so the first that overflows ends its level
  int d = 0;
  c[0] = 0;
  while (d >= 0) {
    if (c[d] >= n_opts[d]) {
      d--;
      if (d >= 0) c[d]++;
      continue;
    }
    const Opt& o = opts[d][c[d]];
    bytes[d + 1] = bytes[d] + o.bytes;
    if (bytes[d + 1] > usable_bytes) {
      c[d] = n_opts[d];
      continue;
    }
    cost[d + 1] = cost[d] + (d == COMB_MSM_Z ? 1.0 : phi) * o.cost;
    worst[d + 1] = worst[d] + o.cost;
    if (d + 1 < COMB_PLAN_MSMS) {
      c[++d] = 0;
      continue;
    }
    if (worst[d + 1] <= worst_max &&
        (cost[d + 1] < best_cost || (cost[d + 1] == best_cost && bytes[d + 1] < best_bytes))) {
      best_cost = cost[d + 1];
      best_bytes = bytes[d + 1];
      for (int i = 0; i < COMB_PLAN_MSMS; i++) {
        best.k[i] = opts[i][c[i]].k;
        best.sg[i] = opts[i][c[i]].sg;
      }
    }
    c[d]++;
  }
  best.fits = best_cost < 1e300;
  return best;
}

}  // namespace zk
