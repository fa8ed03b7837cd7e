// A region spec of the areal prediction (include/mk.h "areal prediction") checked and laid out on the host:
// the partition of the test sites into contiguous runs, the normalised weights and the offsets of the packed
// Cholesky factors.  Standard headers only, so the checks are tested on the host (tests/regionspec_test.cpp).
#pragma once
#include <cmath>
#include <string>
#include <utility>
#include <vector>

namespace mk {

constexpr int REGION_MAXM = 128;   // MK_REGION_MAXM: sites per region at most (one 128-tile of the SYRK)
constexpr int REGION_MAXT = 8;     // MK_MAP_MAXT: thresholds at most

struct RegionPlan {
  int G = 0, n_test = 0, maxm = 0;
  std::vector<int> offsets;    // [G + 1] the first test site of every region, then n_test
  std::vector<double> omega;   // [n_test] weight / (sum of its region's weights, added in index order)
  std::vector<long> foff;      // [G + 1] packed factors of one pair: region g's m_g x m_g block starts at
                               // foff[g] = sum of m^2 over the regions before it; foff[G] doubles in all
};

// The thresholds of a spec: "" when they are fine, else the message (naming the index of a value that is not
// finite, or the count when it is outside 0 .. REGION_MAXT).
inline std::string region_thresholds_check(const double* thresholds, int J) {
  if (J < 0 || J > REGION_MAXT)
    return "areal prediction: n_thresholds = " + std::to_string(J) + " is outside 0 .. " + std::to_string(REGION_MAXT);
  if (J > 0 && !thresholds) return "areal prediction: null thresholds with n_thresholds > 0";
  for (int j = 0; j < J; ++j)
    if (!std::isfinite(thresholds[j]))
      return "areal prediction: threshold " + std::to_string(j) + " is " + std::to_string(thresholds[j]) +
             "; every threshold must be finite";
  return "";
}

// G regions over n_test test sites: offsets [G + 1], weights [n_test] (NULL: every site weighs 1), the sites'
// coordinates cx, cy [n_test] (NULL: the coincidence check is left out).  "" and the plan when the spec is
// fine, else the message naming the offending index; the plan is then untouched.
inline std::string region_plan(int G, const int* offsets, int n_test, const double* weights, const double* cx,
                               const double* cy, RegionPlan* out) {
  if (n_test < 1) return "areal prediction needs test sites: the session has none";
  if (G < 1 || !offsets) return "areal prediction: n_regions = " + std::to_string(G) + " needs offsets[0 .. n_regions]";
  if (offsets[0] != 0) return "areal prediction: offsets[0] = " + std::to_string(offsets[0]) + " must be 0";
  for (int g = 0; g < G; ++g) {
    if (offsets[g + 1] <= offsets[g])
      return "areal prediction: offsets[" + std::to_string(g + 1) + "] = " + std::to_string(offsets[g + 1]) +
             " is not above offsets[" + std::to_string(g) + "] = " + std::to_string(offsets[g]) +
             ": the offsets must increase strictly";
    if (offsets[g + 1] > n_test)
      return "areal prediction: offsets[" + std::to_string(g + 1) + "] = " + std::to_string(offsets[g + 1]) +
             " is past the " + std::to_string(n_test) + " test sites";
    if (offsets[g + 1] - offsets[g] > REGION_MAXM)
      return "areal prediction: region " + std::to_string(g) + " has " + std::to_string(offsets[g + 1] - offsets[g]) +
             " sites; a region holds at most " + std::to_string(REGION_MAXM);
  }
  if (offsets[G] != n_test)
    return "areal prediction: offsets[" + std::to_string(G) + "] = " + std::to_string(offsets[G]) + " must be n_test = " +
           std::to_string(n_test);
  if (weights)
    for (int t = 0; t < n_test; ++t)
      if (!std::isfinite(weights[t]) || weights[t] < 0.0)
        return "areal prediction: weight " + std::to_string(t) + " is " + std::to_string(weights[t]) +
               "; every weight must be finite and >= 0";
  RegionPlan p;
  p.G = G;
  p.n_test = n_test;
  p.offsets.assign(offsets, offsets + G + 1);
  p.omega.assign((size_t)n_test, 0.0);
  p.foff.assign((size_t)G + 1, 0);
  for (int g = 0; g < G; ++g) {
    const int a = offsets[g], b = offsets[g + 1], m = b - a;
    double sum = 0.0;
    for (int t = a; t < b; ++t) sum += weights ? weights[t] : 1.0;
    if (!(sum > 0.0) || !std::isfinite(sum))
      return "areal prediction: the weights of region " + std::to_string(g) + " sum to " + std::to_string(sum) +
             "; every region needs a positive, finite sum";
    for (int t = a; t < b; ++t) p.omega[(size_t)t] = (weights ? weights[t] : 1.0) / sum;
    if (cx && cy)
      for (int i = a; i < b; ++i)
        for (int j = i + 1; j < b; ++j)
          if (cx[i] == cx[j] && cy[i] == cy[j])
            return "areal prediction: test sites " + std::to_string(i) + " and " + std::to_string(j) + " of region " +
                   std::to_string(g) + " have identical coordinates (their joint covariance is singular at every state)";
    p.maxm = m > p.maxm ? m : p.maxm;
    p.foff[(size_t)g + 1] = p.foff[(size_t)g] + (long)m * m;
  }
  *out = std::move(p);
  return "";
}

}  // namespace mk
