#include "solve_schedule.h"

#include <algorithm>
#include <cmath>

bool SolveWeightsPlain(float equation_alpha, float hx, float hy, float hz)
{
  for (float h : {hx, hy, hz}) {
    const float w = equation_alpha / (h * h);   // the kernels' own expression (solve_3d.cu:437-439)
    if (!(w - w == 0.f) || std::signbit(w)) return false;
  }
  return true;
}

std::vector<SweepLaunch> CutSweeps(int K, bool fused, bool tri, bool carry)
{
  std::vector<SweepLaunch> cut;
  for (int first = 0; first < K;) {
    const int left = K - first;
    int sweeps = fused ? std::min(left, tri ? 3 : 2) : 1;
    if (fused && tri && carry && left >= 2 && left <= 4) sweeps = left == 3 ? 1 : 2;   // ... ending in (S, S, P)
    cut.push_back({first, sweeps, false});
    first += sweeps;
  }
  if (fused && carry && !cut.empty()) cut.back().next_weights = cut.back().sweeps == 1 || (tri && cut.back().sweeps == 2);
  return cut;
}

std::vector<SweepLaunch> CutSweepsWeightsFirst(int K)
{
  std::vector<SweepLaunch> cut;
  if (K < 1) return cut;
  cut.push_back({0, 1, false, true});
  for (int first = 1; first < K;) {
    const int sweeps = std::min(K - first, 2);
    cut.push_back({first, sweeps, false, false});
    first += sweeps;
  }
  return cut;
}
