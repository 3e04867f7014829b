// host/threshold_select.cpp (f3d_histogram_edge, f3d_otsu, f3d_histogram_rank) in a program of its own, built with
// -fsanitize=address,undefined by tests/test_histogram_cpu.py: every edge of every bin against an enumeration of all floats of a
// narrow range, the cuts against a brute force without prefix sums, the ranks against the expanded list, and every refusal with
// sentinels around what must not be written.  Prints one line per group with "N wrong" and ends with "ok histogram host".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../cuda-flow3d_amd/csrc/f3d_histogram_bin.h"
#include "threshold_select.h"

typedef unsigned long long u64;

static int check_edges(float lo, float hi, size_t bins)
{
  f3d_hist::Rule rule;
  if (f3d_hist::make_rule(lo, hi, static_cast<long long>(bins), &rule)) return 1;
  // every float of [lo, hi] in key order
  std::vector<float> all;
  for (unsigned key = f3d_hist::key_of(lo); key <= f3d_hist::key_of(hi); ++key) all.push_back(f3d_hist::float_of_key(key));
  int wrong = 0;
  int last = 0;
  std::vector<float> first(bins, NAN);  // the first float of every bin that occurs
  std::vector<char> seen(bins, 0);
  for (float s : all) {
    const int b = f3d_hist::bin_of(rule, s);
    if (b < last || b < 0 || b >= static_cast<int>(bins)) ++wrong;  // monotone and inside
    last = b;
    if (!seen[b]) {
      seen[b] = 1;
      first[b] = s;
    }
  }
  if (f3d_hist::bin_of(rule, hi) != static_cast<int>(bins) - 1 || f3d_hist::bin_of(rule, lo) != 0) ++wrong;
  for (size_t k = 0; k < bins; ++k) {
    // brute force: the first float whose bin is at least k
    size_t at = k;
    while (at < bins && !seen[at]) ++at;
    float edge = -1.f;
    std::string why;
    if (!HistogramEdge(lo, hi, bins, k, &edge, &why) || at >= bins) {
      ++wrong;
      continue;
    }
    if (std::memcmp(&edge, &first[at], sizeof(float)) != 0) ++wrong;
    if (k > 0 && f3d_hist::bin_of(rule, std::nextafterf(edge, -INFINITY)) >= static_cast<int>(k)) ++wrong;
  }
  return wrong;
}

// where the range is too wide to enumerate: the edge's own bin is at least k (exactly k when the bin occurs) and the float below it is in a lower bin
static int check_edges_by_neighbours(float lo, float hi, size_t bins)
{
  f3d_hist::Rule rule;
  if (f3d_hist::make_rule(lo, hi, static_cast<long long>(bins), &rule)) return 1;
  int wrong = 0;
  float last = lo;
  for (size_t k = 0; k < bins; ++k) {
    float edge = -1.f;
    std::string why;
    if (!HistogramEdge(lo, hi, bins, k, &edge, &why)) return wrong + 1;
    if (!(edge >= last && edge <= hi) || f3d_hist::bin_of(rule, edge) < static_cast<int>(k)) ++wrong;
    if (k > 0 && f3d_hist::bin_of(rule, std::nextafterf(edge, -INFINITY)) >= static_cast<int>(k)) ++wrong;
    last = edge;
  }
  return wrong;
}

static double objective_of(const std::vector<u64>& h, const std::vector<size_t>& cuts, bool* empty)
{
  std::vector<size_t> bounds = {0};
  for (size_t c : cuts) bounds.push_back(c);
  bounds.push_back(h.size());
  double total = 0.0;
  *empty = false;
  for (size_t j = 0; j + 1 < bounds.size(); ++j) {
    u64 n = 0, m = 0;
    for (size_t i = bounds[j]; i < bounds[j + 1]; ++i) {
      n += h[i];
      m += i * h[i];
    }
    if (n == 0) {
      *empty = true;
      return 0.0;
    }
    const double md = static_cast<double>(m);
    const double term = md * md / static_cast<double>(n);
    total = j == 0 ? term : total + term;
  }
  return total;
}

static int check_otsu(const std::vector<u64>& h, int classes)
{
  const size_t bins = h.size();
  bool found = false, empty = false;
  double best = 0.0;
  std::vector<size_t> best_cuts;
  if (classes == 2) {
    for (size_t c = 1; c < bins; ++c) {
      const double v = objective_of(h, {c}, &empty);
      if (!empty && (!found || v > best)) found = true, best = v, best_cuts = {c};
    }
  } else {
    for (size_t c1 = 1; c1 + 1 < bins; ++c1)
      for (size_t c2 = c1 + 1; c2 < bins; ++c2) {
        const double v = objective_of(h, {c1, c2}, &empty);
        if (!empty && (!found || v > best)) found = true, best = v, best_cuts = {c1, c2};
      }
  }
  unsigned cuts[4] = {77, 77, 77, 77};
  f3d_otsu_info info;
  std::memset(&info, 0x5a, sizeof(info));
  std::string why;
  if (!OtsuCuts(h.data(), bins, classes, cuts + 1, &info, &why)) return 1;
  int wrong = 0;
  if (cuts[0] != 77 || cuts[classes] != 77) ++wrong;  // nothing beside the classes - 1 cuts
  if (!found) {
    if (info.status != F3D_OTSU_DEGENERATE || cuts[1] != 77 || cuts[2] != 77 || info.objective != 0.0) ++wrong;
    return wrong;
  }
  if (info.status != F3D_OTSU_OK || std::memcmp(&info.objective, &best, sizeof(double)) != 0) ++wrong;
  u64 total = 0;
  for (int j = 0; j < classes - 1; ++j)
    if (cuts[1 + j] != best_cuts[j]) ++wrong;
  for (int j = 0; j < classes; ++j) total += info.populations[j];
  u64 all = 0;
  for (u64 c : h) all += c;
  if (total != all) ++wrong;
  return wrong;
}

static int check_rank(const std::vector<u64>& h)
{
  std::vector<unsigned> expanded;
  for (size_t b = 0; b < h.size(); ++b)
    for (u64 i = 0; i < h[b]; ++i) expanded.push_back(static_cast<unsigned>(b));
  int wrong = 0;
  std::string why;
  for (size_t r = 0; r < expanded.size(); ++r) {
    unsigned bin = 9999;
    if (!HistogramRank(h.data(), h.size(), r, &bin, &why) || bin != expanded[r]) ++wrong;
  }
  unsigned bin = 9999;
  if (HistogramRank(h.data(), h.size(), expanded.size(), &bin, &why) || bin != 9999) ++wrong;  // r == used is refused, nothing written
  return wrong;
}

static int check_refusals()
{
  int wrong = 0;
  std::string why;
  float edge = 5.f;
  const float inf = INFINITY, nan = NAN;
  const struct { float lo, hi; size_t bins, k; } bad[] = {
      {1.f, 1.f, 4, 0}, {2.f, 1.f, 4, 0}, {nan, 1.f, 4, 0}, {0.f, nan, 4, 0}, {-inf, 1.f, 4, 0}, {0.f, inf, 4, 0}, {0.f, 1.f, 0, 0},
      {0.f, 1.f, 4097, 0}, {0.f, 1.f, 4, 4}, {0.f, 1.f, 4, 99}, {-3e38f, 3e38f, 4, 0}, {0.f, 1e-45f, 4096, 0}};
  for (const auto& b : bad) {
    why.clear();
    if (HistogramEdge(b.lo, b.hi, b.bins, b.k, &edge, &why) || edge != 5.f || why.empty()) ++wrong;
  }
  if (HistogramEdge(0.f, 1.f, 4, 0, nullptr, &why)) ++wrong;
  std::vector<u64> h = {1, 2, 3};
  unsigned cuts[2] = {77, 77};
  f3d_otsu_info info;
  std::memset(&info, 0x5a, sizeof(info));
  const f3d_otsu_info before = info;
  if (OtsuCuts(h.data(), 3, 4, cuts, &info, &why) || OtsuCuts(h.data(), 3, 1, cuts, &info, &why) || OtsuCuts(h.data(), 0, 2, cuts, &info, &why) ||
      OtsuCuts(nullptr, 3, 2, cuts, &info, &why) || OtsuCuts(h.data(), 3, 2, nullptr, &info, &why) || OtsuCuts(h.data(), 3, 2, cuts, nullptr, &why))
    ++wrong;
  std::vector<u64> huge = {1ull << 33, 1};
  if (OtsuCuts(huge.data(), 2, 2, cuts, &info, &why)) ++wrong;
  unsigned bin = 9999;
  if (HistogramRank(huge.data(), 2, 0, &bin, &why) || HistogramRank(nullptr, 2, 0, &bin, &why) || HistogramRank(h.data(), 3, 0, nullptr, &why) ||
      HistogramRank(h.data(), 0, 0, &bin, &why) || HistogramRank(h.data(), 5000, 0, &bin, &why))
    ++wrong;
  if (cuts[0] != 77 || cuts[1] != 77 || bin != 9999 || std::memcmp(&info, &before, sizeof(info)) != 0) ++wrong;
  return wrong;
}

int main()
{
  int total = 0;
  const float narrow_hi = 1.f + 0.0009765625f;  // 1 + 2^-10: 8193 floats
  for (size_t bins : {1u, 2u, 7u, 4096u}) {
    const int wrong = check_edges(1.f, narrow_hi, bins);
    std::printf("edges of [1, 1 + 2^-10] at %zu bins: %d wrong\n", bins, wrong);
    total += wrong;
  }
  {
    // wide ranges, across zero and the denormals, and the widest range the rule accepts
    int wrong = check_edges_by_neighbours(-1.f, 1.f, 256) + check_edges_by_neighbours(0.f, 255.f, 256) +
                check_edges_by_neighbours(-1e-37f, 2e-37f, 7) + check_edges_by_neighbours(-1.5e38f, 1.5e38f, 4096) +
                check_edges_by_neighbours(7.f, 243.f, 64);
    f3d_hist::Rule rule;
    if (f3d_hist::make_rule(-1.f, 1.f, 256, &rule)) ++wrong;
    for (float s : {0.f, -0.f, 1e-45f, -1e-45f, 1e-40f, -1e-40f})
      if (f3d_hist::bin_of(rule, s) != 128 || f3d_hist::class_of(rule, s) != f3d_hist::kUsed) ++wrong;
    if (f3d_hist::class_of(rule, NAN) != f3d_hist::kNan || f3d_hist::class_of(rule, -INFINITY) != f3d_hist::kBelow ||
        f3d_hist::class_of(rule, INFINITY) != f3d_hist::kAbove || f3d_hist::class_of(rule, std::nextafterf(1.f, 2.f)) != f3d_hist::kAbove ||
        f3d_hist::class_of(rule, std::nextafterf(-1.f, -2.f)) != f3d_hist::kBelow || f3d_hist::class_of(rule, 1.f) != f3d_hist::kUsed ||
        f3d_hist::class_of(rule, -1.f) != f3d_hist::kUsed)
      ++wrong;
    std::printf("edges of wide ranges and the classes of the special values: %d wrong\n", wrong);
    total += wrong;
  }
  std::mt19937_64 rng(5);
  {
    int wrong = 0;
    for (int trial = 0; trial < 300; ++trial) {
      const size_t bins = 1 + rng() % 14;
      std::vector<u64> h(bins);
      for (u64& c : h) c = rng() % 3 == 0 ? 0 : rng() % (trial % 2 ? 5 : 100000);  // small counts make ties
      wrong += check_otsu(h, 2) + check_otsu(h, 3);
      if (trial < 40) wrong += check_rank(h);
    }
    // the named cases: two-valued, three-valued, single-bin, empty, symmetric (ties go to the smallest cut)
    wrong += check_otsu({0, 4, 0, 0, 9, 0}, 2) + check_otsu({0, 4, 0, 0, 9, 0}, 3) + check_otsu({3, 0, 5, 0, 0, 7}, 3) +
             check_otsu({0, 0, 11, 0}, 2) + check_otsu({0, 0, 0}, 2) + check_otsu({0}, 2) + check_otsu({5, 1, 0, 0, 1, 5}, 2) +
             check_otsu({1ull << 32, 0, 1ull << 32}, 2);
    std::printf("otsu against a brute force and ranks against the list: %d wrong\n", wrong);
    total += wrong;
  }
  {
    // three classes over many bins: the prefix arrays at their full length
    std::vector<u64> h(192);
    for (size_t i = 0; i < h.size(); ++i) h[i] = 1 + rng() % 1000 + (i % 64 < 8 ? 50000 : 0);
    const int wrong = check_otsu(h, 3) + check_otsu(h, 2);
    std::printf("otsu over 192 bins: %d wrong\n", wrong);
    total += wrong;
    std::vector<u64> wide(4096);
    for (u64& c : wide) c = rng() % 1000;
    unsigned cuts[2];
    f3d_otsu_info info;
    std::string why;
    if (!OtsuCuts(wide.data(), wide.size(), 3, cuts, &info, &why) || !(cuts[0] < cuts[1]) || cuts[1] >= 4096) ++total;
  }
  {
    const int wrong = check_refusals();
    std::printf("refusals: %d wrong\n", wrong);
    total += wrong;
  }
  if (total) return 1;
  std::printf("ok histogram host\n");
  return 0;
}
