// f3d_histogram_edge, f3d_otsu and f3d_histogram_rank (include/f3d_host.h).  The bin rule is the kernel's own text
// (csrc/f3d_histogram_bin.h); this file is built with contraction off like the rest of the host library.
#include "threshold_select.h"

#include <vector>

#include "../csrc/f3d_histogram_bin.h"

namespace {

constexpr unsigned long long kMostVoxels = 1ull << 33;  // f3d_histogram's limit: M = sum i h_i stays below 2^45

bool Refuse(std::string* why, const char* what)
{
  if (why) *why = what;
  return false;
}

// N and M of the header over [0, i): bins + 1 entries each
bool Prefixes(const unsigned long long* counts, size_t bins, std::vector<unsigned long long>* n, std::vector<unsigned long long>* m,
              std::string* why)
{
  n->assign(bins + 1, 0);
  m->assign(bins + 1, 0);
  for (size_t i = 0; i < bins; ++i) {
    if (counts[i] > kMostVoxels || (*n)[i] + counts[i] > kMostVoxels) return Refuse(why, "the counts add up to more than 2^33");
    (*n)[i + 1] = (*n)[i] + counts[i];
    (*m)[i + 1] = (*m)[i] + static_cast<unsigned long long>(i) * counts[i];
  }
  return true;
}

// one class's term of the objective, every operation rounded on its own
inline double Term(unsigned long long m, unsigned long long n)
{
  const double md = static_cast<double>(m);
  const double square = md * md;
  return square / static_cast<double>(n);
}

}  // namespace

bool HistogramEdge(float lo, float hi, size_t bins, size_t k, float* edge, std::string* why)
{
  if (!edge) return Refuse(why, "no edge to write to");
  f3d_hist::Rule rule;
  if (const char* bad = f3d_hist::make_rule(lo, hi, bins > 0x7fffffff ? 0x7fffffff : static_cast<long long>(bins), &rule))
    return Refuse(why, bad);
  if (k >= bins) return Refuse(why, "k must be below bins");
  if (k == 0) {
    *edge = lo;
    return true;
  }
  // bin_of is monotone over the ordered keys of [lo, hi], bin_of(lo) == 0 < k and bin_of(hi) == bins - 1 >= k: the smallest key whose
  // bin is at least k, by bisection with bin(below) < k <= bin(above) kept throughout
  unsigned below = f3d_hist::key_of(lo), above = f3d_hist::key_of(hi);
  while (above - below > 1) {
    const unsigned middle = below + (above - below) / 2;
    if (f3d_hist::bin_of(rule, f3d_hist::float_of_key(middle)) >= static_cast<int>(k))
      above = middle;
    else
      below = middle;
  }
  *edge = f3d_hist::float_of_key(above);
  return true;
}

bool OtsuCuts(const unsigned long long* counts, size_t bins, int classes, unsigned* cuts, f3d_otsu_info* info, std::string* why)
{
  if (!counts || !cuts || !info) return Refuse(why, "null argument");
  if (bins < 1 || bins > static_cast<size_t>(f3d_hist::kMaxBins)) return Refuse(why, "bins must be 1 .. 4096");
  if (classes != 2 && classes != 3) return Refuse(why, "classes must be 2 or 3");
  std::vector<unsigned long long> n, m;
  if (!Prefixes(counts, bins, &n, &m, why)) return false;
  size_t occupied = 0;
  for (size_t i = 0; i < bins; ++i) occupied += counts[i] != 0;
  f3d_otsu_info result = {};
  if (occupied < static_cast<size_t>(classes)) {
    result.status = F3D_OTSU_DEGENERATE;
    *info = result;
    return true;
  }
  // candidates in lexicographic order, replaced only on strict >: ties go to the smallest cut
  bool found = false;
  double best = 0.0;
  size_t best_1 = 0, best_2 = 0;
  if (classes == 2) {
    for (size_t c = 1; c < bins; ++c) {
      const unsigned long long n0 = n[c], n1 = n[bins] - n[c];
      if (n0 == 0 || n1 == 0) continue;
      const double objective = Term(m[c], n0) + Term(m[bins] - m[c], n1);
      if (!found || objective > best) {
        found = true;
        best = objective;
        best_1 = c;
      }
    }
  } else {
    for (size_t c1 = 1; c1 + 1 < bins; ++c1) {
      const unsigned long long n0 = n[c1];
      if (n0 == 0) continue;
      if (n[bins] == n0) break;  // nothing is left for the other two, here and further on
      const double first = Term(m[c1], n0);
      for (size_t c2 = c1 + 1; c2 < bins; ++c2) {
        const unsigned long long n1 = n[c2] - n[c1], n2 = n[bins] - n[c2];
        if (n1 == 0 || n2 == 0) continue;
        const double objective = (first + Term(m[c2] - m[c1], n1)) + Term(m[bins] - m[c2], n2);
        if (!found || objective > best) {
          found = true;
          best = objective;
          best_1 = c1;
          best_2 = c2;
        }
      }
    }
  }
  if (!found) return Refuse(why, "no candidate although enough bins are occupied");  // cannot happen
  result.status = F3D_OTSU_OK;
  result.objective = best;
  result.populations[0] = n[best_1];
  if (classes == 2) {
    result.populations[1] = n[bins] - n[best_1];
  } else {
    result.populations[1] = n[best_2] - n[best_1];
    result.populations[2] = n[bins] - n[best_2];
  }
  cuts[0] = static_cast<unsigned>(best_1);
  if (classes == 3) cuts[1] = static_cast<unsigned>(best_2);
  *info = result;
  return true;
}

bool HistogramRank(const unsigned long long* counts, size_t bins, unsigned long long r, unsigned* bin, std::string* why)
{
  if (!counts || !bin) return Refuse(why, "null argument");
  if (bins < 1 || bins > static_cast<size_t>(f3d_hist::kMaxBins)) return Refuse(why, "bins must be 1 .. 4096");
  std::vector<unsigned long long> n, m;
  if (!Prefixes(counts, bins, &n, &m, why)) return false;
  if (r >= n[bins]) return Refuse(why, "r must be below the number of used voxels");
  size_t b = 0;
  while (n[b + 1] <= r) ++b;  // the first bin whose cumulative count exceeds r
  *bin = static_cast<unsigned>(b);
  return true;
}
