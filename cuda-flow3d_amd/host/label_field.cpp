// include/f3d_host.h, f3d_label_field_solve: the definition stands there, the order of evaluation in label_field.h.  Every operation is
// rounded on its own (the host library is built with -ffp-contract=off).
#include "label_field.h"

#include <cmath>
#include <vector>

#include "../csrc/f3d_histogram_bin.h"
#include "threshold_select.h"

namespace {

bool Refuse(std::string* why, const std::string& what)
{
  if (why) *why = what;
  return false;
}

}  // namespace

int LabelFieldShift(float lo, float hi, unsigned long long finite)
{
  if (finite == 0 || !std::isfinite(lo) || !std::isfinite(hi)) return 0;
  const float m = std::fabs(lo) > std::fabs(hi) ? std::fabs(lo) : std::fabs(hi);
  if (m == 0.f) return 0;
  int e;
  std::frexp(m, &e);  // m = f * 2^e with f in [0.5, 1), also for a denormal
  const int shift = 24 - e;
  return shift < -100 ? -100 : (shift > 100 ? 100 : shift);
}

bool SolveLabelField(const struct f3d_label_field_sums* sums, const unsigned* counts, size_t n_labels, int shift, float lo, float hi,
                     size_t bins, unsigned long long min_voxels, f3d_label_field_stat* stats, f3d_label_field_summary* summary,
                     std::string* why)
{
  if (n_labels && (!sums || !stats)) return Refuse(why, "null argument");
  if (shift < -100 || shift > 100) return Refuse(why, "shift must be -100 .. 100");
  if (bins > 256) return Refuse(why, "bins must be 0 .. 256");
  if (bins == 0 && counts) return Refuse(why, "counts given with bins == 0");
  if (bins != 0 && !counts) return Refuse(why, "null counts with bins > 0");
  std::vector<double> edges;  // the float32 edges of the bins, then hi
  if (bins != 0) {
    f3d_hist::Rule rule;
    if (const char* bad = f3d_hist::make_rule(lo, hi, static_cast<long long>(bins), &rule)) return Refuse(why, bad);
    edges.resize(bins + 1);
    for (size_t k = 0; k < bins; ++k) {
      float edge;
      std::string inner;
      if (!HistogramEdge(lo, hi, bins, k, &edge, &inner)) return Refuse(why, inner);
      edges[k] = static_cast<double>(edge);
    }
    edges[bins] = static_cast<double>(hi);
  }

  const double nan = std::nan("");
  f3d_label_field_summary total = {};
  double weighted = 0.0, weight = 0.0;
  std::vector<unsigned long long> row(bins);
  for (size_t l = 0; l < n_labels; ++l) {
    const struct f3d_label_field_sums& s = sums[l];
    f3d_label_field_stat r = {};
    r.n = s.n;
    r.below = s.below;
    r.above = s.above;
    r.q05_bin = r.median_bin = r.q95_bin = -1;
    r.q05 = r.median = r.q95 = nan;
    if (s.n == 0) {
      r.status = F3D_LABEL_EMPTY;
      r.min = r.max = r.mean = r.variance = r.std = nan;
      ++total.empty;
    } else {
      r.status = s.n < min_voxels ? F3D_LABEL_SMALL : F3D_LABEL_OK;
      r.min = static_cast<double>(f3d_hist::float_of_key(static_cast<unsigned>(s.min_key)));
      r.max = static_cast<double>(f3d_hist::float_of_key(static_cast<unsigned>(s.max_key)));
      const double n = static_cast<double>(s.n);
      r.mean = std::ldexp(static_cast<double>(s.iq) / n, -shift);
      const unsigned __int128 iqq = (static_cast<unsigned __int128>(s.iqq_hi) << 32) + s.iqq_lo;
      const unsigned __int128 magnitude = s.iq < 0 ? -static_cast<unsigned __int128>(s.iq) : static_cast<unsigned __int128>(s.iq);
      const unsigned __int128 v = static_cast<unsigned __int128>(s.n) * iqq - magnitude * magnitude;
      const double vq = (static_cast<double>(v) / n) / n;
      r.variance = std::ldexp(vq, -2 * shift);
      r.std = std::ldexp(std::sqrt(vq), -shift);
      if (r.status == F3D_LABEL_OK) {
        ++total.ok;
        weighted = weighted + n * r.mean;
        weight = weight + n;
      } else {
        ++total.small;
      }
    }
    if (bins != 0) {
      unsigned long long m = 0;
      for (size_t k = 0; k < bins; ++k) m += (row[k] = counts[l * bins + k]);
      if (m > 0) {
        const unsigned long long ranks[3] = {(m - 1) / 20, (m - 1) / 2, (m - 1) - (m - 1) / 20};
        int* const bin_out[3] = {&r.q05_bin, &r.median_bin, &r.q95_bin};
        double* const value_out[3] = {&r.q05, &r.median, &r.q95};
        for (int i = 0; i < 3; ++i) {
          unsigned k;
          std::string inner;
          if (!HistogramRank(row.data(), bins, ranks[i], &k, &inner)) return Refuse(why, inner);
          *bin_out[i] = static_cast<int>(k);
          *value_out[i] = (edges[k] + edges[k + 1]) / 2.0;
        }
      }
    }
    stats[l] = r;
  }
  total.mean = total.ok ? weighted / weight : nan;
  if (summary) *summary = total;
  return true;
}
