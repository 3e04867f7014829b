// A stand-alone program around the host solve of the per-label field sums (cuda-flow3d_amd/host/label_field.cpp with
// host/threshold_select.cpp), built by tests/test_label_field_cpu.py with -fsanitize=address,undefined: a constant body (variance exactly
// 0), a body whose sum of squares needs the high limb and the 128-bit product, an empty and a small label, the three ranks on counts of
// 1, 2, 19, 20 and 21 voxels, the shift rule, the refusals, and heap arrays of exactly n_labels entries and n_labels * bins counts whose
// every entry is read and written.  Prints "ok" and returns 0, or says what differs.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../cuda-flow3d_amd/csrc/f3d_histogram_bin.h"
#include "label_field.h"

namespace {

typedef struct f3d_label_field_sums Row;

int failures = 0;

void Expect(bool good, const char* what)
{
  if (good) return;
  std::printf("FAILED: %s\n", what);
  ++failures;
}

// n voxels of the value s at shift `shift` (s * 2^shift an integer)
Row Constant(unsigned long long n, float s, int shift)
{
  Row r = {};
  const long long q = static_cast<long long>(std::ldexp(static_cast<double>(s), shift));
  r.n = n;
  r.min_key = r.max_key = f3d_hist::key_of(s);
  r.iq = static_cast<long long>(n) * q;
  const unsigned __int128 qq = static_cast<unsigned __int128>(n) * static_cast<unsigned __int128>(q * q);
  r.iqq_lo = static_cast<unsigned long long>(qq & 0xffffffffu);
  r.iqq_hi = static_cast<unsigned long long>(qq >> 32);
  return r;
}

}  // namespace

int main()
{
  std::string why;
  // label 1: constant 3.25; label 2: half at +2^24 and half at -2^24 quanta, 2^30 voxels; label 3: empty; label 4: two voxels
  const size_t n_labels = 4;
  std::vector<Row> rows(n_labels);
  rows[0] = Constant(1000, 3.25f, 4);
  const unsigned long long big = 1ull << 30;  // a power of two: every division below is exact
  rows[1].n = big;
  rows[1].min_key = f3d_hist::key_of(-1048576.0f);
  rows[1].max_key = f3d_hist::key_of(1048576.0f);
  rows[1].iq = 0;
  const unsigned __int128 qq = static_cast<unsigned __int128>(big) << 48;  // below 2^79
  rows[1].iqq_lo = static_cast<unsigned long long>(qq & 0xffffffffu);
  rows[1].iqq_hi = static_cast<unsigned long long>(qq >> 32);
  rows[2].min_key = 0xffffffffull;
  rows[3] = Constant(2, -0.5f, 4);
  std::vector<f3d_label_field_stat> stats(n_labels);
  f3d_label_field_summary sum = {};
  Expect(SolveLabelField(rows.data(), nullptr, n_labels, 4, 0.f, 0.f, 0, 3, stats.data(), &sum, &why), "the solve runs without bins");
  Expect(stats[0].status == F3D_LABEL_OK && stats[0].mean == 3.25 && stats[0].variance == 0.0 && stats[0].std == 0.0 &&
             stats[0].min == 3.25 && stats[0].max == 3.25 && stats[0].n == 1000,
         "a constant body: mean exact, variance exactly 0");
  Expect(stats[1].status == F3D_LABEL_OK && stats[1].mean == 0.0 && stats[1].std == 1048576.0 && stats[1].variance == 1048576.0 * 1048576.0 &&
             stats[1].min == -1048576.0 && stats[1].max == 1048576.0,
         "the high limb and the 128-bit product: std 2^24 quanta = 2^20");
  Expect(stats[2].status == F3D_LABEL_EMPTY && std::isnan(stats[2].mean) && std::isnan(stats[2].min) && std::isnan(stats[2].std) &&
             stats[2].n == 0,
         "an empty label");
  Expect(stats[3].status == F3D_LABEL_SMALL && stats[3].mean == -0.5 && stats[3].variance == 0.0, "a small label is still filled");
  Expect(stats[0].q05_bin == -1 && std::isnan(stats[0].median) && std::isnan(stats[3].q95), "no bins: no quantiles");
  Expect(sum.ok == 2 && sum.empty == 1 && sum.small == 1 && sum.mean == (1000.0 * 3.25 + static_cast<double>(big) * 0.0) / (1000.0 + static_cast<double>(big)),
         "the summary");

  // ranks: m voxels, voxel i in bin i of 32 bins over [0, 32]
  const size_t bins = 32;
  const unsigned long long ms[5] = {1, 2, 19, 20, 21};
  std::vector<Row> few(5);
  std::vector<unsigned> counts(5 * bins, 0u);
  for (size_t l = 0; l < 5; ++l) {
    few[l] = Constant(ms[l], 1.0f, 0);
    for (unsigned long long i = 0; i < ms[l]; ++i) counts[l * bins + i] = 1;
  }
  std::vector<f3d_label_field_stat> ranked(5);
  Expect(SolveLabelField(few.data(), counts.data(), 5, 0, 0.f, 32.f, bins, 1, ranked.data(), nullptr, &why), "the solve runs with bins");
  const int want[5][3] = {{0, 0, 0}, {0, 0, 1}, {0, 9, 18}, {0, 9, 19}, {1, 10, 19}};
  for (size_t l = 0; l < 5; ++l)
    Expect(ranked[l].q05_bin == want[l][0] && ranked[l].median_bin == want[l][1] && ranked[l].q95_bin == want[l][2] &&
               ranked[l].median == want[l][1] + 0.5 && ranked[l].q95 == want[l][2] + 0.5,
           "the ranks (m-1)/20, (m-1)/2, (m-1) - (m-1)/20 and the midpoints of their bins");
  counts.assign(5 * bins, 0u);
  counts[bins - 1] = 7;  // the last bin ends at hi
  Expect(SolveLabelField(few.data(), counts.data(), 5, 0, 0.f, 32.f, bins, 1, ranked.data(), nullptr, &why) && ranked[0].q95 == 31.5 &&
             ranked[1].median_bin == -1 && std::isnan(ranked[1].median),
         "the last bin, and a label whose counts are all zero");

  Expect(LabelFieldShift(0.f, 65535.f, 10) == 8 && LabelFieldShift(-0.07f, 0.02f, 10) == 27 && LabelFieldShift(0.f, 0.f, 10) == 0 &&
             LabelFieldShift(1.f, 2.f, 0) == 0 && LabelFieldShift(-3e38f, 1.f, 5) == -100 && LabelFieldShift(0.f, 1e-40f, 5) == 100 &&
             LabelFieldShift(INFINITY, -INFINITY, 0) == 0,
         "the shift rule");

  // refusals write nothing
  stats[0].n = 4242;
  Expect(!SolveLabelField(rows.data(), nullptr, n_labels, 101, 0.f, 0.f, 0, 1, stats.data(), nullptr, &why), "shift");
  Expect(!SolveLabelField(rows.data(), nullptr, n_labels, 0, 0.f, 1.f, 4, 1, stats.data(), nullptr, &why), "bins without counts");
  Expect(!SolveLabelField(rows.data(), counts.data(), n_labels, 0, 0.f, 1.f, 0, 1, stats.data(), nullptr, &why), "counts without bins");
  Expect(!SolveLabelField(rows.data(), counts.data(), n_labels, 0, 1.f, 1.f, 4, 1, stats.data(), nullptr, &why), "lo == hi");
  Expect(!SolveLabelField(rows.data(), counts.data(), n_labels, 0, 0.f, 1.f, 257, 1, stats.data(), nullptr, &why), "bins above 256");
  Expect(!SolveLabelField(nullptr, nullptr, n_labels, 0, 0.f, 0.f, 0, 1, stats.data(), nullptr, &why), "null sums");
  Expect(stats[0].n == 4242 && !why.empty(), "a refused call writes nothing and says why");
  if (failures == 0) std::printf("ok\n");
  return failures ? 1 : 0;
}
