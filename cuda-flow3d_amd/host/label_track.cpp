// include/f3d_host.h, f3d_overlap_solve: the definition and the order of evaluation stand there.  Counts are integers; the few doubles
// are one conversion and one division (or one product) each, every operation rounded on its own (built with -ffp-contract=off).
#include "label_track.h"

#include <limits>

namespace {

// `part`'s share of `whole` counts: one product in binary64
bool Counts(unsigned long long part, double min_fraction, unsigned long long whole)
{
  return static_cast<double>(part) >= min_fraction * static_cast<double>(whole);
}

}  // namespace

bool SolveOverlaps(const struct f3d_overlap* rows, size_t count, size_t n_a, size_t n_b, double min_fraction, f3d_track_a* a, f3d_track_b* b,
                   int* map_b, f3d_track_summary* summary, std::string* error)
{
  if (!(min_fraction > 0.0 && min_fraction <= 1.0)) {
    if (error) *error = "f3d_overlap_solve: min_fraction is not in (0, 1]";
    return false;
  }
  for (size_t i = 0; i < count; ++i) {
    const struct f3d_overlap& r = rows[i];
    if (r.a < 0 || static_cast<size_t>(r.a) > n_a || r.b < -1 || (r.b > 0 && static_cast<size_t>(r.b) > n_b) || (r.a == 0 && r.b <= 0)) {
      if (error)
        *error = "f3d_overlap_solve: row " + std::to_string(i) + " has the key (" + std::to_string(r.a) + ", " + std::to_string(r.b) +
                 "), outside 0 .. n_a x -1 .. n_b or without a body";
      return false;
    }
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < n_a; ++i) {
    f3d_track_a t = {};
    t.fraction = t.iou = nan;
    t.shift[0] = t.shift[1] = t.shift[2] = nan;
    a[i] = t;
  }
  for (size_t i = 0; i < n_b; ++i) b[i] = f3d_track_b{};

  // 1. the sums of the rows and the columns, and the best partner of either side: the largest n, ties to the smaller number
  for (size_t i = 0; i < count; ++i) {
    const struct f3d_overlap& r = rows[i];
    if (r.a >= 1) {
      f3d_track_a& t = a[r.a - 1];
      t.n += r.n;
      if (r.b == -1) t.n_lost += r.n;
      if (r.b == 0) t.n_background += r.n;
      if (r.b >= 1 && r.n > 0 && (r.n > t.n_best || (r.n == t.n_best && r.b < t.best_b))) {
        t.n_best = r.n;
        t.best_b = r.b;
        for (int j = 0; j < 3; ++j)
          t.shift[j] = static_cast<double>(r.cb2[j] - r.ca2[j]) / (2.0 * static_cast<double>(r.n));
      }
    }
    if (r.b >= 1) {
      f3d_track_b& t = b[r.b - 1];
      t.m += r.n;
      if (r.a == 0) t.n_unreached += r.n;
      if (r.a >= 1 && r.n > 0 && (r.n > t.n_best || (r.n == t.n_best && r.a < t.best_a))) {
        t.n_best = r.n;
        t.best_a = r.a;
      }
    }
  }
  // 2. the partners whose share counts
  for (size_t i = 0; i < count; ++i) {
    const struct f3d_overlap& r = rows[i];
    if (r.a < 1 || r.b < 1 || r.n == 0) continue;
    if (Counts(r.n, min_fraction, a[r.a - 1].n)) ++a[r.a - 1].n_targets;
    if (Counts(r.n, min_fraction, b[r.b - 1].m)) ++b[r.b - 1].n_sources;
  }
  // 3. the status, the doubles of A, the new numbers of B
  f3d_track_summary s = {};
  for (size_t i = 0; i < n_a; ++i) {
    f3d_track_a& t = a[i];
    if (t.n == 0) {
      t.status = F3D_TRACK_EMPTY;
      continue;
    }
    t.fraction = static_cast<double>(t.n_best) / static_cast<double>(t.n);
    t.iou = 0.0;
    if (t.best_b >= 1) {
      const f3d_track_b& other = b[t.best_b - 1];
      t.iou = static_cast<double>(t.n_best) / static_cast<double>(t.n + other.m - t.n_best);
      if (other.best_a == static_cast<int>(i + 1)) t.status |= F3D_TRACK_MATCHED;
    }
    if (t.n_targets >= 2) t.status |= F3D_TRACK_SPLIT;
    if (t.n_targets == 0) t.status |= F3D_TRACK_VANISHED;
    if (Counts(t.n_lost, min_fraction, t.n)) t.status |= F3D_TRACK_LEFT;
    s.matched += (t.status & F3D_TRACK_MATCHED) ? 1 : 0;
    s.split += (t.status & F3D_TRACK_SPLIT) ? 1 : 0;
    s.vanished += (t.status & F3D_TRACK_VANISHED) ? 1 : 0;
    s.left += (t.status & F3D_TRACK_LEFT) ? 1 : 0;
  }
  s.n_ids = n_a;
  for (size_t i = 0; i < n_b; ++i) {
    f3d_track_b& t = b[i];
    if (t.m == 0) {
      t.status = F3D_TRACK_EMPTY;
      map_b[i] = 0;
      continue;
    }
    if (t.best_a >= 1 && a[t.best_a - 1].best_b == static_cast<int>(i + 1)) t.status |= F3D_TRACK_MATCHED;
    if (t.n_sources >= 2) t.status |= F3D_TRACK_MERGED;
    if (t.n_sources == 0) t.status |= F3D_TRACK_APPEARED;
    s.merged += (t.status & F3D_TRACK_MERGED) ? 1 : 0;
    s.appeared += (t.status & F3D_TRACK_APPEARED) ? 1 : 0;
    map_b[i] = (t.status & F3D_TRACK_MATCHED) ? t.best_a : static_cast<int>(++s.n_ids);
  }
  if (summary) *summary = s;
  return true;
}
