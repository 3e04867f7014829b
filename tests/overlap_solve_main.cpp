// A stand-alone program around the host solve of the overlap rows (cuda-flow3d_amd/host/label_track.cpp), built by
// tests/test_overlap_cpu.py with -fsanitize=address,undefined: a body that breaks in two, two that merge, one that vanishes, one that
// leaves, one that appears, empty bodies on both sides, sums at the limits of the entry (2^33 voxels, coordinates of 2^49), the
// refusals, and heap arrays of exactly n_a and n_b entries whose every entry is written.  Prints "ok" and returns 0, or says what differs.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "label_track.h"

namespace {

typedef struct f3d_overlap Row;

int failures = 0;

void Expect(bool good, const char* what)
{
  if (good) return;
  std::printf("FAILED: %s\n", what);
  ++failures;
}

Row Make(int a, int b, unsigned long long n, long long shift_x2 = 0)
{
  Row r = {};
  r.a = a;
  r.b = b;
  r.n = n;
  // the part moved by shift_x2 / 2 voxels along x: cb2 - ca2 = n * shift_x2
  r.ca2[0] = -static_cast<long long>(n);
  r.cb2[0] = b >= 0 ? r.ca2[0] + static_cast<long long>(n) * shift_x2 : 0;
  return r;
}

}  // namespace

int main()
{
  // A: 1 breaks into B1 (60) and B2 (40); 2 and 3 merge into B3; 4 vanishes (background); 5 leaves; 6 has no voxel.
  // B: 4 appears ((0, 4) alone); 5 is reached by nothing at all.
  std::vector<Row> rows = {Make(0, 4, 30),  Make(1, 1, 60, 4), Make(1, 2, 40, -3), Make(2, 3, 50, 1), Make(3, 3, 45, 1),
                           Make(4, 0, 20),  Make(5, -1, 70),   Make(5, 0, 5)};
  const size_t n_a = 6, n_b = 5;
  std::vector<f3d_track_a> a(n_a);
  std::vector<f3d_track_b> b(n_b);
  std::vector<int> map_b(n_b);
  f3d_track_summary sum = {};
  std::string why;
  Expect(SolveOverlaps(rows.data(), rows.size(), n_a, n_b, 0.1, a.data(), b.data(), map_b.data(), &sum, &why), "the solve runs");

  Expect(a[0].n == 100 && a[0].best_b == 1 && a[0].n_best == 60 && a[0].n_targets == 2 && a[0].fraction == 0.6, "split: sums");
  Expect(a[0].status == (F3D_TRACK_MATCHED | F3D_TRACK_SPLIT) && a[0].shift[0] == 2.0 && a[0].shift[1] == 0.0, "split: status and shift");
  Expect(a[0].iou == 60.0 / 100.0, "split: iou = 60 / (100 + 60 - 60)");
  Expect(a[1].status == F3D_TRACK_MATCHED && a[2].status == 0u && a[2].best_b == 3, "merge: the larger source is the match");
  Expect(a[1].iou == 50.0 / 95.0 && a[2].iou == 45.0 / 95.0, "merge: iou");
  Expect(a[3].status == F3D_TRACK_VANISHED && a[3].n_background == 20 && a[3].best_b == 0 && a[3].iou == 0.0 && std::isnan(a[3].shift[2]),
         "vanished");
  Expect(a[4].status == (F3D_TRACK_VANISHED | F3D_TRACK_LEFT) && a[4].n_lost == 70 && a[4].n == 75 && a[4].fraction == 0.0, "left");
  Expect(a[5].status == F3D_TRACK_EMPTY && a[5].n == 0 && std::isnan(a[5].fraction) && std::isnan(a[5].iou), "empty body of A");

  Expect(b[0].status == F3D_TRACK_MATCHED && b[0].m == 60 && b[0].best_a == 1 && b[0].n_sources == 1, "B1 keeps the number");
  Expect(b[1].status == 0u && b[1].best_a == 1 && b[1].m == 40, "B2 is the smaller fragment");
  Expect(b[2].status == (F3D_TRACK_MATCHED | F3D_TRACK_MERGED) && b[2].m == 95 && b[2].best_a == 2 && b[2].n_sources == 2, "B3 merged");
  Expect(b[3].status == F3D_TRACK_APPEARED && b[3].n_unreached == 30 && b[3].m == 30 && b[3].best_a == 0, "B4 appeared");
  Expect(b[4].status == F3D_TRACK_EMPTY && b[4].m == 0, "B5 empty");
  Expect(map_b[0] == 1 && map_b[1] == 7 && map_b[2] == 2 && map_b[3] == 8 && map_b[4] == 0, "map_b");
  Expect(sum.matched == 2 && sum.split == 1 && sum.merged == 1 && sum.vanished == 2 && sum.appeared == 1 && sum.left == 1 && sum.n_ids == 8,
         "summary");

  // the same rows in another order give the same bytes; a tie goes to the smaller number
  std::vector<Row> turned(rows.rbegin(), rows.rend());
  std::vector<f3d_track_a> a2(n_a);
  std::vector<f3d_track_b> b2(n_b);
  std::vector<int> map2(n_b);
  Expect(SolveOverlaps(turned.data(), turned.size(), n_a, n_b, 0.1, a2.data(), b2.data(), map2.data(), nullptr, &why), "turned rows");
  Expect(map2 == map_b && a2[0].best_b == a[0].best_b && a2[0].shift[0] == a[0].shift[0] && b2[2].best_a == 2, "the order does not matter");
  std::vector<Row> tie = {Make(1, 2, 10), Make(1, 1, 10), Make(2, 1, 10)};
  Expect(SolveOverlaps(tie.data(), tie.size(), 2, 2, 1.0, a2.data(), b2.data(), map2.data(), &sum, &why), "ties");
  Expect(a2[0].best_b == 1 && b2[0].best_a == 1 && (a2[0].status & F3D_TRACK_MATCHED) && a2[0].n_targets == 0 &&
             (a2[0].status & F3D_TRACK_VANISHED),
         "ties go to the smaller number; with min_fraction 1 half a body is no target");

  // the limits of the device entry: 2^33 voxels whose doubled coordinates sum to nearly 2^49
  Row big = {};
  big.a = 1 << 12;
  big.b = 1 << 12;
  big.n = 1ull << 33;
  big.ca2[0] = -((1ll << 49) - 1);
  big.cb2[0] = (1ll << 49) - 1;
  std::vector<f3d_track_a> wide(static_cast<size_t>(1) << 12);
  std::vector<f3d_track_b> wide_b(static_cast<size_t>(1) << 12);
  std::vector<int> wide_map(static_cast<size_t>(1) << 12);
  Expect(SolveOverlaps(&big, 1, wide.size(), wide_b.size(), 0.5, wide.data(), wide_b.data(), wide_map.data(), &sum, &why), "the limits");
  Expect(wide.back().n == 1ull << 33 && wide.back().shift[0] == static_cast<double>((1ll << 50) - 2) / (2.0 * 8589934592.0) &&
             wide.back().iou == 1.0 && wide_map.back() == 1 << 12 && wide_map[0] == 0 && wide[0].status == F3D_TRACK_EMPTY &&
             sum.matched == 1 && sum.n_ids == 1ull << 12,
         "the limits: sums, shift, numbers");

  // refusals write nothing
  a[0].n = 4242;
  const Row outside[4] = {Make(7, 1, 1), Make(1, 6, 1), Make(0, 0, 1), Make(0, -1, 1)};
  for (const Row& r : outside) Expect(!SolveOverlaps(&r, 1, n_a, n_b, 0.1, a.data(), b.data(), map_b.data(), nullptr, &why), "a key outside");
  const double fractions[4] = {0.0, -0.1, 1.5, std::nan("")};
  for (double f : fractions)
    Expect(!SolveOverlaps(rows.data(), rows.size(), n_a, n_b, f, a.data(), b.data(), map_b.data(), nullptr, &why), "min_fraction");
  Expect(a[0].n == 4242 && !why.empty(), "a refused call writes nothing and says why");
  Expect(SolveOverlaps(nullptr, 0, n_a, n_b, 0.1, a.data(), b.data(), map_b.data(), &sum, &why) && a[0].status == F3D_TRACK_EMPTY &&
             sum.n_ids == n_a && map_b[0] == 0,
         "no rows: every body is empty");
  if (failures == 0) std::printf("ok\n");
  return failures ? 1 : 0;
}
