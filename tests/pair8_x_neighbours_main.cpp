// The lane -> (left, right) address rule of the weights-first launch (csrc/f3d_pair8_plan.h: pair8_x_neighbours,
// pair8_x_neighbour_offset), walked on the host for every lane of every tile column of every width from 1 to 200, over a model of a
// ring slot that holds, for every float the loader puts there, which (array, ring row, column of the volume) it is.  Built and run by
// tests/test_pair8_x_neighbours_cpu.py with AddressSanitizer and UBSan: a read outside the slot is a sanitizer report, a read that names
// the wrong column a line on stderr.
#include <cstdio>
#include <vector>

#include "f3d_pair8_plan.h"

namespace {

struct Cell {
  int array, row, column;
};

int failures = 0;
void fail(const char* what, int width, int tx, int lane, int nj, int array, int row, int got, int expect)
{
  if (++failures <= 20)
    std::fprintf(stderr, "W %d tile column %d lane %d (%d ring rows, array %d, row %d): %s: %d, expected %d\n", width, tx, lane, nj, array, row,
                 what, got, expect);
}

// the slot as the loader fills it: rows [array][row][64] from column x0, halo pieces [array][side][row][4] from column x0-4 / x0+64 --
// or, in a tile at an x face, from inside the row (columns 0 .. 3 / x0+60 .. x0+63: never used, no address leaves the container)
std::vector<Cell> slot_model(int ns, int nj, int x0, int width)
{
  std::vector<Cell> slot(static_cast<size_t>(pair8_slot_floats(ns, nj)), Cell{-1, -1, -1000});
  const bool left_face = x0 == 0, right_face = x0 + kPair8Lanes >= width;
  for (int a = 0; a < ns; ++a)
    for (int j = 0; j < nj; ++j) {
      for (int e = 0; e < kPair8Lanes; ++e) slot[static_cast<size_t>((a * nj + j) * kPair8Lanes + e)] = Cell{a, j, x0 + e};
      for (int s = 0; s < 2; ++s) {
        const int xc = s == 0 ? (left_face ? 0 : x0 - 4) : (right_face ? x0 + kPair8Lanes - 4 : x0 + kPair8Lanes);
        for (int e = 0; e < 4; ++e) slot[static_cast<size_t>(ns * nj * kPair8Lanes + ((a * 2 + s) * nj + j) * 4 + e)] = Cell{a, j, xc + e};
      }
    }
  return slot;
}

void walk(int ns, int nj, int width)
{
  const int ntx = (width + kPair8Lanes - 1) / kPair8Lanes;
  for (int tx = 0; tx < ntx; ++tx) {
    const int x0 = tx * kPair8Lanes;
    const std::vector<Cell> slot = slot_model(ns, nj, x0, width);
    const int floats = static_cast<int>(slot.size());
    for (int lane = 0; lane < kPair8Lanes; ++lane) {
      const int x = x0 + lane;
      const Pair8XNeighbours n = pair8_x_neighbours(lane, x0, width);
      // the rule, restated: columns x-1 and x+1; index -1 is column 1 and index W is column W-2 (a volume one column wide: both reads name
      // column 1, outside it, as the selects of the kernel before did -- its numerator is then (a - a) + b - b of padding on both roads)
      const int want_left = x == 0 ? 1 : x - 1;
      const int want_right = x == width - 1 ? (width == 1 ? 1 : width - 2) : x + 1;
      if (n.left < -1 || n.left > kPair8Lanes) fail("left element", width, tx, lane, nj, 0, 0, n.left, lane - 1);
      if (n.right < -1 || n.right > kPair8Lanes) fail("right element", width, tx, lane, nj, 0, 0, n.right, lane + 1);
      // a halo piece is named by lanes 0 and 63 alone
      if (n.left == -1 && lane != 0) fail("left halo piece named by lane", width, tx, lane, nj, 0, 0, lane, 0);
      if (n.right == kPair8Lanes && lane != kPair8Lanes - 1) fail("right halo piece named by lane", width, tx, lane, nj, 0, 0, lane, 63);
      // ... and each side's by its own read, except where lane 0 is the last column of the volume (W = 64 k + 1, no fold): its right
      // neighbour is its left one
      if (n.left == kPair8Lanes) fail("right halo piece named by a left read", width, tx, lane, nj, 0, 0, n.left, lane - 1);
      if (n.right == -1 && !(lane == 0 && x == width - 1)) fail("left halo piece named by a right read", width, tx, lane, nj, 0, 0, n.right, lane + 1);
      for (int a = 0; a < ns; ++a)
        for (int j = 0; j < nj; ++j) {
          const int ol = pair8_x_neighbour_offset(n.left, a, j, ns, nj), orr = pair8_x_neighbour_offset(n.right, a, j, ns, nj);
          if (ol < 0 || ol >= floats) fail("left offset outside the slot", width, tx, lane, nj, a, j, ol, floats);
          if (orr < 0 || orr >= floats) fail("right offset outside the slot", width, tx, lane, nj, a, j, orr, floats);
          const Cell l = slot[static_cast<size_t>(ol)], r = slot[static_cast<size_t>(orr)];   // (the sanitizer's bound check)
          if (l.array != a || l.row != j) fail("left read of another array or row", width, tx, lane, nj, a, j, l.array * 100 + l.row, a * 100 + j);
          if (r.array != a || r.row != j) fail("right read of another array or row", width, tx, lane, nj, a, j, r.array * 100 + r.row, a * 100 + j);
          if (x >= width) continue;   // lanes beyond the volume do not count: anything inside the slot
          if (l.column != want_left) fail("left column", width, tx, lane, nj, a, j, l.column, want_left);
          if (r.column != want_right) fail("right column", width, tx, lane, nj, a, j, r.column, want_right);
          // what counts is a column of the volume (one column: see above), never a piece that was fetched from inside the row
          if (width > 1 && (l.column < 0 || l.column >= width)) fail("left column outside the volume", width, tx, lane, nj, a, j, l.column, width);
          if (width > 1 && (r.column < 0 || r.column >= width)) fail("right column outside the volume", width, tx, lane, nj, a, j, r.column, width);
          if (x0 == 0 && n.left == -1) fail("left halo piece looked at in a tile at the left face", width, tx, lane, nj, a, j, n.left, 1);
          if (x0 + kPair8Lanes >= width && n.right == kPair8Lanes)
            fail("right halo piece looked at in a tile at the right face", width, tx, lane, nj, a, j, n.right, lane - 1);
        }
    }
  }
}

}  // namespace

int main()
{
  // six stencilled arrays; 8, 12 and 16 ring rows: the tiles of 4, 8 and 12 rows
  for (int nj : {8, 12, 16})
    for (int width = 1; width <= 200; ++width) walk(6, nj, width);
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
