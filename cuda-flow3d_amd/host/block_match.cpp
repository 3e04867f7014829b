#include "block_match.h"

#include <cmath>
#include <limits>

namespace {

// num / sqrt(da * db) of one shift, from the integers of its record
double Zncc(long long n, long long sa, long long da, const int sums[3])
{
  const long long sb = sums[0], sbb = sums[1], sab = sums[2];
  const long long num = n * sab - sa * sb;
  const long long db = n * sbb - sb * sb;
  const double product = static_cast<double>(da) * static_cast<double>(db);
  return static_cast<double>(num) / std::sqrt(product);
}

}  // namespace

bool SolveBlockMatch(const f3d_block_match_record* records, const f3d_block_match_grid* grid, const int* centre, double min_zncc,
                     f3d_block_match_node* nodes, f3d_block_match_summary* summary, std::string* error)
{
  const f3d_block_match_grid& q = *grid;
  if (q.step < 1 || q.nx < 1 || q.ny < 1 || q.nz < 1 ||
      static_cast<unsigned long long>(q.nx) * q.ny * q.nz > F3D_BLOCK_MATCH_MAX_NODES) {
    *error = "f3d_block_match_solve: the grid is empty, has more than 2^22 nodes or a step below 1";
    return false;
  }
  if (q.window < 1 || q.window > F3D_BLOCK_MATCH_MAX_WINDOW || q.rx < 0 || q.ry < 0 || q.rz < 0) {
    *error = "f3d_block_match_solve: the half-window must be 1 .. 8 and no search radius negative";
    return false;
  }
  if (min_zncc != min_zncc) {
    *error = "f3d_block_match_solve: min_zncc is NaN";
    return false;
  }
  const long long side = 2 * q.window + 1, n = side * side * side;
  const int radius[3] = {q.rx, q.ry, q.rz};
  const float nan = std::numeric_limits<float>::quiet_NaN();
  f3d_block_match_summary total = {};
  size_t at = 0;
  for (int k = 0; k < q.nz; ++k)
    for (int j = 0; j < q.ny; ++j)
      for (int i = 0; i < q.nx; ++i, ++at) {
        const f3d_block_match_record& r = records[at];
        f3d_block_match_node row = {};
        row.position[0] = q.ox + i * q.step;
        row.position[1] = q.oy + j * q.step;
        row.position[2] = q.oz + k * q.step;
        row.evaluated = r.evaluated;
        row.outside = r.outside;
        row.flat = r.flat;
        row.zncc = std::numeric_limits<double>::quiet_NaN();
        row.u = row.v = row.w = nan;
        if (r.status == F3D_BLOCK_MATCH_FLAT) {
          row.status = F3D_BLOCK_NODE_FLAT;
        } else if (r.status != F3D_BLOCK_MATCH_OK) {
          row.status = F3D_BLOCK_NODE_NONE;
        } else {
          const long long sa = r.sa, saa = r.saa;
          const long long da = n * saa - sa * sa;
          const double z0 = Zncc(n, sa, da, r.best);
          row.zncc = z0;
          bool on_face = false;
          for (int axis = 0; axis < 3; ++axis) {
            row.shift[axis] = r.shift[axis];
            const int d = r.shift[axis] - (centre ? centre[3 * at + axis] : 0);
            if (radius[axis] > 0 && (d == radius[axis] || d == -radius[axis])) on_face = true;
            double offset = 0.0;
            if ((r.valid >> (2 * axis) & 3) == 3) {
              const double zm = Zncc(n, sa, da, r.neighbour[2 * axis]);
              const double zp = Zncc(n, sa, da, r.neighbour[2 * axis + 1]);
              const double twice = 2.0 * z0;
              const double curvature = (zm - twice) + zp;
              if (curvature < 0.0) {
                const double slope = zm - zp;
                const double denominator = 2.0 * curvature;
                offset = slope / denominator;
                if (offset < -0.5) offset = -0.5;
                if (offset > 0.5) offset = 0.5;
              }
            }
            row.offset[axis] = offset;
          }
          row.status = z0 < min_zncc ? F3D_BLOCK_NODE_LOW : (on_face ? F3D_BLOCK_NODE_EDGE : F3D_BLOCK_NODE_OK);
          if (row.status != F3D_BLOCK_NODE_LOW) {
            row.u = static_cast<float>(static_cast<double>(row.shift[0]) + row.offset[0]);
            row.v = static_cast<float>(static_cast<double>(row.shift[1]) + row.offset[1]);
            row.w = static_cast<float>(static_cast<double>(row.shift[2]) + row.offset[2]);
          }
        }
        total.nodes += 1;
        total.ok += row.status == F3D_BLOCK_NODE_OK;
        total.flat += row.status == F3D_BLOCK_NODE_FLAT;
        total.none += row.status == F3D_BLOCK_NODE_NONE;
        total.low += row.status == F3D_BLOCK_NODE_LOW;
        total.edge += row.status == F3D_BLOCK_NODE_EDGE;
        nodes[at] = row;
      }
  if (summary) *summary = total;
  return true;
}

bool LayoutBlockMatch(size_t width, size_t height, size_t depth, int step, int window, int rx, int ry, int rz, f3d_block_match_grid* grid,
                      std::string* error)
{
  if (step < 1 || window < 1 || window > F3D_BLOCK_MATCH_MAX_WINDOW || rx < 0 || ry < 0 || rz < 0 ||
      window + rx > F3D_BLOCK_MATCH_MAX_REACH || window + ry > F3D_BLOCK_MATCH_MAX_REACH || window + rz > F3D_BLOCK_MATCH_MAX_REACH) {
    *error = "block matching: the step must be at least 1, the half-window 1 .. 8, no radius negative and window + radius at most 16";
    return false;
  }
  const size_t dims[3] = {width, height, depth};
  int first[3], count[3];
  unsigned long long nodes = 1;
  for (int axis = 0; axis < 3; ++axis) {
    if (dims[axis] < static_cast<size_t>(2 * window + 1) || dims[axis] > (1u << 30)) {
      *error = std::string("block matching: a window of this radius leaves the volume along ") + "xyz"[axis];
      return false;
    }
    const long long room = static_cast<long long>(dims[axis]) - 1 - 2 * window;
    first[axis] = window + static_cast<int>((room % step) / 2);
    count[axis] = static_cast<int>((static_cast<long long>(dims[axis]) - 1 - window - first[axis]) / step + 1);
    nodes *= static_cast<unsigned long long>(count[axis]);
  }
  if (nodes > F3D_BLOCK_MATCH_MAX_NODES) {
    *error = "block matching: more than 2^22 nodes (take a larger step)";
    return false;
  }
  const f3d_block_match_grid laid = {first[0], first[1], first[2], step, count[0], count[1], count[2], window, rx, ry, rz};
  *grid = laid;
  return true;
}
