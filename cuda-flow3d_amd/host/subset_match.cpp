#include "subset_match.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace {

// of m values: the one at `index` of the sorted order, NaN when there are none
double Ranked(std::vector<double> values, size_t index)
{
  if (values.empty()) return std::numeric_limits<double>::quiet_NaN();
  std::sort(values.begin(), values.end());
  return values[index];
}

}  // namespace

bool TableSubsetMatch(const f3d_subset_match_record* records, const f3d_subset_match_grid* grid, double min_zncc,
                      const float* const* compare, f3d_subset_match_node* nodes, f3d_subset_match_summary* summary, std::string* error)
{
  const f3d_subset_match_grid& q = *grid;
  if (q.step < 1 || q.nx < 1 || q.ny < 1 || q.nz < 1 ||
      static_cast<unsigned long long>(q.nx) * q.ny * q.nz > F3D_SUBSET_MATCH_MAX_NODES) {
    *error = "f3d_subset_match_table: the grid is empty, has more than 2^22 nodes or a step below 1";
    return false;
  }
  if (q.window < 1 || q.window > F3D_SUBSET_MATCH_MAX_WINDOW) {
    *error = "f3d_subset_match_table: the half-window must be 1 .. 8";
    return false;
  }
  // the device entry wants every node inside a box of at most 2^30 voxels a side: the positions below then fit an int
  const long long first[3] = {q.ox, q.oy, q.oz}, counts[3] = {q.nx, q.ny, q.nz};
  for (int axis = 0; axis < 3; ++axis)
    if (first[axis] < 0 || first[axis] + (counts[axis] - 1) * q.step > (1ll << 30)) {
      *error = "f3d_subset_match_table: a node lies below 0 or beyond 2^30";
      return false;
    }
  if (min_zncc != min_zncc) {
    *error = "f3d_subset_match_table: min_zncc is NaN";
    return false;
  }
  if (compare && (!compare[0] || !compare[1] || !compare[2])) {
    *error = "f3d_subset_match_table: compare needs three arrays";
    return false;
  }
  const float nan = std::numeric_limits<float>::quiet_NaN();
  f3d_subset_match_summary total = {};
  std::vector<double> lengths, znccs;
  double squares = 0.0;
  size_t at = 0;
  for (int k = 0; k < q.nz; ++k)
    for (int j = 0; j < q.ny; ++j)
      for (int i = 0; i < q.nx; ++i, ++at) {
        const f3d_subset_match_record& r = records[at];
        f3d_subset_match_node row = {};
        row.position[0] = q.ox + i * q.step;
        row.position[1] = q.oy + j * q.step;
        row.position[2] = q.oz + k * q.step;
        row.status = r.status;
        if (r.status == F3D_SUBSET_OK) {
          if (r.zncc == r.zncc) znccs.push_back(r.zncc);
          if (!(r.zncc >= min_zncc)) row.status = F3D_SUBSET_NODE_LOW;
        }
        row.iterations = r.iterations;
        row.zncc = r.zncc;
        const bool good = row.status == F3D_SUBSET_OK;
        float vector[3];
        for (int c = 0; c < 3; ++c) {
          vector[c] = good ? static_cast<float>(r.p[4 * c]) : nan;
          for (int d = 0; d < 3; ++d) row.grad[3 * c + d] = good ? static_cast<float>(r.p[4 * c + 1 + d]) : nan;
        }
        row.u = vector[0];
        row.v = vector[1];
        row.w = vector[2];
        double d[3] = {0.0, 0.0, 0.0};
        bool finite = compare != nullptr;
        for (int c = 0; c < 3; ++c) {
          if (compare) {
            d[c] = static_cast<double>(compare[c][at]) - static_cast<double>(vector[c]);
            row.diff[c] = static_cast<float>(d[c]);
            if (d[c] != d[c]) finite = false;
          } else {
            row.diff[c] = nan;
          }
        }
        if (good && finite) {
          const double length = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
          lengths.push_back(length);
          squares = squares + length * length;
        }
        total.nodes += 1;
        if (row.status >= 0 && row.status < F3D_SUBSET_NODE_STATUS_COUNT) total.status[row.status] += 1;
        nodes[at] = row;
      }
  const size_t m = lengths.size();
  total.compared = m;
  total.median_zncc = Ranked(znccs, znccs.empty() ? 0 : (znccs.size() - 1) / 2);
  total.rms = m ? std::sqrt(squares / static_cast<double>(m)) : std::numeric_limits<double>::quiet_NaN();
  total.median = Ranked(lengths, m ? (m - 1) / 2 : 0);
  total.p95 = Ranked(lengths, m ? (95 * m + 99) / 100 - 1 : 0);
  if (summary) *summary = total;
  return true;
}

bool LayoutSubsetMatch(size_t width, size_t height, size_t depth, int step, int window, f3d_subset_match_grid* grid, std::string* error)
{
  if (step < 1 || window < 1 || window > F3D_SUBSET_MATCH_MAX_WINDOW) {
    *error = "subset correlation: the step must be at least 1 and the half-window 1 .. 8";
    return false;
  }
  const size_t dims[3] = {width, height, depth};
  const int reach = window + 1;
  int first[3], count[3];
  unsigned long long nodes = 1;
  for (int axis = 0; axis < 3; ++axis) {
    if (dims[axis] < static_cast<size_t>(2 * reach + 1) || dims[axis] > (1u << 30)) {
      *error = std::string("subset correlation: a window of this radius and a voxel round it leave the volume along ") + "xyz"[axis];
      return false;
    }
    const long long room = static_cast<long long>(dims[axis]) - 1 - 2 * reach;
    first[axis] = reach + static_cast<int>((room % step) / 2);
    count[axis] = static_cast<int>((static_cast<long long>(dims[axis]) - 1 - reach - first[axis]) / step + 1);
    nodes *= static_cast<unsigned long long>(count[axis]);
  }
  if (nodes > F3D_SUBSET_MATCH_MAX_NODES) {
    *error = "subset correlation: more than 2^22 nodes (take a larger step)";
    return false;
  }
  const f3d_subset_match_grid laid = {first[0], first[1], first[2], step, count[0], count[1], count[2], window};
  *grid = laid;
  return true;
}
