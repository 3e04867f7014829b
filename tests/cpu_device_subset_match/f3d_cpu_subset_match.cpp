// TEST INFRASTRUCTURE: f3d_subset_match (include/f3d_subset_match.h) for the host-memory stand-in of tests/cpu_device.  Plain loops,
// the rule of the header word for word, its "Sums" included: 256 partial sums over the voxels i = l, l + 256, ... and the tree over
// them.  The geometry comes from the stand-in's own f3d_get_container.  This directory's Makefile builds the stand-in with this, the
// entries of tests/cpu_device_block_match and tests/cpu_device_initial beside it, the product's host library against it and the
// command-line tool on top.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

#include "f3d_subset_match.h"

namespace {

constexpr int kLanes = F3D_SUBSET_MATCH_LANES;

struct Box {
  size_t w, h, d, pitch_f, rows;
  size_t at(long long x, long long y, long long z) const
  {
    return (static_cast<size_t>(z) * rows + static_cast<size_t>(y)) * pitch_f + static_cast<size_t>(x);
  }
};

bool geometry(size_t w, size_t h, size_t d, Box* box)
{
  f3d_size4 c;
  if (f3d_get_container(&c) != 0 || c.pitch == 0 || c.height == 0) return false;
  if (w == 0 || h == 0 || d == 0 || w > c.width || h > c.height || d > c.depth || w * sizeof(float) > c.pitch) return false;
  *box = {w, h, d, c.pitch / sizeof(float), c.height};
  return true;
}

// "Sums" of the header: the sum of term(i) over the n voxels of a window
double window_sum(int n, const std::function<double(int)>& term)
{
  double lane[kLanes];
  for (int l = 0; l < kLanes; ++l) {
    lane[l] = 0.0;
    for (int i = l; i < n; i += kLanes) lane[l] += term(i);
  }
  for (int half = kLanes / 2; half > 0; half /= 2)
    for (int l = 0; l < half; ++l) lane[l] += lane[l + half];
  return lane[0];
}

double line(const double w[4], double q0, double q1, double q2, double q3) { return ((w[0] * q0 + w[1] * q1) + w[2] * q2) + w[3] * q3; }

void weights(double t, double w[4])
{
  w[0] = (((2.0 - t) * t - 1.0) * t) * 0.5;
  w[1] = (((3.0 * t - 5.0) * t) * t + 2.0) * 0.5;
  w[2] = (((4.0 - 3.0 * t) * t + 1.0) * t) * 0.5;
  w[3] = (((t - 1.0) * t) * t) * 0.5;
}

// one node by the rule of the header
f3d_subset_match_record node_record(const float* a, const float* b, const Box& box, const long long c[3], int W, int m, const double* start,
                                    int max_iterations, double tolerance, double reach)
{
  f3d_subset_match_record rec;
  std::memset(&rec, 0, sizeof(rec));
  double* p = rec.p;
  if (start) {
    bool nan = false;
    for (int k = 0; k < 12; ++k) {
      p[k] = start[k];
      nan = nan || start[k] != start[k];
    }
    if (nan) {
      rec.status = F3D_SUBSET_NO_START;
      return rec;
    }
  }
  const double u0 = p[0], v0 = p[4], w0 = p[8];
  const int side = 2 * W + 1, n = side * side * side;
  auto xi = [&](int i, int axis) { return (axis == 0 ? i % side : (axis == 1 ? (i / side) % side : i / (side * side))) - W; };
  auto a_at = [&](int i, int dx, int dy, int dz) {
    return static_cast<double>(a[box.at(c[0] + xi(i, 0) + dx, c[1] + xi(i, 1) + dy, c[2] + xi(i, 2) + dz)]);
  };
  // the window
  const double total = window_sum(n, [&](int i) { return a_at(i, 0, 0, 0); });
  const double nans = window_sum(n, [&](int i) {
    const double f = a_at(i, 0, 0, 0);
    return f != f ? 1.0 : 0.0;
  });
  rec.nan = static_cast<int>(nans);
  if (rec.nan > 0) {
    rec.status = F3D_SUBSET_NAN;
    return rec;
  }
  const double fm = total / static_cast<double>(n);
  std::vector<double> F(n), G(n), g(n);
  for (int i = 0; i < n; ++i) F[i] = a_at(i, 0, 0, 0) - fm;
  const double df = std::sqrt(window_sum(n, [&](int i) { return F[i] * F[i]; }));
  rec.df = df;
  if (df == 0.0) {
    rec.status = F3D_SUBSET_FLAT;
    return rec;
  }
  // the Hessian and its factor
  std::vector<double> J(static_cast<size_t>(n) * m);
  for (int i = 0; i < n; ++i) {
    const double d[3] = {(a_at(i, 1, 0, 0) - a_at(i, -1, 0, 0)) * 0.5, (a_at(i, 0, 1, 0) - a_at(i, 0, -1, 0)) * 0.5,
                         (a_at(i, 0, 0, 1) - a_at(i, 0, 0, -1)) * 0.5};
    for (int axis = 0; axis < 3; ++axis) {
      if (m == 3) {
        J[static_cast<size_t>(i) * 3 + axis] = d[axis];
      } else {
        double* row = &J[static_cast<size_t>(i) * 12 + 4 * axis];
        row[0] = d[axis];
        for (int k = 0; k < 3; ++k) row[1 + k] = d[axis] * static_cast<double>(xi(i, k));
      }
    }
  }
  double L[12][12];
  for (int r = 0; r < m; ++r)
    for (int k = 0; k < m; ++k) L[r][k] = window_sum(n, [&](int i) { return J[static_cast<size_t>(i) * m + r] * J[static_cast<size_t>(i) * m + k]; });
  for (int j = 0; j < m; ++j) {
    for (int k = 0; k < j; ++k) {
      double v = L[j][k];
      for (int q = 0; q < k; ++q) v -= L[j][q] * L[k][q];
      L[j][k] = v / L[k][k];
    }
    double d = L[j][j];
    for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
    if (!(d > 0.0)) {
      rec.status = F3D_SUBSET_SINGULAR;
      return rec;
    }
    L[j][j] = std::sqrt(d);
  }
  const double last[3] = {static_cast<double>(box.w) - 3.0, static_cast<double>(box.h) - 3.0, static_cast<double>(box.d) - 3.0};
  for (;;) {
    rec.iterations += 1;
    // the points and g
    int outside = 0;
    for (int i = 0; i < n; ++i) {
      const double e[3] = {static_cast<double>(xi(i, 0)), static_cast<double>(xi(i, 1)), static_cast<double>(xi(i, 2))};
      double at[3], base[3];
      bool in = true;
      for (int axis = 0; axis < 3; ++axis) {
        const double* q = p + 4 * axis;
        at[axis] = static_cast<double>(c[axis] + xi(i, axis)) + (((q[0] + q[1] * e[0]) + q[2] * e[1]) + q[3] * e[2]);
        base[axis] = std::floor(at[axis]);
        in = in && base[axis] >= 1.0 && base[axis] <= last[axis];
      }
      if (!in) {
        ++outside;
        continue;
      }
      double wx[4], wy[4], wz[4], planes[4];
      weights(at[0] - base[0], wx);
      weights(at[1] - base[1], wy);
      weights(at[2] - base[2], wz);
      const long long ix = static_cast<long long>(base[0]) - 1, iy = static_cast<long long>(base[1]) - 1, iz = static_cast<long long>(base[2]) - 1;
      for (int kz = 0; kz < 4; ++kz) {
        double rows[4];
        for (int ky = 0; ky < 4; ++ky) {
          const float* row = b + box.at(ix, iy + ky, iz + kz);
          rows[ky] = line(wx, static_cast<double>(row[0]), static_cast<double>(row[1]), static_cast<double>(row[2]), static_cast<double>(row[3]));
        }
        planes[kz] = line(wy, rows[0], rows[1], rows[2], rows[3]);
      }
      g[i] = line(wz, planes[0], planes[1], planes[2], planes[3]);
    }
    if (outside > 0) {
      rec.status = F3D_SUBSET_OUTSIDE;
      return rec;
    }
    const double sum_g = window_sum(n, [&](int i) { return g[i]; });
    if (sum_g != sum_g) {
      rec.status = F3D_SUBSET_NAN;
      return rec;
    }
    const double gm = sum_g / static_cast<double>(n);
    for (int i = 0; i < n; ++i) G[i] = g[i] - gm;
    const double dg = std::sqrt(window_sum(n, [&](int i) { return G[i] * G[i]; }));
    const double fg = window_sum(n, [&](int i) { return F[i] * G[i]; });
    rec.dg = dg;
    if (dg == 0.0) {
      rec.status = F3D_SUBSET_FLAT_TARGET;
      return rec;
    }
    rec.zncc = fg / (df * dg);
    // the step
    const double ratio = df / dg;
    double y[12], dp[12];
    for (int j = 0; j < m; ++j) {
      double v = window_sum(n, [&](int i) { return J[static_cast<size_t>(i) * m + j] * (F[i] - ratio * G[i]); });
      for (int q = 0; q < j; ++q) v -= L[j][q] * y[q];
      y[j] = v / L[j][j];
    }
    for (int j = m - 1; j >= 0; --j) {
      double v = y[j];
      for (int q = j + 1; q < m; ++q) v -= L[q][j] * y[q];
      y[j] = v / L[j][j];
    }
    for (int k = 0; k < 12; ++k) dp[k] = 0.0;
    for (int k = 0; k < m; ++k) dp[m == 3 ? 4 * k : k] = -y[k];
    // the update
    double A[3][3], B[3][3], C[3][3], V[3][3], N[3][3];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) {
        A[r][k] = (r == k ? 1.0 : 0.0) + p[4 * r + 1 + k];
        B[r][k] = (r == k ? 1.0 : 0.0) + dp[4 * r + 1 + k];
      }
    C[0][0] = B[1][1] * B[2][2] - B[1][2] * B[2][1];
    C[0][1] = B[0][2] * B[2][1] - B[0][1] * B[2][2];
    C[0][2] = B[0][1] * B[1][2] - B[0][2] * B[1][1];
    C[1][0] = B[1][2] * B[2][0] - B[1][0] * B[2][2];
    C[1][1] = B[0][0] * B[2][2] - B[0][2] * B[2][0];
    C[1][2] = B[0][2] * B[1][0] - B[0][0] * B[1][2];
    C[2][0] = B[1][0] * B[2][1] - B[1][1] * B[2][0];
    C[2][1] = B[0][1] * B[2][0] - B[0][0] * B[2][1];
    C[2][2] = B[0][0] * B[1][1] - B[0][1] * B[1][0];
    const double det = (B[0][0] * C[0][0] + B[0][1] * C[1][0]) + B[0][2] * C[2][0];
    if (det == 0.0) {
      rec.status = F3D_SUBSET_SINGULAR;
      return rec;
    }
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) V[r][k] = C[r][k] / det;
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) N[r][k] = (A[r][0] * V[0][k] + A[r][1] * V[1][k]) + A[r][2] * V[2][k];
    for (int r = 0; r < 3; ++r) {
      p[4 * r] = p[4 * r] - ((N[r][0] * dp[0] + N[r][1] * dp[4]) + N[r][2] * dp[8]);
      for (int k = 0; k < 3; ++k) p[4 * r + 1 + k] = N[r][k] - (r == k ? 1.0 : 0.0);
    }
    // the stop
    double grads = 0.0;
    for (int k = 0; k < 12; ++k)
      if (k % 4) grads += dp[k] * dp[k];
    const double ww = static_cast<double>(W) * static_cast<double>(W);
    rec.step = std::sqrt(((dp[0] * dp[0] + dp[4] * dp[4]) + dp[8] * dp[8]) + ww * grads);
    const double du = p[0] - u0, dv = p[4] - v0, dw = p[8] - w0;
    if (rec.step < tolerance) {
      rec.status = F3D_SUBSET_OK;
      return rec;
    }
    if (std::sqrt((du * du + dv * dv) + dw * dw) > reach) {
      rec.status = F3D_SUBSET_LOST;
      return rec;
    }
    if (rec.iterations == max_iterations) {
      rec.status = F3D_SUBSET_NOT_CONVERGED;
      return rec;
    }
  }
}

}  // namespace

extern "C" int f3d_subset_match(f3d_devptr a, f3d_devptr b, size_t width, size_t height, size_t depth, const f3d_subset_match_grid* grid,
                                int model, const double* start, int max_iterations, double tolerance, double reach,
                                f3d_subset_match_record* records, f3d_subset_match_info* info)
{
  Box box;
  if (!a || !b || !grid || !records) return 1;
  if (model != F3D_SUBSET_TRANSLATION && model != F3D_SUBSET_AFFINE) return 1;
  const f3d_subset_match_grid& q = *grid;
  if (q.step < 1 || q.nx < 1 || q.ny < 1 || q.nz < 1) return 1;
  const unsigned long long count = static_cast<unsigned long long>(q.nx) * q.ny * q.nz;
  if (count > F3D_SUBSET_MATCH_MAX_NODES || q.window < 1 || q.window > F3D_SUBSET_MATCH_MAX_WINDOW) return 1;
  if (max_iterations < 1 || max_iterations > F3D_SUBSET_MATCH_MAX_ITERATIONS || !(tolerance > 0.0) || !(reach > 0.0)) return 1;
  if (!geometry(width, height, depth, &box)) return 1;
  const long long first[3] = {q.ox, q.oy, q.oz}, counts[3] = {q.nx, q.ny, q.nz};
  const long long dims[3] = {static_cast<long long>(width), static_cast<long long>(height), static_cast<long long>(depth)};
  for (int axis = 0; axis < 3; ++axis)
    if (first[axis] - q.window - 1 < 0 || first[axis] + (counts[axis] - 1) * q.step + q.window + 1 > dims[axis] - 1) return 1;
  const float* fa = reinterpret_cast<const float*>(static_cast<uintptr_t>(a));
  const float* fb = reinterpret_cast<const float*>(static_cast<uintptr_t>(b));
  std::vector<f3d_subset_match_record> found(count);
  size_t node = 0;
  for (int k = 0; k < q.nz; ++k)
    for (int j = 0; j < q.ny; ++j)
      for (int i = 0; i < q.nx; ++i, ++node) {
        const long long c[3] = {q.ox + static_cast<long long>(i) * q.step, q.oy + static_cast<long long>(j) * q.step,
                                q.oz + static_cast<long long>(k) * q.step};
        found[node] = node_record(fa, fb, box, c, q.window, model == F3D_SUBSET_AFFINE ? 12 : 3, start ? start + 12 * node : nullptr,
                                  max_iterations, tolerance, reach);
      }
  std::memcpy(records, found.data(), count * sizeof(f3d_subset_match_record));
  if (info) {
    f3d_subset_match_info t = {};
    t.nodes = count;
    for (const f3d_subset_match_record& r : found) {
      t.status[r.status] += 1;
      t.iterations += static_cast<unsigned long long>(r.iterations);
      t.nan += static_cast<unsigned long long>(r.nan);
    }
    *info = t;
  }
  return 0;
}
