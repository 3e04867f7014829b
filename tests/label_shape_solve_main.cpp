// A stand-alone program around the host solve of the label shapes (cuda-flow3d_amd/host/label_shape.cpp), built by
// tests/test_label_shape_cpu.py with -fsanitize=address,undefined: blocks whose answers are known in closed form, an empty label, a
// label at the limits of the entry (2^31 - 1 voxels at coordinates up to 32767: the 128-bit products), and heap arrays whose every
// entry is written.  Prints "ok" and returns 0, or says what differs.
#include <cmath>
#include <cstdio>
#include <vector>

#include "label_shape.h"

namespace {

typedef struct f3d_label_shape_sums Sums;  // the entry of the same name hides the plain type name

int failures = 0;

void Expect(bool good, const char* what)
{
  if (good) return;
  std::printf("FAILED: %s\n", what);
  ++failures;
}

bool Near(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fabs(b); }

// the sums of the block [x0, x0 + a) x [y0, y0 + b) x [z0, z0 + c) inside a box that it does not touch
Sums Block(unsigned long long x0, unsigned long long y0, unsigned long long z0, unsigned long long a, unsigned long long b,
           unsigned long long c)
{
  Sums s = {};
  const unsigned long long lo[3] = {x0, y0, z0}, len[3] = {a, b, c};
  s.n = a * b * c;
  unsigned long long first[3], second[3];  // sum x and sum x^2 over one axis
  for (int i = 0; i < 3; ++i) {
    s.lo[i] = static_cast<long long>(lo[i]);
    s.hi[i] = static_cast<long long>(lo[i] + len[i] - 1);
    first[i] = second[i] = 0;
    for (unsigned long long x = lo[i]; x < lo[i] + len[i]; ++x) first[i] += x, second[i] += x * x;
    s.s1[i] = first[i] * (s.n / len[i]);
    s.s2[i] = second[i] * (s.n / len[i]);
  }
  s.s2[3] = first[0] * first[1] * c;
  s.s2[4] = first[0] * first[2] * b;
  s.s2[5] = first[1] * first[2] * a;
  const long long d[13][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, -1, 0}, {1, 0, 1}, {1, 0, -1},
                              {0, 1, 1}, {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};
  for (int k = 0; k < 13; ++k) {
    s.pairs[k] = 1;
    for (int i = 0; i < 3; ++i) s.pairs[k] *= len[i] - static_cast<unsigned long long>(d[k][i] < 0 ? -d[k][i] : d[k][i]);
  }
  s.squares[0] = (a - 1) * (b - 1) * c;
  s.squares[1] = (a - 1) * b * (c - 1);
  s.squares[2] = a * (b - 1) * (c - 1);
  s.cubes = (a - 1) * (b - 1) * (c - 1);
  return s;
}

}  // namespace

int main()
{
  std::vector<Sums> sums;
  sums.push_back(Block(3, 4, 5, 7, 5, 2));
  sums.push_back(Sums());  // no voxel
  sums.back().hi[0] = sums.back().hi[1] = sums.back().hi[2] = -1;
  sums.push_back(Block(1, 1, 1, 1, 1, 1));
  sums.push_back(Block(32768 - 2047, 32768 - 1024, 32768 - 1024, 2047, 1024, 1024));  // 2^31 - 2^20 voxels in the far corner
  std::vector<f3d_label_shape> out(sums.size());
  SolveLabelShapes(sums.data(), sums.size(), out.data());

  const f3d_label_shape& b = out[0];
  Expect(b.status == F3D_LABEL_OK && b.voxels == 70 && b.euler == 1, "block: status, voxels, euler");
  Expect(b.centroid[0] == 6.0 && b.centroid[1] == 6.0 && b.centroid[2] == 5.5, "block: centroid");
  Expect(b.faces == 2 * (7 * 5 + 7 * 2 + 5 * 2), "block: faces");
  Expect(Near(b.semi_axes[0], std::sqrt(5.0 * 49.0 / 12.0), 1e-14) && Near(b.semi_axes[1], std::sqrt(5.0 * 25.0 / 12.0), 1e-14) &&
             Near(b.semi_axes[2], std::sqrt(5.0 * 4.0 / 12.0), 1e-14),
         "block: semi-axes");
  Expect(b.axes[0] == 1.0 && b.axes[4] == 1.0 && b.axes[8] == 1.0, "block: axes along x, y, z");
  Expect(Near(b.diameter, std::cbrt(6.0 * 70.0 / 3.14159265358979323846), 1e-15), "block: diameter");
  Expect(b.surface > 0.0 && b.sphericity > 0.0 && b.sphericity < 1.0, "block: surface and sphericity");

  const f3d_label_shape& e = out[1];
  Expect(e.status == F3D_LABEL_EMPTY && e.voxels == 0 && e.box_lo[0] == 0 && e.box_hi[2] == -1 && e.faces == 0 && e.euler == 0,
         "empty: integers");
  Expect(std::isnan(e.centroid[1]) && std::isnan(e.diameter) && std::isnan(e.semi_axes[2]) && std::isnan(e.axes[8]) &&
             std::isnan(e.surface) && std::isnan(e.sphericity),
         "empty: doubles are NaN");

  const f3d_label_shape& v = out[2];
  Expect(v.voxels == 1 && v.euler == 1 && v.faces == 6 && v.centroid[0] == 1.0, "voxel: integers");
  Expect(Near(v.semi_axes[0], std::sqrt(5.0 / 12.0), 1e-15) && Near(v.semi_axes[2], std::sqrt(5.0 / 12.0), 1e-15), "voxel: semi-axes");
  // one voxel has 26 open ends: the weights sum to 1 over +-d, so surface = 2 * sum w_k * 2 / |d_k|
  Expect(Near(v.surface, 4.0 * (3 * 0.0915557824 + 6 * 0.0739612557 / std::sqrt(2.0) + 4 * 0.0703912796 / std::sqrt(3.0)), 1e-14),
         "voxel: surface");

  const f3d_label_shape& g = out[3];
  Expect(g.voxels == 2047ull * 1024 * 1024 && g.euler == 1, "corner block: voxels, euler");
  Expect(Near(g.centroid[0], 32768 - 2047 + 1023.0, 1e-15) && Near(g.centroid[2], 32768 - 1024 + 511.5, 1e-15), "corner block: centroid");
  Expect(Near(g.semi_axes[0], std::sqrt(5.0 * 2047.0 * 2047.0 / 12.0), 1e-12) &&
             Near(g.semi_axes[1], std::sqrt(5.0 * 1024.0 * 1024.0 / 12.0), 1e-12),
         "corner block: semi-axes without cancellation");

  // a rotated covariance: the axes are unit, orthogonal, signed by their largest component
  const double c[6] = {4.0, 3.0, 2.0, 1.0, 0.5, -0.25};
  double values[3], axes[9];
  LabelShapeAxes(c, values, axes);
  Expect(values[0] >= values[1] && values[1] >= values[2] && Near(values[0] + values[1] + values[2], 9.0, 1e-14), "axes: order and trace");
  for (int i = 0; i < 3; ++i) {
    const double* a = axes + 3 * i;
    int big = 0;
    for (int k = 1; k < 3; ++k)
      if (std::fabs(a[k]) > std::fabs(a[big])) big = k;
    Expect(a[big] > 0.0 && Near(a[0] * a[0] + a[1] * a[1] + a[2] * a[2], 1.0, 1e-14), "axes: unit and signed");
    const double* n = axes + 3 * ((i + 1) % 3);
    Expect(std::fabs(a[0] * n[0] + a[1] * n[1] + a[2] * n[2]) < 1e-14, "axes: orthogonal");
  }
  if (failures == 0) std::printf("ok\n");
  return failures ? 1 : 0;
}
