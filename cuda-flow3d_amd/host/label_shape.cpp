// include/f3d_host.h, f3d_label_shape_solve: the definition and the order of evaluation stand there.  Every operation is rounded on
// its own (the host library is built with -ffp-contract=off).
#include "label_shape.h"

#include <cmath>

namespace {

const double kPi = 3.14159265358979323846;
// the share of the unit sphere nearest to +-d_k among the 26 directions: axes, face diagonals, body diagonals
const double kAxisWeight = 0.0915557824, kFaceWeight = 0.0739612557, kBodyWeight = 0.0703912796;

// A <- J^T A J and V <- V J for the rotation in the (p, q) plane that annihilates A[p][q]
void Rotate(double A[3][3], double V[3][3], int p, int q)
{
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
  const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
  for (int k = 0; k < 3; ++k) {  // columns p and q
    const double akp = A[k][p], akq = A[k][q];
    A[k][p] = c * akp - s * akq;
    A[k][q] = s * akp + c * akq;
  }
  for (int k = 0; k < 3; ++k) {  // rows p and q
    const double apk = A[p][k], aqk = A[q][k];
    A[p][k] = c * apk - s * aqk;
    A[q][k] = s * apk + c * aqk;
  }
  A[p][q] = A[q][p] = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][p], vkq = V[k][q];
    V[k][p] = c * vkp - s * vkq;
    V[k][q] = s * vkp + c * vkq;
  }
}

}  // namespace

void LabelShapeAxes(const double c[6], double values[3], double axes[9])
{
  double A[3][3] = {{c[0], c[3], c[4]}, {c[3], c[1], c[5]}, {c[4], c[5], c[2]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < kLabelShapeSweeps; ++sweep) {
    Rotate(A, V, 0, 1);
    Rotate(A, V, 0, 2);
    Rotate(A, V, 1, 2);
  }
  // descending, equal values in the order of their columns (a stable insertion sort of three)
  int order[3] = {0, 1, 2};
  for (int i = 1; i < 3; ++i)
    for (int j = i; j > 0 && A[order[j]][order[j]] > A[order[j - 1]][order[j - 1]]; --j) {
      const int held = order[j];
      order[j] = order[j - 1];
      order[j - 1] = held;
    }
  for (int i = 0; i < 3; ++i) {
    const int col = order[i];
    values[i] = A[col][col];
    double v[3] = {V[0][col], V[1][col], V[2][col]};
    const double norm = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    int big = 0;  // the component of largest magnitude, the first on ties
    for (int a = 1; a < 3; ++a)
      if (std::fabs(v[a]) > std::fabs(v[big])) big = a;
    const double sign = v[big] < 0.0 ? -1.0 : 1.0;
    for (int a = 0; a < 3; ++a) axes[3 * i + a] = sign * v[a] / norm;
  }
}

void SolveLabelShapes(const struct f3d_label_shape_sums* sums, size_t n_labels, f3d_label_shape* out)
{
  const double nan = std::nan("");
  const double root2 = std::sqrt(2.0), root3 = std::sqrt(3.0);
  for (size_t l = 0; l < n_labels; ++l) {
    const struct f3d_label_shape_sums& s = sums[l];
    f3d_label_shape r = {};
    r.voxels = s.n;
    for (int i = 0; i < 3; ++i) {
      r.box_lo[i] = s.lo[i];
      r.box_hi[i] = s.hi[i];
      r.border[i] = s.border[i];
    }
    if (s.n == 0) {
      r.status = F3D_LABEL_EMPTY;
      for (int i = 0; i < 3; ++i) r.centroid[i] = r.semi_axes[i] = nan;
      for (int i = 0; i < 9; ++i) r.axes[i] = nan;
      r.diameter = r.surface = r.sphericity = nan;
      out[l] = r;
      continue;
    }
    r.status = F3D_LABEL_OK;
    const double n = static_cast<double>(s.n);
    for (int i = 0; i < 3; ++i) r.centroid[i] = static_cast<double>(s.s1[i]) / n;
    r.diameter = std::cbrt(6.0 * n / kPi);
    // n s2_ik - s1_i s1_k exactly (below 2^93), rounded to binary64 once
    static const int kI[6] = {0, 1, 2, 0, 0, 1}, kK[6] = {0, 1, 2, 1, 2, 2};
    const double nn = n * n;
    double cov[6];
    for (int j = 0; j < 6; ++j) {
      const __int128 m = static_cast<__int128>(s.n) * static_cast<__int128>(s.s2[j]) -
                         static_cast<__int128>(s.s1[kI[j]]) * static_cast<__int128>(s.s1[kK[j]]);
      cov[j] = static_cast<double>(m) / nn;
      if (j < 3) cov[j] = cov[j] + 1.0 / 12.0;
    }
    double values[3];
    LabelShapeAxes(cov, values, r.axes);
    for (int i = 0; i < 3; ++i) r.semi_axes[i] = std::sqrt(5.0 * values[i]);
    r.faces = 0;
    double crofton = 0.0;
    for (int k = 0; k < 13; ++k) {
      const unsigned long long open = 2 * (s.n - s.pairs[k]);
      if (k < 3) r.faces += open;
      const double weight = k < 3 ? kAxisWeight : (k < 9 ? kFaceWeight : kBodyWeight);
      const double length = k < 3 ? 1.0 : (k < 9 ? root2 : root3);
      crofton = crofton + weight * static_cast<double>(open) / length;
    }
    r.surface = 2.0 * crofton;
    const double six_n = 6.0 * n;
    r.sphericity = std::cbrt(kPi * (six_n * six_n)) / r.surface;
    r.euler = static_cast<long long>(s.n) - static_cast<long long>(s.pairs[0] + s.pairs[1] + s.pairs[2]) +
              static_cast<long long>(s.squares[0] + s.squares[1] + s.squares[2]) - static_cast<long long>(s.cubes);
    out[l] = r;
  }
}
