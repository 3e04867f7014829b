// include/f3d_host.h, f3d_motion_solve: the definition stands there.
#include "motion_fit.h"

#include <algorithm>
#include <cmath>

namespace {

// Sxx is stored xx yy zz xy xz yz
int Sym(int i, int k)
{
  static const int at[3][3] = {{0, 3, 4}, {3, 1, 5}, {4, 5, 2}};
  return at[i][k];
}

bool Fail(std::string* error, const char* what)
{
  if (error) *error = std::string("f3d_motion_solve: ") + what;
  return false;
}

// least squares of d ~ t + M X from the normal equations [[n, Sx^T], [Sx, Sxx]] (t_j, M_j0, M_j1, M_j2) = (Sd_j, Sxd_0j, Sxd_1j, Sxd_2j)
bool SolveAffine(const struct f3d_motion_sums& s, double t[3], double M[9], std::string* error)
{
  // an axis along which every present voxel has the same coordinate: n Sxx_aa == Sx_a^2 in the exact integers of doubled coordinates
  int axis[3], axes = 0;
  for (int a = 0; a < 3; ++a) {
    const __int128 xx4 = static_cast<__int128>(4.0 * s.Sxx[a]), x2 = static_cast<__int128>(2.0 * s.Sx[a]);
    if (static_cast<__int128>(s.n) * xx4 != x2 * x2) axis[axes++] = a;
  }
  if (axes < 2) return Fail(error, "the present voxels are collinear: the affine model is not determined");
  const int k = axes + 1;
  double N[4][4], L[4][4] = {}, rhs[4][3];
  N[0][0] = static_cast<double>(s.n);
  for (int j = 0; j < 3; ++j) rhs[0][j] = s.Sd[j];
  for (int p = 0; p < axes; ++p) {
    N[0][p + 1] = N[p + 1][0] = s.Sx[axis[p]];
    for (int q = 0; q < axes; ++q) N[p + 1][q + 1] = s.Sxx[Sym(axis[p], axis[q])];
    for (int j = 0; j < 3; ++j) rhs[p + 1][j] = s.Sxd[3 * axis[p] + j];
  }
  // Cholesky N = L L^T; a pivot that is not above 2^-40 of its diagonal entry is the rounding noise of a singular matrix
  for (int i = 0; i < k; ++i) {
    for (int j = 0; j <= i; ++j) {
      double v = N[i][j];
      for (int m = 0; m < j; ++m) v -= L[i][m] * L[j][m];
      if (i == j) {
        if (!(v > 0x1p-40 * N[i][i])) return Fail(error, "the present voxels are coplanar: the affine model is not determined");
        L[i][i] = std::sqrt(v);
      } else {
        L[i][j] = v / L[j][j];
      }
    }
  }
  for (int j = 0; j < 3; ++j) {
    double y[4], x[4];
    for (int i = 0; i < k; ++i) {
      double v = rhs[i][j];
      for (int m = 0; m < i; ++m) v -= L[i][m] * y[m];
      y[i] = v / L[i][i];
    }
    for (int i = k - 1; i >= 0; --i) {
      double v = y[i];
      for (int m = i + 1; m < k; ++m) v -= L[m][i] * x[m];
      x[i] = v / L[i][i];
    }
    t[j] = x[0];
    for (int c = 0; c < 3; ++c) M[3 * j + c] = 0.0;
    for (int p = 0; p < axes; ++p) M[3 * j + axis[p]] = x[p + 1];
  }
  return true;
}

void Cross(const double a[3], const double b[3], double out[3])
{
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}

double Dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Kabsch: the rotation R that brings the centred X closest to the centred X + d
bool SolveRigid(const struct f3d_motion_sums& s, double t[3], double M[9], std::string* error)
{
  if (s.n < 3) return Fail(error, "fewer than three present voxels: the rigid model is not determined");
  const double n = static_cast<double>(s.n);
  // B = sum (y - ybar)(x - xbar)^T with y = x + d, i.e. the transpose of H = Cxx + Cxd; kept as its three columns
  double col[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};  // col[c][r] = B[r][c]; V[c] = column c of V
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) {
      const double cxx = s.Sxx[Sym(c, r)] - s.Sx[c] * s.Sx[r] / n;
      const double cxd = s.Sxd[3 * c + r] - s.Sx[c] * s.Sd[r] / n;
      col[c][r] = cxx + cxd;
    }
  // Jacobi eigen-decomposition of B^T B, carried out on the columns of B (one-sided, Hestenes): rotations of column pairs until
  // they are orthogonal.  B V = U S then holds with the singular values as column lengths, none of them squared.
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double alpha = Dot(col[p], col[p]), beta = Dot(col[q], col[q]), gamma = Dot(col[p], col[q]);
        if (gamma == 0.0 || std::fabs(gamma) <= 0x1p-53 * std::sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double tn = (zeta < 0 ? -1.0 : 1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / std::sqrt(1.0 + tn * tn), sn = cs * tn;
        for (int r = 0; r < 3; ++r) {
          const double gp = col[p][r], gq = col[q][r], vp = V[p][r], vq = V[q][r];
          col[p][r] = cs * gp - sn * gq;
          col[q][r] = sn * gp + cs * gq;
          V[p][r] = cs * vp - sn * vq;
          V[q][r] = sn * vp + cs * vq;
        }
      }
    if (!rotated) break;
  }
  double sv[3];
  int order[3] = {0, 1, 2};
  for (int c = 0; c < 3; ++c) sv[c] = std::sqrt(Dot(col[c], col[c]));
  std::sort(order, order + 3, [&](int a, int b) { return sv[a] > sv[b]; });
  const int a = order[0], b = order[1];
  if (!(sv[b] > 0x1p-40 * sv[a])) return Fail(error, "the present voxels are collinear: the rigid model is not determined");
  // U from the two largest columns, orthonormalised; the third column of U and of V by cross products, so that both are proper and
  // R = U V^T has determinant +1 whatever the sign of det B
  double u1[3], u2[3], u3[3], v3[3];
  for (int r = 0; r < 3; ++r) u1[r] = col[a][r] / sv[a];
  const double along = Dot(u1, col[b]);
  for (int r = 0; r < 3; ++r) u2[r] = col[b][r] - along * u1[r];
  const double len = std::sqrt(Dot(u2, u2));
  for (int r = 0; r < 3; ++r) u2[r] /= len;
  Cross(u1, u2, u3);
  Cross(V[a], V[b], v3);
  double R[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (u1[r] * V[a][c] + u2[r] * V[b][c]) + u3[r] * v3[c];
  for (int i = 0; i < 9; ++i) M[i] = R[i] - (i % 4 == 0 ? 1.0 : 0.0);
  for (int r = 0; r < 3; ++r) {
    const double xb[3] = {s.Sx[0] / n, s.Sx[1] / n, s.Sx[2] / n};
    t[r] = s.Sd[r] / n - ((M[3 * r] * xb[0] + M[3 * r + 1] * xb[1]) + M[3 * r + 2] * xb[2]);
  }
  return true;
}

}  // namespace

bool SolveMotion(const struct f3d_motion_sums& s, int model, f3d_motion_fit* fit, std::string* error)
{
  if (!fit) return Fail(error, "null fit");
  if (model != F3D_MOTION_TRANSLATION && model != F3D_MOTION_RIGID && model != F3D_MOTION_AFFINE)
    return Fail(error, "model must be F3D_MOTION_TRANSLATION, F3D_MOTION_RIGID or F3D_MOTION_AFFINE");
  if (s.n == 0) return Fail(error, "no voxel is present");
  const double n = static_cast<double>(s.n);
  double t[3] = {0, 0, 0}, M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (model == F3D_MOTION_TRANSLATION) {
    for (int j = 0; j < 3; ++j) t[j] = s.Sd[j] / n;
  } else if (model == F3D_MOTION_AFFINE) {
    if (!SolveAffine(s, t, M, error)) return false;
  } else if (!SolveRigid(s, t, M, error)) {
    return false;
  }
  for (int j = 0; j < 3; ++j) fit->t[j] = t[j];
  for (int i = 0; i < 9; ++i) fit->M[i] = M[i];
  fit->n = s.n;
  fit->rms_before = std::sqrt(((s.Sdd[0] + s.Sdd[1]) + s.Sdd[2]) / n);
  fit->model = model;
  fit->cos_angle = 0.0;
  fit->axial[0] = fit->axial[1] = fit->axial[2] = 0.0;
  if (model == F3D_MOTION_RIGID) {
    fit->cos_angle = (((M[0] + M[4]) + M[8]) + 2.0) / 2.0;  // (tr R - 1) / 2 with R = I + M
    fit->axial[0] = (M[7] - M[5]) / 2.0;
    fit->axial[1] = (M[2] - M[6]) / 2.0;
    fit->axial[2] = (M[3] - M[1]) / 2.0;
  }
  return true;
}

// include/f3d_host.h, f3d_motion_solve_labels: the definition stands there.
bool SolveLabelMotions(const struct f3d_motion_sums* sums, size_t n_labels, int model, unsigned long long min_voxels,
                       const double volume_centre[3], f3d_motion_fit* fits, int* status, std::string* error)
{
  if (model != F3D_MOTION_TRANSLATION && model != F3D_MOTION_RIGID && model != F3D_MOTION_AFFINE) {
    if (error) *error = "f3d_motion_solve_labels: model must be F3D_MOTION_TRANSLATION, F3D_MOTION_RIGID or F3D_MOTION_AFFINE";
    return false;
  }
  for (size_t l = 0; l < n_labels; ++l) {
    const struct f3d_motion_sums& s = sums[l];
    f3d_motion_fit fit = {};
    fit.n = s.n;
    fit.model = model;
    if (s.n == 0) {
      status[l] = F3D_LABEL_EMPTY;
    } else if (s.n < min_voxels) {
      status[l] = F3D_LABEL_SMALL;
    } else if (!SolveMotion(s, model, &fit, nullptr)) {
      status[l] = F3D_LABEL_DEGENERATE;
    } else {
      status[l] = F3D_LABEL_OK;
      const double n = static_cast<double>(s.n);
      const double xb[3] = {s.Sx[0] / n, s.Sx[1] / n, s.Sx[2] / n};
      for (int a = 0; a < 3; ++a) fit.centre[a] = volume_centre[a] + xb[a];
      for (int r = 0; r < 3; ++r) fit.t[r] = fit.t[r] + ((fit.M[3 * r] * xb[0] + fit.M[3 * r + 1] * xb[1]) + fit.M[3 * r + 2] * xb[2]);
    }
    fits[l] = fit;
  }
  return true;
}
