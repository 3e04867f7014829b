// What follows the gradient in f3d_principal_strain (f3d_principal.hip), f3d_polar_decomposition (f3d_polar.hip) and their
// from-gradient entries (f3d_from_gradient.hip): from the G of one voxel and whether it is defined, rules 2-4 of
// f3d_principal_strain and rules 1 (vol, E) - 6 of f3d_polar_decomposition in include/f3d.h, the stores and the lane's statistics,
// then the wave / workgroup reduction and the host's reading of the folded partial.  One text, inlined into every kernel, so a
// gradient gives the same bits whichever kernel formed it.
//
// Everything is in an anonymous namespace ON PURPOSE: each translation unit gets partial types of its own, so the
// fold_partials<P> kernels of two units stay two kernels instead of one template instantiation registered from two code objects.
#ifndef F3D_TENSOR_TAIL_H_
#define F3D_TENSOR_TAIL_H_
#include "f3d_jacobi3.h"
#include "f3d_strain_grad.h"

namespace {

using namespace f3d_strain;
using namespace f3d_partials;

// ---- principal strains ---------------------------------------------------------------------------------------------------------

struct PrincipalPartial {
  unsigned long long defined;
  float e1_max, e3_min, shear_max, pad;

  static __device__ __forceinline__ PrincipalPartial identity() { return {0ull, -INFINITY, INFINITY, -INFINITY, 0.f}; }
  __device__ __forceinline__ void merge(const PrincipalPartial& q)
  {
    defined += q.defined;
    e1_max = fmaxf(e1_max, q.e1_max);
    e3_min = fminf(e3_min, q.e3_min);
    shear_max = fmaxf(shear_max, q.shear_max);
  }
};

struct PrincipalOut {
  float* f[10];  // e1, e2, e3, gmax, d1x, d1y, d1z, d3x, d3y, d3z (null = not stored)
};

// rule 3: value and column exchanged together when the first is strictly smaller
template <bool DIRS>
__device__ __forceinline__ void order(float& li, float& lj, float (&vi)[3], float (&vj)[3])
{
  if (li < lj) {
    const float l = li;
    li = lj;
    lj = l;
    if (DIRS) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float x = vi[k];
        vi[k] = vj[k];
        vj[k] = x;
      }
    }
  }
}

// rule 4: the component of largest magnitude (the first of x, y, z among equals) is made non-negative
__device__ __forceinline__ void fix_sign(float (&d)[3])
{
  float lead = d[0];
  if (fabsf(d[1]) > fabsf(lead)) lead = d[1];
  if (fabsf(d[2]) > fabsf(lead)) lead = d[2];
  if (lead < 0.f) {
    d[0] = -d[0];
    d[1] = -d[1];
    d[2] = -d[2];
  }
}

// One voxel of f3d_principal_strain from its gradient: def = the voxel is defined (G is not read as a number otherwise), owns = the
// lane has a voxel to store at index i.  Every lane of the wave calls it (the sweeps ballot).
template <bool STATS, bool DIRS>
__device__ __forceinline__ void principal_voxel(const Gradient& G, bool def, bool owns, size_t i, const PrincipalOut& out,
                                                PrincipalPartial& sum)
{
  const float nan = __builtin_nanf("");
  const auto& [G00, G01, G02, G10, G11, G12, G20, G21, G22] = G;

  float a00, a11, a22, a01, a02, a12;
  green_lagrange(G00, G01, G02, G10, G11, G12, G20, G21, G22, a00, a11, a22, a01, a02, a12);
  if (!def) a00 = a11 = a22 = a01 = a02 = a12 = 0.f;  // NaN in every output below; nothing to rotate meanwhile
  float v0[3] = {1.f, 0.f, 0.f}, v1[3] = {0.f, 1.f, 0.f}, v2[3] = {0.f, 0.f, 1.f};  // the columns of V

  f3d_jacobi3::sweeps<DIRS>(a00, a11, a22, a01, a02, a12, v0, v1, v2);  // rule 2

  order<DIRS>(a00, a11, v0, v1);
  order<DIRS>(a00, a22, v0, v2);
  order<DIRS>(a11, a22, v1, v2);
  float e1 = a00, e2 = a11, e3 = a22;
  float gmax = 0.5f * (e1 - e3);
  if (DIRS) {
    fix_sign(v0);
    fix_sign(v2);
  }
  if (!def) {
    e1 = e2 = e3 = gmax = nan;
    v0[0] = v0[1] = v0[2] = v2[0] = v2[1] = v2[2] = nan;
  }

  if (owns) {
    if (out.f[0]) out.f[0][i] = e1;
    if (out.f[1]) out.f[1][i] = e2;
    if (out.f[2]) out.f[2][i] = e3;
    if (out.f[3]) out.f[3][i] = gmax;
    if (DIRS) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (out.f[4 + k]) out.f[4 + k][i] = v0[k];
        if (out.f[7 + k]) out.f[7 + k][i] = v2[k];
      }
    }
  }
  if (STATS && !isnan(e1)) {
    ++sum.defined;
    sum.e1_max = fmaxf(sum.e1_max, e1);
    sum.e3_min = fminf(sum.e3_min, e3);
    sum.shear_max = fmaxf(sum.shear_max, gmax);
  }
}

// the lanes' sums into the workgroup's partial; every thread of a (kBX, kBY) workgroup calls it
__device__ __forceinline__ void principal_partial(PrincipalPartial& sum, PrincipalPartial* __restrict__ partials)
{
  sum.defined = wave_sum(sum.defined);
  sum.e1_max = wave_max(sum.e1_max);
  sum.e3_min = wave_min(sum.e3_min);
  sum.shear_max = wave_max(sum.shear_max);
  block_partial<PrincipalPartial, kBY>(sum, partials);
}

inline void principal_stats_of(const PrincipalPartial& r, f3d_principal_stats* stats)
{
  stats->defined = r.defined;
  stats->e1_max = r.defined ? r.e1_max : __builtin_nanf("");
  stats->e3_min = r.defined ? r.e3_min : __builtin_nanf("");
  stats->shear_max = r.defined ? r.shear_max : __builtin_nanf("");
}

// ---- polar decomposition -------------------------------------------------------------------------------------------------------

struct PolarPartial {
  unsigned long long defined, folded;
  float theta_max, l1_max, l3_min, pad;
  double theta_sum;

  static __device__ __forceinline__ PolarPartial identity() { return {0ull, 0ull, -INFINITY, -INFINITY, INFINITY, 0.f, 0.0}; }
  __device__ __forceinline__ void merge(const PolarPartial& q)
  {
    defined += q.defined;
    folded += q.folded;
    theta_max = fmaxf(theta_max, q.theta_max);
    l1_max = fmaxf(l1_max, q.l1_max);
    l3_min = fminf(l3_min, q.l3_min);
    theta_sum += q.theta_sum;
  }
};

struct PolarOut {
  float* f[7];  // theta, rx, ry, rz, l1, l2, l3 (null = not stored)
};

// include/f3d.h, f3d_polar_decomposition, rule 3: the values exchanged when the first is strictly smaller
__device__ __forceinline__ void order(float& li, float& lj)
{
  if (li < lj) {
    const float l = li;
    li = lj;
    lj = l;
  }
}

// rule 6: the angle of (c, s), s >= 0, in [0, pi] from + - * / and sqrt alone
__device__ __forceinline__ float atan2_pos(float s, float c)
{
  constexpr float k3 = 1.f / 3.f, k5 = 1.f / 5.f, k7 = 1.f / 7.f, k9 = 1.f / 9.f;  // each the float32 nearest to the fraction
  constexpr float pi = 3.14159274101257324f, half_pi = 1.57079637050628662f;      // 0x40490FDB, 0x3FC90FDB
  const bool big = fabsf(c) >= s;
  float x = big ? s / c : c / s;
  if (s == 0.f && c == 0.f) x = 0.f;
  x = x / (1.f + sqrtf(x * x + 1.f));
  x = x / (1.f + sqrtf(x * x + 1.f));
  const float z = x * x;
  const float p = (((z * k9 - k7) * z + k5) * z - k3) * z + 1.f;
  const float t = 4.f * (x * p);
  return big ? (c > 0.f ? t : pi + t) : half_pi - t;
}

// One voxel of f3d_polar_decomposition from its gradient; def, owns and i as in principal_voxel.  ROT = false carries no V and
// skips R, the angle and the vector (a selection of the stretches alone without statistics).
template <bool STATS, bool ROT>
__device__ __forceinline__ void polar_voxel(const Gradient& G, bool def, bool owns, size_t i, const PolarOut& out, PolarPartial& sum)
{
  const float nan = __builtin_nanf("");
  const auto& [G00, G01, G02, G10, G11, G12, G20, G21, G22] = G;

  // rule 1: vol and E by f3d_flow_strain's expressions
  const float I1 = (G00 + G11) + G22;
  const float I2 = ((G00 * G11 - G01 * G10) + (G11 * G22 - G12 * G21)) + (G00 * G22 - G02 * G20);
  const float I3 = (G00 * (G11 * G22 - G12 * G21) - G01 * (G10 * G22 - G12 * G20)) + G02 * (G10 * G21 - G11 * G20);
  const float vol = (I1 + I2) + I3;
  float a00, a11, a22, a01, a02, a12;
  green_lagrange(G00, G01, G02, G10, G11, G12, G20, G21, G22, a00, a11, a22, a01, a02, a12);
  bool folded = def && vol <= -1.f;
  if (!def || folded) a00 = a11 = a22 = a01 = a02 = a12 = 0.f;  // NaN in every output below; nothing to rotate meanwhile
  float v0[3] = {1.f, 0.f, 0.f}, v1[3] = {0.f, 1.f, 0.f}, v2[3] = {0.f, 0.f, 1.f};  // the columns of V

  f3d_jacobi3::sweeps<ROT>(a00, a11, a22, a01, a02, a12, v0, v1, v2);  // rule 2

  // rule 3: the eigenvalues of C = F^T F, the folded voxels, the stretches
  const float m0 = 2.f * a00 + 1.f, m1 = 2.f * a11 + 1.f, m2 = 2.f * a22 + 1.f;
  folded = folded || (def && (!(m0 > 0.f) || !(m1 > 0.f) || !(m2 > 0.f)));
  const bool good = def && !folded;
  const float s0 = sqrtf(m0), s1 = sqrtf(m1), s2 = sqrtf(m2);
  float l1 = s0, l2 = s1, l3 = s2;
  order(l1, l2);
  order(l1, l3);
  order(l2, l3);

  float theta = 0.f, rx = 0.f, ry = 0.f, rz = 0.f;
  if (ROT) {
    // rule 4: U^-1 = V diag(q) V^T entry by entry, R = (I + G) U^-1
    const float q0 = 1.f / s0, q1 = 1.f / s1, q2 = 1.f / s2;
    float ui[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) ui[r][c] = ((v0[r] * q0) * v0[c] + (v1[r] * q1) * v1[c]) + (v2[r] * q2) * v2[c];
    const float fm[3][3] = {{G00 + 1.f, G01, G02}, {G10, G11 + 1.f, G12}, {G20, G21, G22 + 1.f}};
    float R[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[r][c] = (fm[r][0] * ui[0][c] + fm[r][1] * ui[1][c]) + fm[r][2] * ui[2][c];
    // rule 5: the angle from the trace and the skew part, the rotation vector along the skew part
    const float cs = 0.5f * (((R[0][0] + R[1][1]) + R[2][2]) - 1.f);
    const float ax = 0.5f * (R[2][1] - R[1][2]), ay = 0.5f * (R[0][2] - R[2][0]), az = 0.5f * (R[1][0] - R[0][1]);
    const float sn = sqrtf((ax * ax + ay * ay) + az * az);
    theta = atan2_pos(sn, cs);
    const float k = theta / sn;
    rx = k * ax;
    ry = k * ay;
    rz = k * az;
    if (sn == 0.f) rx = ry = rz = 0.f;
  }
  if (!good) theta = rx = ry = rz = l1 = l2 = l3 = nan;

  if (owns) {
    if (ROT) {
      if (out.f[0]) out.f[0][i] = theta;
      if (out.f[1]) out.f[1][i] = rx;
      if (out.f[2]) out.f[2][i] = ry;
      if (out.f[3]) out.f[3][i] = rz;
    }
    if (out.f[4]) out.f[4][i] = l1;
    if (out.f[5]) out.f[5][i] = l2;
    if (out.f[6]) out.f[6][i] = l3;
  }
  if (STATS) {
    sum.folded += folded ? 1 : 0;
    if (good) {
      ++sum.defined;
      sum.theta_max = fmaxf(sum.theta_max, theta);
      sum.l1_max = fmaxf(sum.l1_max, l1);
      sum.l3_min = fminf(sum.l3_min, l3);
      sum.theta_sum += static_cast<double>(theta);
    }
  }
}

// the lanes' sums into the workgroup's partial; every thread of a (kBX, kBY) workgroup calls it
__device__ __forceinline__ void polar_partial(PolarPartial& sum, PolarPartial* __restrict__ partials)
{
  sum.defined = wave_sum(sum.defined);
  sum.folded = wave_sum(sum.folded);
  sum.theta_max = wave_max(sum.theta_max);
  sum.l1_max = wave_max(sum.l1_max);
  sum.l3_min = wave_min(sum.l3_min);
  sum.theta_sum = wave_sum(sum.theta_sum);
  block_partial<PolarPartial, kBY>(sum, partials);
}

inline void polar_stats_of(const PolarPartial& r, f3d_polar_stats* stats)
{
  stats->defined = r.defined;
  stats->folded = r.folded;
  stats->theta_max = r.defined ? r.theta_max : __builtin_nanf("");
  stats->l1_max = r.defined ? r.l1_max : __builtin_nanf("");
  stats->l3_min = r.defined ? r.l3_min : __builtin_nanf("");
  stats->theta_sum = r.theta_sum;
}

}  // namespace
#endif  // F3D_TENSOR_TAIL_H_
