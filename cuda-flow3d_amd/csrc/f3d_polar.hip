// Polar decomposition F = R U of the local deformation gradient of a displacement for gfx950: per voxel the gradient G and the
// Green-Lagrange tensor E of f3d_flow_strain (same missing-sample rules, same expressions: f3d_strain_grad.h), diagonalised by the five
// Jacobi sweeps of f3d_principal_strain (f3d_jacobi3.h); the principal stretches are the square roots of the eigenvalues 2 e_i + 1 of
// C = F^T F, and R = F U^-1 with U^-1 = V diag(1 / lambda) V^T gives the rotation angle and the rotation vector.  The definition and
// the evaluation order are those of include/f3d.h (f3d_polar_decomposition); tests/polar_ref.py restates them in float32 numpy and
// matches the kernel bit for bit.
//
// Shape: k_principal_strain's (a wave on 64 consecutive x of one row, a workgroup kBY rows, a register march in z over kZ planes, the
// x neighbours by __shfl, full-row stores, the ballot exit from the sweep loop).  Lanes outside the volume, lanes of undefined voxels
// and lanes whose vol already says folded diagonalise the zero matrix and never hold their wave back.  ROT = false serves a selection
// of the stretches alone without statistics: it carries no V and skips R, the angle and the vector.  The statistics hold the angle,
// so a call that asks for them runs ROT = true whatever it stores.
//
// Statistics (optional): one partial per workgroup, folded in a fixed order by a one-workgroup kernel (f3d_partials.h).
#include "f3d_jacobi3.h"
#include "f3d_strain_grad.h"

namespace {

using namespace f3d_strain;
using namespace f3d_partials;

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

template <bool STATS, bool ROT>
__global__ __launch_bounds__(kBX* kBY) void k_polar(const float* __restrict__ du, const float* __restrict__ dv,
                                                    const float* __restrict__ dw, PolarOut out, F3dGeo g,
                                                    PolarPartial* __restrict__ partials)
{
  const float nan = __builtin_nanf("");
  PolarPartial sum = PolarPartial::identity();  // this lane's voxels

  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  Column own;
  march_prime(du, dv, dw, g, z_begin, own);
  for (int z = z_begin; z < z_end; ++z) {
    Gradient G;
    const bool def = march_step(du, dv, dw, g, z, z_end, own, G);
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

    if (march_owns(g)) {
      const size_t i = own.row + march_x();
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
    march_advance(own);
  }

  if (STATS) {
    sum.defined = wave_sum(sum.defined);
    sum.folded = wave_sum(sum.folded);
    sum.theta_max = wave_max(sum.theta_max);
    sum.l1_max = wave_max(sum.l1_max);
    sum.l3_min = wave_min(sum.l3_min);
    sum.theta_sum = wave_sum(sum.theta_sum);
    block_partial<PolarPartial, kBY>(sum, partials);
  }
}

}  // namespace

extern "C" {

int f3d_polar_decomposition(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[7], unsigned fields, size_t width,
                            size_t height, size_t depth, f3d_polar_stats* stats)
{
  F3D_REQUIRE_READY("f3d_polar_decomposition");
  if (!u || !v || !w) return f3d::fail("f3d_polar_decomposition: null input");
  const unsigned all = F3D_POLAR_ANGLE | F3D_POLAR_VECTOR | F3D_POLAR_STRETCH;
  if (fields == 0 || (fields & ~all))
    return f3d::fail("f3d_polar_decomposition: fields must be a non-empty combination of F3D_POLAR_ANGLE, F3D_POLAR_VECTOR, "
                     "F3D_POLAR_STRETCH (got %u)", fields);
  if (!out) return f3d::fail("f3d_polar_decomposition: null output array");
  static const char* const names[7] = {"theta", "rx", "ry", "rz", "l1", "l2", "l3"};
  static const unsigned groups[7] = {F3D_POLAR_ANGLE,   F3D_POLAR_VECTOR,  F3D_POLAR_VECTOR, F3D_POLAR_VECTOR,
                                     F3D_POLAR_STRETCH, F3D_POLAR_STRETCH, F3D_POLAR_STRETCH};
  PolarOut o;
  if (!f3d::select_outputs("f3d_polar_decomposition", "the stencil reads neighbours", o.f, out, 7, names, groups, fields, u, v, w))
    return 1;
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_polar_decomposition")) return 1;
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ);
  if (!stats) {
    if (fields & (F3D_POLAR_ANGLE | F3D_POLAR_VECTOR))
      hipLaunchKernelGGL((k_polar<false, true>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, o, g, nullptr);
    else
      hipLaunchKernelGGL((k_polar<false, false>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, o, g, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  PolarPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](PolarPartial* d_part) {
        hipLaunchKernelGGL((k_polar<true, true>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, o, g, d_part);
      }))
    return 1;
  stats->defined = r.defined;
  stats->folded = r.folded;
  stats->theta_max = r.defined ? r.theta_max : __builtin_nanf("");
  stats->l1_max = r.defined ? r.l1_max : __builtin_nanf("");
  stats->l3_min = r.defined ? r.l3_min : __builtin_nanf("");
  stats->theta_sum = r.theta_sum;
  return 0;
}

}  // extern "C"
