// The per-voxel displacement gradient and Green-Lagrange tensor that f3d_flow_strain (f3d_strain.hip) and f3d_principal_strain
// (f3d_principal.hip) both form: the samples of a displacement, the missing-sample rules of a column of G, the six components of
// E in include/f3d.h's evaluation order, and the wave reductions of their statistics.  Everything here is inlined into its kernel.
#ifndef F3D_STRAIN_GRAD_H_
#define F3D_STRAIN_GRAD_H_
#include "f3d_internal.h"

namespace f3d_strain {

struct Sample {
  float u, v, w;
};

__device__ __forceinline__ bool present(const Sample& s) { return !(isnan(s.u) || isnan(s.v) || isnan(s.w)); }

__device__ __forceinline__ Sample load(const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ w,
                                       size_t i, bool in)
{
  const float nan = __builtin_nanf("");
  Sample s = {nan, nan, nan};
  if (in) {
    s.u = u[i];
    s.v = v[i];
    s.w = w[i];
  }
  return s;
}

// column a of G from the samples at p - e_a (m), p (c) and p + e_a (q); n1: the axis has size 1; false when neither neighbour exists
__device__ __forceinline__ bool column(const Sample& m, const Sample& c, const Sample& q, bool n1, float& g0, float& g1, float& g2)
{
  if (n1) {
    g0 = g1 = g2 = 0.f;
    return true;
  }
  const bool hm = present(m), hq = present(q);
  if (hm && hq) {
    g0 = (q.u - m.u) * 0.5f;
    g1 = (q.v - m.v) * 0.5f;
    g2 = (q.w - m.w) * 0.5f;
  } else if (hq) {
    g0 = q.u - c.u;
    g1 = q.v - c.v;
    g2 = q.w - c.w;
  } else if (hm) {
    g0 = c.u - m.u;
    g1 = c.v - m.v;
    g2 = c.w - m.w;
  } else {
    return false;
  }
  return true;
}

// E = 1/2 (F^T F - I) of G[r][c] = d(component r) / d(axis c); include/f3d.h, f3d_flow_strain: the evaluation order is part of the
// ABI (contraction is off in this build)
__device__ __forceinline__ void green_lagrange(float G00, float G01, float G02, float G10, float G11, float G12, float G20,
                                               float G21, float G22, float& exx, float& eyy, float& ezz, float& exy, float& exz,
                                               float& eyz)
{
  exx = 0.5f * ((G00 + G00) + ((G00 * G00 + G10 * G10) + G20 * G20));
  eyy = 0.5f * ((G11 + G11) + ((G01 * G01 + G11 * G11) + G21 * G21));
  ezz = 0.5f * ((G22 + G22) + ((G02 * G02 + G12 * G12) + G22 * G22));
  exy = 0.5f * ((G01 + G10) + ((G00 * G01 + G10 * G11) + G20 * G21));
  exz = 0.5f * ((G02 + G20) + ((G00 * G02 + G10 * G12) + G20 * G22));
  eyz = 0.5f * ((G12 + G21) + ((G01 * G02 + G11 * G12) + G21 * G22));
}

__device__ __forceinline__ float wave_min(float x)
{
  for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float wave_max(float x)
{
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ double wave_sum(double x)
{
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x)
{
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

}  // namespace f3d_strain
#endif  // F3D_STRAIN_GRAD_H_
