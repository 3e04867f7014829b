// The per-voxel displacement gradient and Green-Lagrange tensor that f3d_flow_strain (f3d_strain.hip) and f3d_principal_strain
// (f3d_principal.hip) both form: the samples of a displacement, the missing-sample rules of a column of G, the six components of
// E in include/f3d.h's evaluation order, and the march in z that gathers a voxel's neighbours.  Everything here is inlined into its
// kernel; the statistics of both go through f3d_partials.h.
#ifndef F3D_STRAIN_GRAD_H_
#define F3D_STRAIN_GRAD_H_
#include "f3d_internal.h"
#include "f3d_partials.h"

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

// The eight outputs vol, exx, eyy, ezz, exy, exz, eyz, eq of f3d_flow_strain from a gradient: the one text f3d_flow_strain and
// f3d_window_strain (f3d_window_strain.hip) both store.  include/f3d.h, f3d_flow_strain: the evaluation order is part of the ABI
// (contraction is off in this build)
__device__ __forceinline__ void strain_fields(float G00, float G01, float G02, float G10, float G11, float G12, float G20, float G21,
                                              float G22, float& vol, float& exx, float& eyy, float& ezz, float& exy, float& exz,
                                              float& eyz, float& eq)
{
  const float I1 = (G00 + G11) + G22;
  const float I2 = ((G00 * G11 - G01 * G10) + (G11 * G22 - G12 * G21)) + (G00 * G22 - G02 * G20);
  const float I3 = (G00 * (G11 * G22 - G12 * G21) - G01 * (G10 * G22 - G12 * G20)) + G02 * (G10 * G21 - G11 * G20);
  vol = (I1 + I2) + I3;
  green_lagrange(G00, G01, G02, G10, G11, G12, G20, G21, G22, exx, eyy, ezz, exy, exz, eyz);
  const float mean = ((exx + eyy) + ezz) / 3.f;
  const float a = exx - mean, b = eyy - mean, c = ezz - mean;
  const float s = ((a * a + b * b) + c * c) + 2.f * ((exy * exy + exz * exz) + eyz * eyz);
  eq = sqrtf(s / 1.5f);
}

// The geometry both kernels march over: a wave on kBX consecutive x of one row, a workgroup kBY rows, a run of kZ planes in z.
constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;

struct Gradient {
  float G00, G01, G02, G10, G11, G12, G20, G21, G22;  // G[r][c] = d(component r) / d(axis c)
};

// One lane's walk along z through its run of planes [z_begin, z_end), z_begin = blockIdx.z * kZ: march_prime() before the loop, then
// per plane march_step(), which gathers the six neighbours and gives G, and march_advance().  The lane keeps the z-1 / z / z+1
// samples of its own column in registers and loads plane z+2 during step z (one new plane per step, one step ahead), takes
// x-1 / x+1 from the neighbouring lanes (lanes 0 and kBX-1 load the halo column), and loads y-1 / y+1 through L1 / L2.  Every lane
// of the wave walks, owner of a column or not (the shuffles need them all).
// The geometry goes into these helpers BY VALUE: handed on by reference the compiler strength-reduces the row addresses of
// k_flow_strain into one pointer per array (80 / 94 VGPRs and a wave per SIMD less, against 71 / 84 with the addresses formed per step).
struct Column {
  Sample zm, zc, zq, zn;
  size_t row;  // of the step's plane
};

__device__ __forceinline__ int march_x() { return blockIdx.x * kBX + threadIdx.x; }
__device__ __forceinline__ int march_y() { return blockIdx.y * kBY + threadIdx.y; }
// the lane owns a column of the volume
__device__ __forceinline__ bool march_owns(const F3dGeo g) { return march_x() < g.W && march_y() < g.H; }

__device__ __forceinline__ void march_prime(const float* du, const float* dv, const float* dw, const F3dGeo g, int z_begin, Column& c)
{
  const int x = march_x(), y = march_y();
  const bool col = march_owns(g);
  c.zm = load(du, dv, dw, col && z_begin > 0 ? f3d_row(g, y, z_begin - 1) + x : 0, col && z_begin > 0);
  c.zc = load(du, dv, dw, col ? f3d_row(g, y, z_begin) + x : 0, col);
  c.zq = load(du, dv, dw, col && z_begin + 1 < g.D ? f3d_row(g, y, z_begin + 1) + x : 0, col && z_begin + 1 < g.D);
}

// G of the voxel at plane z; false when the voxel is outside the volume, absent, or lacks both neighbours along an axis
__device__ __forceinline__ bool march_step(const float* du, const float* dv, const float* dw, const F3dGeo g, int z, int z_end,
                                           Column& c, Gradient& G)
{
  const Sample &zm = c.zm, &zc = c.zc, &zq = c.zq;
  Sample& zn = c.zn;
  const int lane = threadIdx.x;
  const int x = march_x(), y = march_y();
  const bool col = march_owns(g);
  const bool nx1 = g.W == 1, ny1 = g.H == 1, nz1 = g.D == 1;
  const int x_halo = lane == 0 ? x - 1 : x + 1;  // lanes 0 and 63 load the neighbour outside the wave's 64 columns
  const bool halo_in = (lane == 0 || lane == kBX - 1) && x_halo >= 0 && x_halo < g.W && y < g.H;

  const size_t row = c.row = f3d_row(g, y, z);
  const Sample ym = load(du, dv, dw, col && y > 0 ? f3d_row(g, y - 1, z) + x : 0, col && y > 0);
  const Sample yq = load(du, dv, dw, col && y + 1 < g.H ? f3d_row(g, y + 1, z) + x : 0, col && y + 1 < g.H);
  const Sample xh = load(du, dv, dw, halo_in ? row + x_halo : 0, halo_in);
  // the plane after next, for the next step: issued last, so it stays in flight while this step computes and stores
  const bool in2 = col && z + 1 < z_end && z + 2 < g.D;
  zn = load(du, dv, dw, in2 ? f3d_row(g, y, z + 2) + x : 0, in2);
  Sample xm, xq;
  xm.u = __shfl(zc.u, lane - 1);
  xm.v = __shfl(zc.v, lane - 1);
  xm.w = __shfl(zc.w, lane - 1);
  xq.u = __shfl(zc.u, lane + 1);
  xq.v = __shfl(zc.v, lane + 1);
  xq.w = __shfl(zc.w, lane + 1);
  if (lane == 0) xm = xh;
  if (lane == kBX - 1) xq = xh;

  bool def = col && present(zc);
  def = column(xm, zc, xq, nx1, G.G00, G.G10, G.G20) && def;
  def = column(ym, zc, yq, ny1, G.G01, G.G11, G.G21) && def;
  def = column(zm, zc, zq, nz1, G.G02, G.G12, G.G22) && def;
  return def;
}

__device__ __forceinline__ void march_advance(Column& c)
{
  c.zm = c.zc;
  c.zc = c.zq;
  c.zq = c.zn;
}

}  // namespace f3d_strain
#endif  // F3D_STRAIN_GRAD_H_
