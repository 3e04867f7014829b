// Principal strains of a displacement for gfx950: per voxel the Green-Lagrange tensor E of f3d_flow_strain (same gradient, same
// missing-sample rules, same expressions: f3d_strain_grad.h), diagonalised by five cyclic Jacobi sweeps, ordered, and stored as
// e1 >= e2 >= e3, the maximum shear and the directions of e1 and e3.  The definition and the evaluation order are those of
// include/f3d.h (f3d_principal_strain); tests/principal_ref.py restates them in float32 numpy and matches the kernel bit for bit.
//
// Shape: k_flow_strain's (a wave on 64 consecutive x of one row, a workgroup kBY rows, a register march in z over kZ planes, the
// x neighbours by __shfl, full-row stores).  E never goes to memory.  The Jacobi part is per-lane vector arithmetic on the six
// entries of A and, when a direction is stored, the nine of V (DIRS; without it V is not carried).  A rotation whose off-diagonal
// is 0 is the identity by definition, so a wave leaves the sweep loop as soon as no lane has an off-diagonal left; lanes outside the
// volume and lanes of undefined voxels diagonalise the zero matrix and never hold their wave back.
//
// Statistics (optional): one partial per workgroup, folded in a fixed order by a one-workgroup kernel (f3d_partials.h).
#include "f3d_jacobi3.h"
#include "f3d_strain_grad.h"

namespace {

using namespace f3d_strain;
using namespace f3d_partials;

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

template <bool STATS, bool DIRS>
__global__ __launch_bounds__(kBX* kBY) void k_principal_strain(const float* __restrict__ du, const float* __restrict__ dv,
                                                               const float* __restrict__ dw, PrincipalOut out, F3dGeo g,
                                                               PrincipalPartial* __restrict__ partials)
{
  const float nan = __builtin_nanf("");
  PrincipalPartial sum = PrincipalPartial::identity();  // this lane's voxels

  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  Column own;
  march_prime(du, dv, dw, g, z_begin, own);
  for (int z = z_begin; z < z_end; ++z) {
    Gradient G;
    const bool def = march_step(du, dv, dw, g, z, z_end, own, G);
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

    if (march_owns(g)) {
      const size_t i = own.row + march_x();
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
    march_advance(own);
  }

  if (STATS) {
    sum.defined = wave_sum(sum.defined);
    sum.e1_max = wave_max(sum.e1_max);
    sum.e3_min = wave_min(sum.e3_min);
    sum.shear_max = wave_max(sum.shear_max);
    block_partial<PrincipalPartial, kBY>(sum, partials);
  }
}

template <bool DIRS>
int launch(const float* u, const float* v, const float* w, const PrincipalOut& o, const F3dGeo& g, f3d_principal_stats* stats)
{
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ);
  if (!stats) {
    hipLaunchKernelGGL((k_principal_strain<false, DIRS>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), u, v, w, o, g, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  PrincipalPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](PrincipalPartial* d_part) {
        hipLaunchKernelGGL((k_principal_strain<true, DIRS>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), u, v, w, o, g, d_part);
      }))
    return 1;
  stats->defined = r.defined;
  stats->e1_max = r.defined ? r.e1_max : __builtin_nanf("");
  stats->e3_min = r.defined ? r.e3_min : __builtin_nanf("");
  stats->shear_max = r.defined ? r.shear_max : __builtin_nanf("");
  return 0;
}

}  // namespace

extern "C" {

int f3d_principal_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[10], unsigned fields, size_t width,
                         size_t height, size_t depth, f3d_principal_stats* stats)
{
  F3D_REQUIRE_READY("f3d_principal_strain");
  if (!u || !v || !w) return f3d::fail("f3d_principal_strain: null input");
  const unsigned all = F3D_PRINCIPAL_VALUES | F3D_PRINCIPAL_SHEAR | F3D_PRINCIPAL_DIR1 | F3D_PRINCIPAL_DIR3;
  if (fields == 0 || (fields & ~all))
    return f3d::fail("f3d_principal_strain: fields must be a non-empty combination of F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_SHEAR, "
                     "F3D_PRINCIPAL_DIR1, F3D_PRINCIPAL_DIR3 (got %u)", fields);
  if (!out) return f3d::fail("f3d_principal_strain: null output array");
  static const char* const names[10] = {"e1", "e2", "e3", "gmax", "d1x", "d1y", "d1z", "d3x", "d3y", "d3z"};
  static const unsigned groups[10] = {F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_SHEAR,
                                      F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR3,
                                      F3D_PRINCIPAL_DIR3,   F3D_PRINCIPAL_DIR3};
  PrincipalOut o;
  if (!f3d::select_outputs("f3d_principal_strain", "the stencil reads neighbours", o.f, out, 10, names, groups, fields, u, v, w))
    return 1;
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_principal_strain")) return 1;
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  if (fields & (F3D_PRINCIPAL_DIR1 | F3D_PRINCIPAL_DIR3)) return launch<true>(pu, pv, pw, o, g, stats);
  return launch<false>(pu, pv, pw, o, g, stats);
}

}  // extern "C"
