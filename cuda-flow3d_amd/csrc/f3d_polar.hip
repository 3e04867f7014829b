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
#include "f3d_tensor_tail.h"

namespace {

template <bool STATS, bool ROT>
__global__ __launch_bounds__(kBX* kBY) void k_polar(const float* __restrict__ du, const float* __restrict__ dv,
                                                    const float* __restrict__ dw, PolarOut out, F3dGeo g,
                                                    PolarPartial* __restrict__ partials)
{
  PolarPartial sum = PolarPartial::identity();  // this lane's voxels

  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  Column own;
  march_prime(du, dv, dw, g, z_begin, own);
  for (int z = z_begin; z < z_end; ++z) {
    Gradient G;
    const bool def = march_step(du, dv, dw, g, z, z_end, own, G);
    polar_voxel<STATS, ROT>(G, def, march_owns(g), own.row + march_x(), out, sum);  // f3d_tensor_tail.h
    march_advance(own);
  }

  if (STATS) polar_partial(sum, partials);
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
  polar_stats_of(r, stats);
  return 0;
}

}  // extern "C"
