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
#include "f3d_tensor_tail.h"

namespace {

template <bool STATS, bool DIRS>
__global__ __launch_bounds__(kBX* kBY) void k_principal_strain(const float* __restrict__ du, const float* __restrict__ dv,
                                                               const float* __restrict__ dw, PrincipalOut out, F3dGeo g,
                                                               PrincipalPartial* __restrict__ partials)
{
  PrincipalPartial sum = PrincipalPartial::identity();  // this lane's voxels

  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  Column own;
  march_prime(du, dv, dw, g, z_begin, own);
  for (int z = z_begin; z < z_end; ++z) {
    Gradient G;
    const bool def = march_step(du, dv, dw, g, z, z_end, own, G);
    principal_voxel<STATS, DIRS>(G, def, march_owns(g), own.row + march_x(), out, sum);  // f3d_tensor_tail.h
    march_advance(own);
  }

  if (STATS) principal_partial(sum, partials);
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
  principal_stats_of(r, stats);
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
