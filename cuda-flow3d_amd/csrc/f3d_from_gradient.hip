// Principal strains and the polar decomposition of a stored displacement gradient for gfx950: f3d_principal_from_gradient and
// f3d_polar_from_gradient of include/f3d.h.  The nine entries of G come from containers (f3d_window_strain's F3D_WSTRAIN_G group, an
// FE solution, a filter of the caller's) instead of a stencil on the displacement; everything after G is the text of
// f3d_principal_strain and f3d_polar_decomposition (f3d_tensor_tail.h), so the central-difference gradient fed here gives their
// results bit for bit.  tests/from_gradient_ref.py restates both in float32 numpy and matches the kernels bit for bit.
//
// Shape: the decomposition of the stencil siblings, so the statistics fold in the same order (a wave on 64 consecutive x of one
// row, a workgroup kBY rows, a register march in z over kZ planes, grid (ceil(W / 64), ceil(H / 4), ceil(D / 32)), the partial index
// and the fold of f3d_partials.h).  Pointwise in G: no neighbours, no LDS, no shuffles but the sweeps' ballot.  The nine loads of
// plane z + 1 are issued before plane z is computed and stored (the zn idea of march_step), full-row stores.  A voxel is
// undefined iff any of its nine entries is NaN; lanes outside the volume hold NaN and diagonalise the zero matrix.
//
// The inputs carry no __restrict__: two entries of grad may be the same container.  No output is an input (refused).
#include "f3d_tensor_tail.h"

namespace {

struct GradientIn {
  const float* g[9];  // G00 G01 G02 G10 G11 G12 G20 G21 G22
};

// the nine entries at index i, NaN when the lane has nothing there
__device__ __forceinline__ Gradient load_gradient(const GradientIn& in, size_t i, bool have)
{
  const float nan = __builtin_nanf("");
  Gradient G = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
  if (have) {
    G.G00 = in.g[0][i];
    G.G01 = in.g[1][i];
    G.G02 = in.g[2][i];
    G.G10 = in.g[3][i];
    G.G11 = in.g[4][i];
    G.G12 = in.g[5][i];
    G.G20 = in.g[6][i];
    G.G21 = in.g[7][i];
    G.G22 = in.g[8][i];
  }
  return G;
}

__device__ __forceinline__ bool defined(const Gradient& G)
{
  return !(isnan(G.G00) || isnan(G.G01) || isnan(G.G02) || isnan(G.G10) || isnan(G.G11) || isnan(G.G12) || isnan(G.G20) ||
           isnan(G.G21) || isnan(G.G22));
}

// The march both kernels make: voxel(G, def, owns, i) for every plane of the lane's run, the next plane's loads in flight meanwhile.
template <typename Voxel>
__device__ __forceinline__ void march(const GradientIn& in, const F3dGeo g, Voxel&& voxel)
{
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const int x = march_x(), y = march_y();
  const bool col = march_owns(g);
  Gradient next = load_gradient(in, col ? f3d_row(g, y, z_begin) + x : 0, col);
  for (int z = z_begin; z < z_end; ++z) {
    const Gradient G = next;
    const bool more = col && z + 1 < z_end;
    next = load_gradient(in, more ? f3d_row(g, y, z + 1) + x : 0, more);
    voxel(G, col && defined(G), col, f3d_row(g, y, z) + x);
  }
}

template <bool STATS, bool DIRS>
__global__ __launch_bounds__(kBX* kBY) void k_principal_from_gradient(GradientIn in, PrincipalOut out, F3dGeo g,
                                                                      PrincipalPartial* __restrict__ partials)
{
  PrincipalPartial sum = PrincipalPartial::identity();  // this lane's voxels
  march(in, g, [&](const Gradient& G, bool def, bool owns, size_t i) { principal_voxel<STATS, DIRS>(G, def, owns, i, out, sum); });
  if (STATS) principal_partial(sum, partials);
}

template <bool STATS, bool ROT>
__global__ __launch_bounds__(kBX* kBY) void k_polar_from_gradient(GradientIn in, PolarOut out, F3dGeo g,
                                                                  PolarPartial* __restrict__ partials)
{
  PolarPartial sum = PolarPartial::identity();  // this lane's voxels
  march(in, g, [&](const Gradient& G, bool def, bool owns, size_t i) { polar_voxel<STATS, ROT>(G, def, owns, i, out, sum); });
  if (STATS) polar_partial(sum, partials);
}

dim3 grid_of(const F3dGeo& g) { return dim3((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ); }

template <bool DIRS>
int launch_principal(const GradientIn& in, const PrincipalOut& o, const F3dGeo& g, f3d_principal_stats* stats)
{
  const dim3 grid = grid_of(g);
  if (!stats) {
    hipLaunchKernelGGL((k_principal_from_gradient<false, DIRS>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), in, o, g, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  PrincipalPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](PrincipalPartial* d_part) {
        hipLaunchKernelGGL((k_principal_from_gradient<true, DIRS>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), in, o, g, d_part);
      }))
    return 1;
  principal_stats_of(r, stats);
  return 0;
}

const char* const kReads = "a plane's gradient is loaded before the plane before it is stored";

// the checks of grad both entries make; false with the error set
bool gradient_in(const char* who, const f3d_devptr* grad, GradientIn* in)
{
  if (!grad) return !f3d::fail("%s: null gradient array", who);
  for (int k = 0; k < 9; ++k) {
    if (!grad[k]) return !f3d::fail("%s: gradient entry %d (G%d%d) is null", who, k, k / 3, k % 3);
    in->g[k] = f3d_ptr<const float>(grad[k]);
  }
  return true;
}

}  // namespace

extern "C" {

int f3d_principal_from_gradient(const f3d_devptr grad[9], const f3d_devptr out[10], unsigned fields, size_t width, size_t height,
                                size_t depth, f3d_principal_stats* stats)
{
  const char* const who = "f3d_principal_from_gradient";
  F3D_REQUIRE_READY(who);
  GradientIn in;
  if (!gradient_in(who, grad, &in)) return 1;
  const unsigned all = F3D_PRINCIPAL_VALUES | F3D_PRINCIPAL_SHEAR | F3D_PRINCIPAL_DIR1 | F3D_PRINCIPAL_DIR3;
  if (fields == 0 || (fields & ~all))
    return f3d::fail("%s: fields must be a non-empty combination of F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_SHEAR, F3D_PRINCIPAL_DIR1, "
                     "F3D_PRINCIPAL_DIR3 (got %u)", who, fields);
  if (!out) return f3d::fail("%s: null output array", who);
  static const char* const names[10] = {"e1", "e2", "e3", "gmax", "d1x", "d1y", "d1z", "d3x", "d3y", "d3z"};
  static const unsigned groups[10] = {F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_SHEAR,
                                      F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR3,
                                      F3D_PRINCIPAL_DIR3,   F3D_PRINCIPAL_DIR3};
  PrincipalOut o;
  if (!f3d::select_outputs(who, kReads, o.f, out, 10, names, groups, fields, grad, 9)) return 1;
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, who)) return 1;
  if (fields & (F3D_PRINCIPAL_DIR1 | F3D_PRINCIPAL_DIR3)) return launch_principal<true>(in, o, g, stats);
  return launch_principal<false>(in, o, g, stats);
}

int f3d_polar_from_gradient(const f3d_devptr grad[9], const f3d_devptr out[7], unsigned fields, size_t width, size_t height,
                            size_t depth, f3d_polar_stats* stats)
{
  const char* const who = "f3d_polar_from_gradient";
  F3D_REQUIRE_READY(who);
  GradientIn in;
  if (!gradient_in(who, grad, &in)) return 1;
  const unsigned all = F3D_POLAR_ANGLE | F3D_POLAR_VECTOR | F3D_POLAR_STRETCH;
  if (fields == 0 || (fields & ~all))
    return f3d::fail("%s: fields must be a non-empty combination of F3D_POLAR_ANGLE, F3D_POLAR_VECTOR, F3D_POLAR_STRETCH (got %u)", who,
                     fields);
  if (!out) return f3d::fail("%s: null output array", who);
  static const char* const names[7] = {"theta", "rx", "ry", "rz", "l1", "l2", "l3"};
  static const unsigned groups[7] = {F3D_POLAR_ANGLE,   F3D_POLAR_VECTOR,  F3D_POLAR_VECTOR, F3D_POLAR_VECTOR,
                                     F3D_POLAR_STRETCH, F3D_POLAR_STRETCH, F3D_POLAR_STRETCH};
  PolarOut o;
  if (!f3d::select_outputs(who, kReads, o.f, out, 7, names, groups, fields, grad, 9)) return 1;
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, who)) return 1;
  const dim3 grid = grid_of(g);
  if (!stats) {
    // the statistics hold the angle; without them a selection of the stretches alone carries no V
    if (fields & (F3D_POLAR_ANGLE | F3D_POLAR_VECTOR))
      hipLaunchKernelGGL((k_polar_from_gradient<false, true>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), in, o, g, nullptr);
    else
      hipLaunchKernelGGL((k_polar_from_gradient<false, false>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), in, o, g, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  PolarPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](PolarPartial* d_part) {
        hipLaunchKernelGGL((k_polar_from_gradient<true, true>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), in, o, g, d_part);
      }))
    return 1;
  polar_stats_of(r, stats);
  return 0;
}

}  // extern "C"
