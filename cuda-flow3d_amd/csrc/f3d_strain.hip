// Strain fields of a displacement for gfx950: per voxel the displacement gradient G = dd/dx by central differences (one-sided where a
// neighbour is missing), and from it the relative volume change J - 1, the Green-Lagrange strain E = 1/2 (F^T F - I) and its
// equivalent (von Mises) strain.  The definition, the missing-sample rules and the evaluation order are those of include/f3d.h
// (f3d_flow_strain); tests/strain_ref.py restates them in float32 numpy and matches the kernel bit for bit.
//
// Shape: a wave on 64 consecutive x of one row, a workgroup kBY rows, marching in z over a run of kZ planes.  Each lane keeps the
// z-1 / z / z+1 samples of its own column in registers and loads plane z+2 during step z (one new plane per step, one step ahead, so
// that its HBM latency overlaps the step's arithmetic and stores), takes x-1 / x+1 from the neighbouring lanes (__shfl; lanes 0 and
// 63 load the halo column), and loads y-1 / y+1, which the neighbouring waves are reading at the same time, through L1 / L2.
// Compulsory traffic: 12 B read + 4 B per stored field.  Stores are full 256-B rows (plain stores: non-temporal ones measured the
// same).
//
// Statistics (optional): each workgroup reduces its voxels into one partial (counts, min / max, double sum) in a buffer of its own;
// a one-workgroup kernel then folds the partials in a fixed order, so the result does not depend on scheduling.
#include "f3d_strain_grad.h"

namespace {

using namespace f3d_strain;
using namespace f3d_partials;

struct StrainPartial {
  unsigned long long defined, folded;
  float vol_min, vol_max, eq_max, pad;
  double vol_sum;

  static __device__ __forceinline__ StrainPartial identity() { return {0ull, 0ull, INFINITY, -INFINITY, -INFINITY, 0.f, 0.0}; }
  __device__ __forceinline__ void merge(const StrainPartial& q)
  {
    defined += q.defined;
    folded += q.folded;
    vol_min = fminf(vol_min, q.vol_min);
    vol_max = fmaxf(vol_max, q.vol_max);
    eq_max = fmaxf(eq_max, q.eq_max);
    vol_sum += q.vol_sum;
  }
};

struct StrainOut {
  float* f[8];  // vol, exx, eyy, ezz, exy, exz, eyz, eq (null = not stored)
};

template <bool STATS>
__global__ __launch_bounds__(kBX* kBY) void k_flow_strain(const float* __restrict__ du, const float* __restrict__ dv,
                                                          const float* __restrict__ dw, StrainOut out, F3dGeo g,
                                                          StrainPartial* __restrict__ partials)
{
  StrainPartial sum = StrainPartial::identity();  // this lane's voxels

  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  Column own;
  march_prime(du, dv, dw, g, z_begin, own);
  for (int z = z_begin; z < z_end; ++z) {
    Gradient G;
    const bool def = march_step(du, dv, dw, g, z, z_end, own, G);
    const auto& [G00, G01, G02, G10, G11, G12, G20, G21, G22] = G;

    float vol, exx, eyy, ezz, exy, exz, eyz, eq;
    strain_fields(G00, G01, G02, G10, G11, G12, G20, G21, G22, vol, exx, eyy, ezz, exy, exz, eyz, eq);
    if (!def) {
      vol = exx = eyy = ezz = exy = exz = eyz = eq = __builtin_nanf("");
    }

    if (march_owns(g)) {
      const size_t i = own.row + march_x();
      const float vals[8] = {vol, exx, eyy, ezz, exy, exz, eyz, eq};
#pragma unroll
      for (int f = 0; f < 8; ++f)
        if (out.f[f]) out.f[f][i] = vals[f];
    }
    if (STATS && !isnan(vol)) {
      ++sum.defined;
      sum.folded += vol <= -1.f ? 1 : 0;
      sum.vol_min = fminf(sum.vol_min, vol);
      sum.vol_max = fmaxf(sum.vol_max, vol);
      sum.eq_max = fmaxf(sum.eq_max, eq);
      sum.vol_sum += static_cast<double>(vol);
    }
    march_advance(own);
  }

  if (STATS) {
    sum.defined = wave_sum(sum.defined);
    sum.folded = wave_sum(sum.folded);
    sum.vol_min = wave_min(sum.vol_min);
    sum.vol_max = wave_max(sum.vol_max);
    sum.eq_max = wave_max(sum.eq_max);
    sum.vol_sum = wave_sum(sum.vol_sum);
    block_partial<StrainPartial, kBY>(sum, partials);
  }
}

}  // namespace

extern "C" {

int f3d_flow_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[8], unsigned fields, size_t width,
                    size_t height, size_t depth, f3d_strain_stats* stats)
{
  F3D_REQUIRE_READY("f3d_flow_strain");
  if (!u || !v || !w) return f3d::fail("f3d_flow_strain: null input");
  if (fields == 0 || (fields & ~(F3D_STRAIN_VOL | F3D_STRAIN_E | F3D_STRAIN_EQ)))
    return f3d::fail("f3d_flow_strain: fields must be a non-empty combination of F3D_STRAIN_VOL, F3D_STRAIN_E, F3D_STRAIN_EQ (got %u)",
                     fields);
  if (!out) return f3d::fail("f3d_flow_strain: null output array");
  static const char* const names[8] = {"vol", "exx", "eyy", "ezz", "exy", "exz", "eyz", "eq"};
  static const unsigned groups[8] = {F3D_STRAIN_VOL, F3D_STRAIN_E, F3D_STRAIN_E, F3D_STRAIN_E,
                                     F3D_STRAIN_E,   F3D_STRAIN_E, F3D_STRAIN_E, F3D_STRAIN_EQ};
  StrainOut o;
  if (!f3d::select_outputs("f3d_flow_strain", "the stencil reads neighbours", o.f, out, 8, names, groups, fields, u, v, w)) return 1;
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_flow_strain")) return 1;
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ);
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  if (!stats) {
    hipLaunchKernelGGL(k_flow_strain<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, o, g, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  StrainPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](StrainPartial* d_part) {
        hipLaunchKernelGGL(k_flow_strain<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, o, g, d_part);
      }))
    return 1;
  stats->defined = r.defined;
  stats->folded = r.folded;
  stats->vol_min = r.defined ? r.vol_min : __builtin_nanf("");
  stats->vol_max = r.defined ? r.vol_max : __builtin_nanf("");
  stats->eq_max = r.defined ? r.eq_max : __builtin_nanf("");
  stats->vol_sum = r.vol_sum;
  return 0;
}

}  // extern "C"
