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

constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;
constexpr int kReduceThreads = 256;

struct StrainPartial {
  unsigned long long defined, folded;
  float vol_min, vol_max, eq_max, pad;
  double vol_sum;
};

struct StrainOut {
  float* f[8];  // vol, exx, eyy, ezz, exy, exz, eyz, eq (null = not stored)
};

template <bool STATS>
__global__ __launch_bounds__(kBX* kBY) void k_flow_strain(const float* __restrict__ du, const float* __restrict__ dv,
                                                          const float* __restrict__ dw, StrainOut out, F3dGeo g,
                                                          StrainPartial* __restrict__ partials)
{
  const int lane = threadIdx.x;
  const int x = blockIdx.x * kBX + lane;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const bool col = x < g.W && y < g.H;  // the lane owns a column of the volume (every lane stays for the shuffles)
  const bool nx1 = g.W == 1, ny1 = g.H == 1, nz1 = g.D == 1;
  const int x_halo = lane == 0 ? x - 1 : x + 1;  // lanes 0 and 63 load the neighbour outside the wave's 64 columns
  const bool halo_in = (lane == 0 || lane == kBX - 1) && x_halo >= 0 && x_halo < g.W && y < g.H;

  unsigned long long n_defined = 0, n_folded = 0;
  float vmin = INFINITY, vmax = -INFINITY, emax = -INFINITY;
  double vsum = 0.0;

  Sample zm = load(du, dv, dw, col && z_begin > 0 ? f3d_row(g, y, z_begin - 1) + x : 0, col && z_begin > 0);
  Sample zc = load(du, dv, dw, col ? f3d_row(g, y, z_begin) + x : 0, col);
  Sample zq = load(du, dv, dw, col && z_begin + 1 < g.D ? f3d_row(g, y, z_begin + 1) + x : 0, col && z_begin + 1 < g.D);
  for (int z = z_begin; z < z_end; ++z) {
    const size_t row = f3d_row(g, y, z);
    const Sample ym = load(du, dv, dw, col && y > 0 ? f3d_row(g, y - 1, z) + x : 0, col && y > 0);
    const Sample yq = load(du, dv, dw, col && y + 1 < g.H ? f3d_row(g, y + 1, z) + x : 0, col && y + 1 < g.H);
    const Sample xh = load(du, dv, dw, halo_in ? row + x_halo : 0, halo_in);
    // the plane after next, for the next step: issued last, so it stays in flight while this step computes and stores
    const bool in2 = col && z + 1 < z_end && z + 2 < g.D;
    const Sample zn = load(du, dv, dw, in2 ? f3d_row(g, y, z + 2) + x : 0, in2);
    Sample xm, xq;
    xm.u = __shfl(zc.u, lane - 1);
    xm.v = __shfl(zc.v, lane - 1);
    xm.w = __shfl(zc.w, lane - 1);
    xq.u = __shfl(zc.u, lane + 1);
    xq.v = __shfl(zc.v, lane + 1);
    xq.w = __shfl(zc.w, lane + 1);
    if (lane == 0) xm = xh;
    if (lane == kBX - 1) xq = xh;

    float G00, G01, G02, G10, G11, G12, G20, G21, G22;  // G[r][c] = d(component r) / d(axis c)
    bool def = col && present(zc);
    def = column(xm, zc, xq, nx1, G00, G10, G20) && def;
    def = column(ym, zc, yq, ny1, G01, G11, G21) && def;
    def = column(zm, zc, zq, nz1, G02, G12, G22) && def;

    // include/f3d.h, f3d_flow_strain: the evaluation order is part of the ABI (contraction is off in this build)
    const float I1 = (G00 + G11) + G22;
    const float I2 = ((G00 * G11 - G01 * G10) + (G11 * G22 - G12 * G21)) + (G00 * G22 - G02 * G20);
    const float I3 = (G00 * (G11 * G22 - G12 * G21) - G01 * (G10 * G22 - G12 * G20)) + G02 * (G10 * G21 - G11 * G20);
    float vol = (I1 + I2) + I3;
    float exx, eyy, ezz, exy, exz, eyz;
    green_lagrange(G00, G01, G02, G10, G11, G12, G20, G21, G22, exx, eyy, ezz, exy, exz, eyz);
    const float mean = ((exx + eyy) + ezz) / 3.f;
    const float a = exx - mean, b = eyy - mean, c = ezz - mean;
    const float s = ((a * a + b * b) + c * c) + 2.f * ((exy * exy + exz * exz) + eyz * eyz);
    float eq = sqrtf(s / 1.5f);
    if (!def) {
      vol = exx = eyy = ezz = exy = exz = eyz = eq = __builtin_nanf("");
    }

    if (col) {
      const size_t i = row + x;
      const float vals[8] = {vol, exx, eyy, ezz, exy, exz, eyz, eq};
#pragma unroll
      for (int f = 0; f < 8; ++f)
        if (out.f[f]) out.f[f][i] = vals[f];
    }
    if (STATS && !isnan(vol)) {
      ++n_defined;
      n_folded += vol <= -1.f ? 1 : 0;
      vmin = fminf(vmin, vol);
      vmax = fmaxf(vmax, vol);
      emax = fmaxf(emax, eq);
      vsum += static_cast<double>(vol);
    }
    zm = zc;
    zc = zq;
    zq = zn;
  }

  if (STATS) {
    // every lane is still here (no early return): wave reduction, then the kBY waves through LDS, one partial per workgroup
    __shared__ StrainPartial wave_part[kBY];
    n_defined = wave_sum(n_defined);
    n_folded = wave_sum(n_folded);
    vmin = wave_min(vmin);
    vmax = wave_max(vmax);
    emax = wave_max(emax);
    vsum = wave_sum(vsum);
    if (lane == 0) wave_part[threadIdx.y] = {n_defined, n_folded, vmin, vmax, emax, 0.f, vsum};
    __syncthreads();
    if (lane == 0 && threadIdx.y == 0) {
      StrainPartial p = wave_part[0];
      for (int i = 1; i < kBY; ++i) {
        p.defined += wave_part[i].defined;
        p.folded += wave_part[i].folded;
        p.vol_min = fminf(p.vol_min, wave_part[i].vol_min);
        p.vol_max = fmaxf(p.vol_max, wave_part[i].vol_max);
        p.eq_max = fmaxf(p.eq_max, wave_part[i].eq_max);
        p.vol_sum += wave_part[i].vol_sum;
      }
      partials[(static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = p;
    }
  }
}

// the n partials folded into partials[n] by one workgroup: strided per thread, then a tree in LDS (a fixed order)
__global__ __launch_bounds__(kReduceThreads) void k_flow_strain_stats(StrainPartial* __restrict__ partials, size_t n)
{
  __shared__ StrainPartial part[kReduceThreads];
  StrainPartial p = {0ull, 0ull, INFINITY, -INFINITY, -INFINITY, 0.f, 0.0};
  for (size_t i = threadIdx.x; i < n; i += kReduceThreads) {
    const StrainPartial q = partials[i];
    p.defined += q.defined;
    p.folded += q.folded;
    p.vol_min = fminf(p.vol_min, q.vol_min);
    p.vol_max = fmaxf(p.vol_max, q.vol_max);
    p.eq_max = fmaxf(p.eq_max, q.eq_max);
    p.vol_sum += q.vol_sum;
  }
  part[threadIdx.x] = p;
  __syncthreads();
  for (int s = kReduceThreads / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) {
      StrainPartial& a = part[threadIdx.x];
      const StrainPartial& b = part[threadIdx.x + s];
      a.defined += b.defined;
      a.folded += b.folded;
      a.vol_min = fminf(a.vol_min, b.vol_min);
      a.vol_max = fmaxf(a.vol_max, b.vol_max);
      a.eq_max = fmaxf(a.eq_max, b.eq_max);
      a.vol_sum += b.vol_sum;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[n] = part[0];
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
  StrainOut o;
  for (int f = 0; f < 8; ++f) {
    const unsigned group = f == 0 ? F3D_STRAIN_VOL : (f == 7 ? F3D_STRAIN_EQ : F3D_STRAIN_E);
    o.f[f] = nullptr;
    if (!(fields & group)) continue;
    if (!out[f]) return f3d::fail("f3d_flow_strain: output %d (%s) is selected but null", f, names[f]);
    if (out[f] == u || out[f] == v || out[f] == w)
      return f3d::fail("f3d_flow_strain: output %d (%s) is also an input (the stencil reads neighbours)", f, names[f]);
    for (int e = 0; e < f; ++e)
      if (o.f[e] && out[e] == out[f])
        return f3d::fail("f3d_flow_strain: outputs %d (%s) and %d (%s) are the same container", e, names[e], f, names[f]);
    o.f[f] = f3d_ptr<float>(out[f]);
  }
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_flow_strain")) return 1;
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ);
  if (!stats) {
    hipLaunchKernelGGL(k_flow_strain<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), f3d_ptr<const float>(u),
                       f3d_ptr<const float>(v), f3d_ptr<const float>(w), o, g, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  // one partial per workgroup and one for the result; per thread: two lanes may ask at once
  static thread_local StrainPartial* d_part = nullptr;
  static thread_local size_t d_part_count = 0;
  const size_t n = static_cast<size_t>(grid.x) * grid.y * grid.z;
  if (d_part_count < n + 1) {
    if (d_part) F3D_HIP(hipFree(d_part));
    d_part = nullptr;
    d_part_count = 0;
    F3D_HIP(hipMalloc(reinterpret_cast<void**>(&d_part), (n + 1) * sizeof(StrainPartial)));
    d_part_count = n + 1;
  }
  hipLaunchKernelGGL(k_flow_strain<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), f3d_ptr<const float>(u),
                     f3d_ptr<const float>(v), f3d_ptr<const float>(w), o, g, d_part);
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_flow_strain_stats, dim3(1), dim3(kReduceThreads), 0, f3d::stream(), d_part, n);
  F3D_HIP(hipGetLastError());
  StrainPartial r;
  F3D_HIP(hipMemcpyAsync(&r, d_part + n, sizeof(r), hipMemcpyDeviceToHost, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  stats->defined = r.defined;
  stats->folded = r.folded;
  stats->vol_min = r.defined ? r.vol_min : __builtin_nanf("");
  stats->vol_max = r.defined ? r.vol_max : __builtin_nanf("");
  stats->eq_max = r.defined ? r.eq_max : __builtin_nanf("");
  stats->vol_sum = r.vol_sum;
  return 0;
}

}  // extern "C"
