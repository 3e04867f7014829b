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
// Statistics (optional): one partial per workgroup, folded in a fixed order by a one-workgroup kernel, as in f3d_strain.hip.
#include "f3d_strain_grad.h"

namespace {

using namespace f3d_strain;

constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;
constexpr int kSweeps = 5;
constexpr int kReduceThreads = 256;

struct PrincipalPartial {
  unsigned long long defined;
  float e1_max, e3_min, shear_max, pad;
};

struct PrincipalOut {
  float* f[10];  // e1, e2, e3, gmax, d1x, d1y, d1z, d3x, d3y, d3z (null = not stored)
};

// include/f3d.h, f3d_principal_strain, rule 2: the rotation of the pair (p, q) with r the third index; vp / vq: columns p and q of V
template <bool DIRS>
__device__ __forceinline__ void rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float (&vp)[3], float (&vq)[3])
{
  if (apq == 0.f) return;
  const float theta = (aqq - app) / (2.f * apq);
  float t = 1.f / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  if (theta < 0.f) t = -t;
  const float c = 1.f / sqrtf(t * t + 1.f);
  const float s = t * c;
  const float h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.f;
  const float rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  if (DIRS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float kp = vp[k], kq = vq[k];
      vp[k] = c * kp - s * kq;
      vq[k] = s * kp + c * kq;
    }
  }
}

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
  const int lane = threadIdx.x;
  const int x = blockIdx.x * kBX + lane;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const bool col = x < g.W && y < g.H;  // the lane owns a column of the volume (every lane stays for the shuffles)
  const bool nx1 = g.W == 1, ny1 = g.H == 1, nz1 = g.D == 1;
  const int x_halo = lane == 0 ? x - 1 : x + 1;  // lanes 0 and 63 load the neighbour outside the wave's 64 columns
  const bool halo_in = (lane == 0 || lane == kBX - 1) && x_halo >= 0 && x_halo < g.W && y < g.H;
  const float nan = __builtin_nanf("");

  unsigned long long n_defined = 0;
  float e1max = -INFINITY, e3min = INFINITY, smax = -INFINITY;

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

    float a00, a11, a22, a01, a02, a12;
    green_lagrange(G00, G01, G02, G10, G11, G12, G20, G21, G22, a00, a11, a22, a01, a02, a12);
    if (!def) a00 = a11 = a22 = a01 = a02 = a12 = 0.f;  // NaN in every output below; nothing to rotate meanwhile
    float v0[3] = {1.f, 0.f, 0.f}, v1[3] = {0.f, 1.f, 0.f}, v2[3] = {0.f, 0.f, 1.f};  // the columns of V

    for (int sweep = 0; sweep < kSweeps; ++sweep) {
      // rule 2: a sweep over three zero off-diagonals is the identity, so once that holds in every lane the rest can go
      if (__ballot(a01 != 0.f || a02 != 0.f || a12 != 0.f) == 0) break;
      rotate<DIRS>(a00, a11, a01, a02, a12, v0, v1);  // (0, 1), r = 2
      rotate<DIRS>(a00, a22, a02, a01, a12, v0, v2);  // (0, 2), r = 1
      rotate<DIRS>(a11, a22, a12, a01, a02, v1, v2);  // (1, 2), r = 0
    }

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

    if (col) {
      const size_t i = row + x;
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
      ++n_defined;
      e1max = fmaxf(e1max, e1);
      e3min = fminf(e3min, e3);
      smax = fmaxf(smax, gmax);
    }
    zm = zc;
    zc = zq;
    zq = zn;
  }

  if (STATS) {
    // every lane is still here (no early return): wave reduction, then the kBY waves through LDS, one partial per workgroup
    __shared__ PrincipalPartial wave_part[kBY];
    n_defined = wave_sum(n_defined);
    e1max = wave_max(e1max);
    e3min = wave_min(e3min);
    smax = wave_max(smax);
    if (lane == 0) wave_part[threadIdx.y] = {n_defined, e1max, e3min, smax, 0.f};
    __syncthreads();
    if (lane == 0 && threadIdx.y == 0) {
      PrincipalPartial p = wave_part[0];
      for (int i = 1; i < kBY; ++i) {
        p.defined += wave_part[i].defined;
        p.e1_max = fmaxf(p.e1_max, wave_part[i].e1_max);
        p.e3_min = fminf(p.e3_min, wave_part[i].e3_min);
        p.shear_max = fmaxf(p.shear_max, wave_part[i].shear_max);
      }
      partials[(static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = p;
    }
  }
}

// the n partials folded into partials[n] by one workgroup: strided per thread, then a tree in LDS (a fixed order)
__global__ __launch_bounds__(kReduceThreads) void k_principal_strain_stats(PrincipalPartial* __restrict__ partials, size_t n)
{
  __shared__ PrincipalPartial part[kReduceThreads];
  PrincipalPartial p = {0ull, -INFINITY, INFINITY, -INFINITY, 0.f};
  for (size_t i = threadIdx.x; i < n; i += kReduceThreads) {
    const PrincipalPartial q = partials[i];
    p.defined += q.defined;
    p.e1_max = fmaxf(p.e1_max, q.e1_max);
    p.e3_min = fminf(p.e3_min, q.e3_min);
    p.shear_max = fmaxf(p.shear_max, q.shear_max);
  }
  part[threadIdx.x] = p;
  __syncthreads();
  for (int s = kReduceThreads / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) {
      PrincipalPartial& a = part[threadIdx.x];
      const PrincipalPartial& b = part[threadIdx.x + s];
      a.defined += b.defined;
      a.e1_max = fmaxf(a.e1_max, b.e1_max);
      a.e3_min = fminf(a.e3_min, b.e3_min);
      a.shear_max = fmaxf(a.shear_max, b.shear_max);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[n] = part[0];
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
  // one partial per workgroup and one for the result; per thread: two lanes may ask at once
  static thread_local PrincipalPartial* d_part = nullptr;
  static thread_local size_t d_part_count = 0;
  const size_t n = static_cast<size_t>(grid.x) * grid.y * grid.z;
  if (d_part_count < n + 1) {
    if (d_part) F3D_HIP(hipFree(d_part));
    d_part = nullptr;
    d_part_count = 0;
    F3D_HIP(hipMalloc(reinterpret_cast<void**>(&d_part), (n + 1) * sizeof(PrincipalPartial)));
    d_part_count = n + 1;
  }
  hipLaunchKernelGGL((k_principal_strain<true, DIRS>), grid, dim3(kBX, kBY, 1), 0, f3d::stream(), u, v, w, o, g, d_part);
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_principal_strain_stats, dim3(1), dim3(kReduceThreads), 0, f3d::stream(), d_part, n);
  F3D_HIP(hipGetLastError());
  PrincipalPartial r;
  F3D_HIP(hipMemcpyAsync(&r, d_part + n, sizeof(r), hipMemcpyDeviceToHost, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
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
  for (int f = 0; f < 10; ++f) {
    o.f[f] = nullptr;
    if (!(fields & groups[f])) continue;
    if (!out[f]) return f3d::fail("f3d_principal_strain: output %d (%s) is selected but null", f, names[f]);
    if (out[f] == u || out[f] == v || out[f] == w)
      return f3d::fail("f3d_principal_strain: output %d (%s) is also an input (the stencil reads neighbours)", f, names[f]);
    for (int e = 0; e < f; ++e)
      if (o.f[e] && out[e] == out[f])
        return f3d::fail("f3d_principal_strain: outputs %d (%s) and %d (%s) are the same container", e, names[e], f, names[f]);
    o.f[f] = f3d_ptr<float>(out[f]);
  }
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_principal_strain")) return 1;
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  if (fields & (F3D_PRINCIPAL_DIR1 | F3D_PRINCIPAL_DIR3)) return launch<true>(pu, pv, pw, o, g, stats);
  return launch<false>(pu, pv, pw, o, g, stats);
}

}  // extern "C"
