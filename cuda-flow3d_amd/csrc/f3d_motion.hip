// Rigid-body / affine motion of a displacement for gfx950: the moment sums a least-squares fit d ~ t + M (x - c) needs
// (f3d_motion_sums: one reduction pass over u, v, w and an optional binary mask) and the subtraction of a fit per voxel
// (f3d_remove_motion: one streaming pass, with the statistics of the residual on request).  The definitions, the presence rule and
// the evaluation order are those of include/f3d.h; the solve between the two is host code (host/motion_fit.cpp).
// tests/motion_ref.py restates both in numpy: the residuals match bit for bit, the sums within the bound of any summation order.
//
// Shape: k_flow_strain's without the stencil.  A wave on 64 consecutive x of one row, a workgroup kBY rows, a lane marching in z over
// a run of kZ planes of its own column with the next plane's loads issued before the current plane's arithmetic.  Loads and stores
// are full 256-B rows; no LDS beyond the skeleton's, no scratch, no AGPRs.
//
// Sums: the coordinate sums are exact integers of the doubled coordinates 2x - (W-1); a lane keeps the count, the sum and the sum
// of squares of its run's doubled z and forms the nine coordinate sums from them and its column's constant doubled x and y at the
// end of the run.  The displacement sums are binary64; a lane keeps sum d, sum Z d and sum d^2 per component (nine accumulators)
// and forms X sum d and Y sum d at the end of the run.  Workgroups write one partial each and a one-workgroup kernel folds them in
// the fixed order of f3d_partials.h, so the same input gives the same bytes.
#include "f3d_internal.h"
#include "f3d_partials.h"

namespace {

using namespace f3d_partials;

constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;

struct MotionPartial {
  long long n;
  long long x2[3];   // sums of the doubled coordinates
  long long xx4[6];  // sums of their products: xx yy zz xy xz yz
  double d[3], xd[9], dd[3];

  static __device__ __forceinline__ MotionPartial identity()
  {
    MotionPartial p;
    p.n = 0;
    for (long long& v : p.x2) v = 0;
    for (long long& v : p.xx4) v = 0;
    for (double& v : p.d) v = 0.0;
    for (double& v : p.xd) v = 0.0;
    for (double& v : p.dd) v = 0.0;
    return p;
  }
  __device__ __forceinline__ void merge(const MotionPartial& q)
  {
    n += q.n;
    for (int i = 0; i < 3; ++i) x2[i] += q.x2[i];
    for (int i = 0; i < 6; ++i) xx4[i] += q.xx4[i];
    for (int i = 0; i < 3; ++i) d[i] += q.d[i];
    for (int i = 0; i < 9; ++i) xd[i] += q.xd[i];
    for (int i = 0; i < 3; ++i) dd[i] += q.dd[i];
  }
};

__device__ __forceinline__ long long wave_sum_i64(long long x)
{
  return static_cast<long long>(wave_sum(static_cast<unsigned long long>(x)));  // two's complement: the wrapped sum is the signed one
}

// include/f3d.h, f3d_motion_sums
template <bool WEIGHT>
__global__ __launch_bounds__(kBX* kBY) void k_motion_sums(const float* __restrict__ du, const float* __restrict__ dv,
                                                          const float* __restrict__ dw, const float* __restrict__ weight,
                                                          float weight_min, F3dGeo g, MotionPartial* __restrict__ partials)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const bool col = x < g.W && y < g.H;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const float nan = __builtin_nanf("");

  int cnt = 0;
  long long sz2 = 0, szz4 = 0;
  double su = 0.0, sv = 0.0, sw = 0.0, zu = 0.0, zv = 0.0, zw = 0.0, uu = 0.0, vv = 0.0, ww = 0.0;

  // the plane one step ahead: absent lanes and the step past the run carry NaN, which fails the presence test
  float u = nan, v = nan, w = nan, m = 0.f;
  if (col) {
    const size_t i = f3d_row(g, y, z_begin) + x;
    u = du[i];
    v = dv[i];
    w = dw[i];
    if (WEIGHT) m = weight[i];
  }
  for (int z = z_begin; z < z_end; ++z) {
    float nu = nan, nv = nan, nw = nan, nm = 0.f;
    if (col && z + 1 < z_end) {
      const size_t i = f3d_row(g, y, z + 1) + x;
      nu = du[i];
      nv = dv[i];
      nw = dw[i];
      if (WEIGHT) nm = weight[i];
    }
    bool present = !(isnan(u) || isnan(v) || isnan(w));
    if (WEIGHT) present = present && m >= weight_min;  // a NaN weight fails the comparison
    if (present) {
      const int z2 = 2 * z - (g.D - 1);
      const double Z = 0.5 * static_cast<double>(z2);  // exact
      const double a = static_cast<double>(u), b = static_cast<double>(v), c = static_cast<double>(w);
      ++cnt;
      sz2 += z2;
      szz4 += static_cast<long long>(z2) * z2;
      su += a;
      sv += b;
      sw += c;
      zu += Z * a;
      zv += Z * b;
      zw += Z * c;
      uu += a * a;
      vv += b * b;
      ww += c * c;
    }
    u = nu;
    v = nv;
    w = nw;
    m = nm;
  }

  // the column's constant doubled x and y come in once per run (a lane without a column has counted nothing)
  const long long x2 = 2 * x - (g.W - 1), y2 = 2 * y - (g.H - 1);
  const double X = 0.5 * static_cast<double>(x2), Y = 0.5 * static_cast<double>(y2);
  const long long n = cnt;
  MotionPartial p;
  p.n = wave_sum_i64(n);
  p.x2[0] = wave_sum_i64(x2 * n);
  p.x2[1] = wave_sum_i64(y2 * n);
  p.x2[2] = wave_sum_i64(sz2);
  p.xx4[0] = wave_sum_i64(x2 * x2 * n);
  p.xx4[1] = wave_sum_i64(y2 * y2 * n);
  p.xx4[2] = wave_sum_i64(szz4);
  p.xx4[3] = wave_sum_i64(x2 * y2 * n);
  p.xx4[4] = wave_sum_i64(x2 * sz2);
  p.xx4[5] = wave_sum_i64(y2 * sz2);
  p.d[0] = wave_sum(su);
  p.d[1] = wave_sum(sv);
  p.d[2] = wave_sum(sw);
  p.xd[0] = wave_sum(X * su);
  p.xd[1] = wave_sum(X * sv);
  p.xd[2] = wave_sum(X * sw);
  p.xd[3] = wave_sum(Y * su);
  p.xd[4] = wave_sum(Y * sv);
  p.xd[5] = wave_sum(Y * sw);
  p.xd[6] = wave_sum(zu);
  p.xd[7] = wave_sum(zv);
  p.xd[8] = wave_sum(zw);
  p.dd[0] = wave_sum(uu);
  p.dd[1] = wave_sum(vv);
  p.dd[2] = wave_sum(ww);
  block_partial<MotionPartial, kBY>(p, partials);
}

struct ResidualPartial {
  unsigned long long present;
  double sum_sq;
  float max_abs, pad;

  static __device__ __forceinline__ ResidualPartial identity() { return {0ull, 0.0, -INFINITY, 0.f}; }
  __device__ __forceinline__ void merge(const ResidualPartial& q)
  {
    present += q.present;
    sum_sq += q.sum_sq;
    max_abs = fmaxf(max_abs, q.max_abs);
  }
};

struct MotionFitArg {
  double centre[3], t[3], M[9];
};

// include/f3d.h, f3d_remove_motion.  out_* may be the inputs themselves (a lane reads its voxel before it writes it), so nothing
// here is __restrict__.
template <bool STATS>
__global__ __launch_bounds__(kBX* kBY) void k_remove_motion(const float* du, const float* dv, const float* dw, float* out_u,
                                                            float* out_v, float* out_w, MotionFitArg fit, F3dGeo g,
                                                            ResidualPartial* partials)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const bool col = x < g.W && y < g.H;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const float nan = __builtin_nanf("");

  // the part of M (x - centre) that does not change along the run: the same operations on the same values give the same bits
  const double X = static_cast<double>(x) - fit.centre[0], Y = static_cast<double>(y) - fit.centre[1];
  const double a0 = fit.M[0] * X + fit.M[1] * Y;
  const double a1 = fit.M[3] * X + fit.M[4] * Y;
  const double a2 = fit.M[6] * X + fit.M[7] * Y;

  ResidualPartial sum = ResidualPartial::identity();
  float u = nan, v = nan, w = nan;
  if (col) {
    const size_t i = f3d_row(g, y, z_begin) + x;
    u = du[i];
    v = dv[i];
    w = dw[i];
  }
  for (int z = z_begin; z < z_end; ++z) {
    float nu = nan, nv = nan, nw = nan;
    if (col && z + 1 < z_end) {
      const size_t i = f3d_row(g, y, z + 1) + x;
      nu = du[i];
      nv = dv[i];
      nw = dw[i];
    }
    const double Z = static_cast<double>(z) - fit.centre[2];
    const float ru = static_cast<float>(static_cast<double>(u) - (fit.t[0] + (a0 + fit.M[2] * Z)));
    const float rv = static_cast<float>(static_cast<double>(v) - (fit.t[1] + (a1 + fit.M[5] * Z)));
    const float rw = static_cast<float>(static_cast<double>(w) - (fit.t[2] + (a2 + fit.M[8] * Z)));
    if (col) {
      const size_t i = f3d_row(g, y, z) + x;
      out_u[i] = ru;
      out_v[i] = rv;
      out_w[i] = rw;
      if (STATS && !(isnan(ru) || isnan(rv) || isnan(rw))) {
        ++sum.present;
        sum.sum_sq += static_cast<double>(ru) * static_cast<double>(ru);
        sum.sum_sq += static_cast<double>(rv) * static_cast<double>(rv);
        sum.sum_sq += static_cast<double>(rw) * static_cast<double>(rw);
        sum.max_abs = fmaxf(sum.max_abs, fmaxf(fmaxf(fabsf(ru), fabsf(rv)), fabsf(rw)));
      }
    }
    u = nu;
    v = nv;
    w = nw;
  }

  if (STATS) {
    sum.present = wave_sum(sum.present);
    sum.sum_sq = wave_sum(sum.sum_sq);
    sum.max_abs = wave_max(sum.max_abs);
    block_partial<ResidualPartial, kBY>(sum, partials);
  }
}

dim3 motion_grid(const F3dGeo& g) { return dim3((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ); }

}  // namespace

extern "C" {

int f3d_motion_sums(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr weight, float weight_min, size_t width, size_t height,
                    size_t depth, struct f3d_motion_sums* out)
{
  F3D_REQUIRE_READY("f3d_motion_sums");
  if (!u || !v || !w) return f3d::fail("f3d_motion_sums: null input");
  if (!out) return f3d::fail("f3d_motion_sums: null out");
  if (weight && weight_min != weight_min) return f3d::fail("f3d_motion_sums: weight_min is NaN");
  if (width == 0 || height == 0 || depth == 0)
    return f3d::fail("f3d_motion_sums: empty volume %zux%zux%zu", width, height, depth);
  // the signed 64-bit sums of doubled coordinates hold for these (include/f3d.h); no device holds more
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > (static_cast<size_t>(1) << 33))
    return f3d::fail("f3d_motion_sums: volume %zux%zux%zu exceeds 32768 along an axis or 2^33 voxels", width, height, depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_motion_sums")) return 1;
  const dim3 grid = motion_grid(g);
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  const float* pm = f3d_ptr<const float>(weight);
  MotionPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](MotionPartial* d_part) {
        if (pm)
          hipLaunchKernelGGL(k_motion_sums<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, pm, weight_min, g, d_part);
        else
          hipLaunchKernelGGL(k_motion_sums<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, pm, weight_min, g, d_part);
      }))
    return 1;
  out->n = static_cast<unsigned long long>(r.n);
  for (int i = 0; i < 3; ++i) out->Sx[i] = 0.5 * static_cast<double>(r.x2[i]);
  for (int i = 0; i < 6; ++i) out->Sxx[i] = 0.25 * static_cast<double>(r.xx4[i]);
  // + 0.0: a sum that is zero is +0 (a lane left of the centre with nothing to add contributes X * +0 = -0)
  for (int i = 0; i < 3; ++i) out->Sd[i] = r.d[i] + 0.0;
  for (int i = 0; i < 9; ++i) out->Sxd[i] = r.xd[i] + 0.0;
  for (int i = 0; i < 3; ++i) out->Sdd[i] = r.dd[i] + 0.0;
  return 0;
}

int f3d_remove_motion(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w,
                      const f3d_motion_fit* fit, size_t width, size_t height, size_t depth, f3d_motion_residual* stats)
{
  F3D_REQUIRE_READY("f3d_remove_motion");
  if (!u || !v || !w) return f3d::fail("f3d_remove_motion: null input");
  if (!out_u || !out_v || !out_w) return f3d::fail("f3d_remove_motion: null output");
  if (!fit) return f3d::fail("f3d_remove_motion: null fit");
  const f3d_devptr in[3] = {u, v, w}, out[3] = {out_u, out_v, out_w};
  static const char* const names[3] = {"u", "v", "w"};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      if (i != j && out[i] == in[j])
        return f3d::fail("f3d_remove_motion: out_%s is the input %s (in place means out_%s == %s)", names[i], names[j], names[i],
                         names[i]);
      if (i < j && out[i] == out[j]) return f3d::fail("f3d_remove_motion: out_%s and out_%s are the same container", names[i], names[j]);
      if (i < j && in[i] == in[j]) return f3d::fail("f3d_remove_motion: %s and %s are the same container", names[i], names[j]);
    }
  MotionFitArg arg;
  for (int i = 0; i < 3; ++i) arg.centre[i] = fit->centre[i];
  for (int i = 0; i < 3; ++i) arg.t[i] = fit->t[i];
  for (int i = 0; i < 9; ++i) arg.M[i] = fit->M[i];
  bool finite = true;
  for (double e : arg.centre) finite = finite && e - e == 0.0;  // false for an infinity and for a NaN
  for (double e : arg.t) finite = finite && e - e == 0.0;
  for (double e : arg.M) finite = finite && e - e == 0.0;
  if (!finite) return f3d::fail("f3d_remove_motion: the fit has an entry of centre, t or M that is not finite");
  if (width == 0 || height == 0 || depth == 0)
    return f3d::fail("f3d_remove_motion: empty volume %zux%zux%zu", width, height, depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_remove_motion")) return 1;
  const dim3 grid = motion_grid(g);
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  float *qu = f3d_ptr<float>(out_u), *qv = f3d_ptr<float>(out_v), *qw = f3d_ptr<float>(out_w);
  if (!stats) {
    hipLaunchKernelGGL(k_remove_motion<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, qu, qv, qw, arg, g, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  ResidualPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](ResidualPartial* d_part) {
        hipLaunchKernelGGL(k_remove_motion<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, qu, qv, qw, arg, g, d_part);
      }))
    return 1;
  stats->present = r.present;
  stats->sum_sq = r.sum_sq;
  stats->max_abs = r.present ? r.max_abs : __builtin_nanf("");
  return 0;
}

}  // extern "C"
