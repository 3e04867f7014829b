// Inverse displacement and field carrying for gfx950: from the displacement d of every voxel of frame 0 (frame 0's grid) the inverse
// g on frame k's grid with g(y) = -d(y + g(y)), by the fixed-point iteration g <- -d(y + g) of each voxel on its own, and the gather
// out(x) = field(x + m(x)) of any field through a displacement, trilinear or nearest neighbour, NaN where the point is outside the
// volume.  The definitions, the lost rules and the evaluation order are those of include/f3d.h (f3d_invert_displacement,
// f3d_carry_field); tests/inverse_ref.py restates them in float32 numpy and matches the kernels bit for bit.
//
// Shape as k_compose_flow (f3d_gather.h): one voxel per lane, a wave64 on 64 consecutive x of one row, a workgroup 4 rows.  The
// iterate of a voxel needs only itself and d, never a neighbour's iterate, so the whole iteration is one launch: every step is one
// compose-like gather (24 loads: 8 corners x 3 components, on the same and the neighbouring rows while displacements are small, served
// by L1/L2), and a voxel stops on its own residual.  A wave leaves the loop when a ballot finds no lane still iterating; lanes outside
// the volume and lost lanes count as stopped.  Stores of g and err are full rows (256 B per wave).
//
// Statistics (optional): each workgroup reduces its voxels into one partial in a buffer of its own; a one-workgroup kernel then folds
// the partials in a fixed order (f3d_partials.h), so the result does not depend on scheduling (no float atomics).
#include "f3d_gather.h"
#include "f3d_partials.h"

namespace {

using namespace f3d_gather;
using namespace f3d_partials;

struct InversePartial {
  unsigned long long defined, unconverged, steps_sum;
  float err_max, pad;

  static __device__ __forceinline__ InversePartial identity() { return {0ull, 0ull, 0ull, -INFINITY, 0.f}; }
  __device__ __forceinline__ void merge(const InversePartial& q)
  {
    defined += q.defined;
    unconverged += q.unconverged;
    steps_sum += q.steps_sum;
    err_max = fmaxf(err_max, q.err_max);
  }
};

// include/f3d.h, f3d_invert_displacement.  err is nullable; partials only with STATS.
template <bool STATS>
__global__ __launch_bounds__(kBX* kBY) void k_invert_displacement(const float* __restrict__ du, const float* __restrict__ dv,
                                                                  const float* __restrict__ dw, float* __restrict__ out_u,
                                                                  float* __restrict__ out_v, float* __restrict__ out_w,
                                                                  float* __restrict__ out_err, F3dGeo g, unsigned iterations,
                                                                  float tolerance, InversePartial* __restrict__ partials)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z = g.z_lo + blockIdx.z;
  const bool in = x < g.W && y < g.H;
  const float xf = static_cast<float>(x), yf = static_cast<float>(y), zf = static_cast<float>(z);

  float gu = 0.f, gv = 0.f, gw = 0.f, e = 0.f;
  unsigned n = 0;
  bool iterating = in, lost = false;
  // every lane of the wave stays in the loop until none iterates (no early return: the ballot and the reductions need them all)
  while (__ballot(iterating)) {
    if (iterating) {
      const float x_f = xf + gu, y_f = yf + gv, z_f = zf + gw;
      if (!inside(g, x_f, y_f, z_f)) {
        lost = true;
        iterating = false;
      } else {
        const Cell c = cell_of(g, x_f, y_f, z_f);
        const float su = trilinear(du, c), sv = trilinear(dv, c), sw = trilinear(dw, c);
        if (isnan(su) || isnan(sv) || isnan(sw)) {
          lost = true;
          iterating = false;
        } else {
          const float eu = gu + su, ev = gv + sv, ew = gw + sw;
          e = fmaxf(fmaxf(fabsf(eu), fabsf(ev)), fabsf(ew));
          if (e <= tolerance || n == iterations) {
            iterating = false;
          } else {
            gu = -su;
            gv = -sv;
            gw = -sw;
            ++n;
          }
        }
      }
    }
  }

  if (in) {
    const float nan = __builtin_nanf("");
    const size_t i = f3d_row(g, y, z) + x;
    out_u[i] = lost ? nan : gu;
    out_v[i] = lost ? nan : gv;
    out_w[i] = lost ? nan : gw;
    if (out_err) out_err[i] = lost ? nan : e;
  }

  if (STATS) {
    const bool def = in && !lost;
    const unsigned long long n_defined = __popcll(__ballot(def));
    const unsigned long long n_unconverged = __popcll(__ballot(def && e > tolerance));
    const unsigned long long steps = wave_sum(static_cast<unsigned long long>(def ? n : 0u));
    const float emax = wave_max(def ? e : -INFINITY);
    block_partial<InversePartial, kBY>({n_defined, n_unconverged, steps, emax, 0.f}, partials);
  }
}

// include/f3d.h, f3d_carry_field: out(x) = field(x + m(x)); the field travels as its bits, so the nearest mode copies exactly
template <bool NEAREST>
__global__ __launch_bounds__(kBX* kBY) void k_carry_field(const float* __restrict__ field, const float* __restrict__ mu,
                                                          const float* __restrict__ mv, const float* __restrict__ mw,
                                                          float* __restrict__ out, F3dGeo g, unsigned long long* lost)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z = g.z_lo + blockIdx.z;
  bool is_lost = false;
  if (x < g.W && y < g.H) {
    const size_t i = f3d_row(g, y, z) + x;
    const float x_f = static_cast<float>(x) + mu[i];
    const float y_f = static_cast<float>(y) + mv[i];
    const float z_f = static_cast<float>(z) + mw[i];
    float r = __builtin_nanf("");
    if (inside(g, x_f, y_f, z_f)) {
      if (NEAREST) {
        const int xn = min(g.W - 1, static_cast<int>(floorf(x_f + 0.5f)));
        const int yn = min(g.H - 1, static_cast<int>(floorf(y_f + 0.5f)));
        const int zn = min(g.D - 1, static_cast<int>(floorf(z_f + 0.5f)));
        r = field[f3d_row(g, yn, zn) + xn];
      } else {
        r = trilinear(field, cell_of(g, x_f, y_f, z_f));
      }
    }
    is_lost = isnan(r);
    out[i] = r;
  }
  count_lost(lost, is_lost);
}

}  // namespace

extern "C" {

int f3d_invert_displacement(f3d_devptr d_u, f3d_devptr d_v, f3d_devptr d_w, f3d_devptr g_u, f3d_devptr g_v, f3d_devptr g_w,
                            f3d_devptr err, size_t width, size_t height, size_t depth, unsigned iterations, float tolerance,
                            f3d_inverse_stats* stats)
{
  F3D_REQUIRE_READY("f3d_invert_displacement");
  if (!d_u || !d_v || !d_w) return f3d::fail("f3d_invert_displacement: null input");
  if (!g_u || !g_v || !g_w) return f3d::fail("f3d_invert_displacement: null output (g_u, g_v and g_w are all required)");
  static const char* const names[4] = {"g_u", "g_v", "g_w", "err"};
  const f3d_devptr outs[4] = {g_u, g_v, g_w, err};
  float* q[4];
  if (!f3d::select_outputs("f3d_invert_displacement", "every step gathers from the inputs", q, outs, 4, names, nullptr, 0, d_u, d_v,
                           d_w))
    return 1;
  if (iterations < 1 || iterations > 64)
    return f3d::fail("f3d_invert_displacement: iterations must be 1 .. 64 (got %u)", iterations);
  if (!(tolerance >= 0.f)) return f3d::fail("f3d_invert_displacement: tolerance must be a number >= 0 (got %g)", tolerance);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_invert_displacement")) return 1;
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, g.z_hi - g.z_lo);
  const float *pu = f3d_ptr<const float>(d_u), *pv = f3d_ptr<const float>(d_v), *pw = f3d_ptr<const float>(d_w);
  if (!stats) {
    if (g.z_hi > g.z_lo) {
      hipLaunchKernelGGL(k_invert_displacement<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, q[0], q[1], q[2], q[3], g,
                         iterations, tolerance, nullptr);
      F3D_HIP(hipGetLastError());
    }
    return 0;
  }
  InversePartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](InversePartial* d_part) {
        hipLaunchKernelGGL(k_invert_displacement<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, q[0], q[1], q[2], q[3],
                           g, iterations, tolerance, d_part);
      }))
    return 1;
  stats->defined = r.defined;
  stats->unconverged = r.unconverged;
  stats->steps_sum = r.steps_sum;
  stats->err_max = r.defined ? r.err_max : __builtin_nanf("");
  return 0;
}

int f3d_carry_field(f3d_devptr field, f3d_devptr m_u, f3d_devptr m_v, f3d_devptr m_w, f3d_devptr out, size_t width, size_t height,
                    size_t depth, unsigned mode, unsigned long long* lost)
{
  F3D_REQUIRE_READY("f3d_carry_field");
  if (!field || !m_u || !m_v || !m_w || !out) return f3d::fail("f3d_carry_field: null argument");
  if (mode != F3D_CARRY_LINEAR && mode != F3D_CARRY_NEAREST)
    return f3d::fail("f3d_carry_field: mode must be F3D_CARRY_LINEAR or F3D_CARRY_NEAREST (got %u)", mode);
  if (out == field || out == m_u || out == m_v || out == m_w)
    return f3d::fail("f3d_carry_field: out is also an input (the gather reads other voxels)");
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_carry_field")) return 1;
  unsigned long long* d_lost;
  if (lost_zero(lost, &d_lost)) return 1;
  if (g.z_hi > g.z_lo) {
    const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, g.z_hi - g.z_lo);
    const float *pf = f3d_ptr<const float>(field), *pu = f3d_ptr<const float>(m_u), *pv = f3d_ptr<const float>(m_v),
                *pw = f3d_ptr<const float>(m_w);
    if (mode == F3D_CARRY_NEAREST)
      hipLaunchKernelGGL(k_carry_field<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pf, pu, pv, pw, f3d_ptr<float>(out), g,
                         d_lost);
    else
      hipLaunchKernelGGL(k_carry_field<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pf, pu, pv, pw, f3d_ptr<float>(out), g,
                         d_lost);
    F3D_HIP(hipGetLastError());
  }
  return lost_read(lost, d_lost);
}

}  // extern "C"
