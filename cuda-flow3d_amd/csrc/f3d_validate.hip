// Validation of a displacement for gfx950: the normalised median test (Westerweel & Scarano 2005) over the up to 26 neighbours
// `step` voxels away, with the rejected vectors set to NaN or replaced by the neighbour median (f3d_validate_displacement).  The
// definition, the presence rule and the classes are those of include/f3d.h; tests/outlier_ref.py restates them in numpy and every
// stored value matches it bit for bit.
//
// Shape: the derived-field skeleton.  A wave on 64 consecutive x of one row, a workgroup kBY rows, a lane marching in z over a run of
// kZ planes of its own column.  For any step the 27 reads of a lane are row-contiguous across the wave.
//
// Per voxel: one pass over the 26 neighbours loads u, v, w (and the weight) and leaves a 26-bit presence mask and the u list; the v
// and w lists are loaded again under the mask (they hit the cache: the pass before has just touched the same lines).  An absent
// neighbour is +inf, so after sort26 the k present values are s_0 .. s_{k-1} for any k and no NaN ever enters a min or max.  Two
// observations save the second sort of each component (only the multiset of the residuals matters):
//   1. |s_i - med| over the sorted list is the same multiset as over the neighbours in any order, and the +inf pads stay +inf;
//   2. that list falls and then rises (float subtraction is monotonic), so one bitonic merger orders it, and only ranks 0 .. 13 of
//      it can be the median of at most 26 values (vmerge26, pruned to them).
// The median of k values is picked from the ranks by a chain of selects on k (k differs between lanes; an indexed register array
// would go to scratch).  No LDS beyond the skeleton's, no scratch, no AGPRs.
//
// Built WITHOUT -fno-honor-nans (the Makefile's MEDIAN_FLAGS): presence is a test for NaN.
#include "f3d_internal.h"
#include "f3d_partials.h"
#include "f3d_validate_nets.h"

namespace {

using namespace f3d_partials;

constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;

struct ValidatePartial {
  unsigned long long present, tested, outliers, replaced, undefined;
  float r_max, pad;

  static __device__ __forceinline__ ValidatePartial identity() { return {0ull, 0ull, 0ull, 0ull, 0ull, -INFINITY, 0.f}; }
  __device__ __forceinline__ void merge(const ValidatePartial& q)
  {
    present += q.present;
    tested += q.tested;
    outliers += q.outliers;
    replaced += q.replaced;
    undefined += q.undefined;
    r_max = fmaxf(r_max, q.r_max);
  }
};

// rank i of the ranks s0 .. s13 (i differs between the lanes of a wave: a chain of selects, since an indexed register array would go
// to scratch; the ranks come as values because a select between loads of an array is turned into a load of a selected address)
__device__ __forceinline__ float pick14(float s0, float s1, float s2, float s3, float s4, float s5, float s6, float s7, float s8,
                                        float s9, float s10, float s11, float s12, float s13, int i)
{
  float r = s0;
  r = i == 1 ? s1 : r;
  r = i == 2 ? s2 : r;
  r = i == 3 ? s3 : r;
  r = i == 4 ? s4 : r;
  r = i == 5 ? s5 : r;
  r = i == 6 ? s6 : r;
  r = i == 7 ? s7 : r;
  r = i == 8 ? s8 : r;
  r = i == 9 ? s9 : r;
  r = i == 10 ? s10 : r;
  r = i == 11 ? s11 : r;
  r = i == 12 ? s12 : r;
  r = i == 13 ? s13 : r;
  return r;
}

// the median of s_0 .. s_{k-1} by the rule of include/f3d.h, k in 1 .. 26 (0 for k == 0: nothing reads it); N >= 14
template <int N>
__device__ __forceinline__ float median_of(const float (&s)[N], int k)
{
  const float hi = pick14(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], s[13], k >> 1);
  const float lo = pick14(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], s[13], max(k - 1, 0) >> 1);
  const float med = (k & 1) ? hi : 0.5f * (lo + hi);
  return k ? med : 0.f;
}

// one component: v holds the neighbours' values with +inf for an absent one; gives the neighbour median and the median residual
__device__ __forceinline__ void median_and_residual(const float (&v)[26], int k, float* med_out, float* rm_out)
{
  float s[26];
  sort26(v, s);
  const float med = median_of(s, k);
  float a[26];
#pragma unroll
  for (int i = 0; i < 26; ++i) a[i] = fabsf(s[i] - med);  // falls to the median, rises after it; inf - med = inf
  float ranks[14];
  vmerge26(a, ranks);
  *med_out = med;
  *rm_out = median_of(ranks, k);
}

struct ValidateArg {
  float weight_min, eps, threshold;
  int step, min_neighbours;
  bool replace;
};

// include/f3d.h, f3d_validate_displacement.  The outputs are never the inputs (the entry refuses it); a null output is not stored.
template <bool WEIGHT, bool STATS>
__global__ __launch_bounds__(kBX* kBY) void k_validate(const float* __restrict__ du, const float* __restrict__ dv,
                                                       const float* __restrict__ dw, const float* __restrict__ weight,
                                                       ValidateArg arg, float* __restrict__ out_r, float* __restrict__ out_u,
                                                       float* __restrict__ out_v, float* __restrict__ out_w, F3dGeo g,
                                                       ValidatePartial* __restrict__ partials)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const bool col = x < g.W && y < g.H;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const float nan = __builtin_nanf("");
  const int step = arg.step;

  ValidatePartial sum = ValidatePartial::identity();
  if (col) {
    // the in-plane part of the neighbour offsets does not change along the run
    bool in_x[3], in_y[3];
    int nx[3], ny[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      nx[i] = x + (i - 1) * step;
      ny[i] = y + (i - 1) * step;
      in_x[i] = nx[i] >= 0 && nx[i] < g.W;
      in_y[i] = ny[i] >= 0 && ny[i] < g.H;
    }
    for (int z = z_begin; z < z_end; ++z) {
      const size_t at = f3d_row(g, y, z) + x;
      const float u = du[at], v = dv[at], w = dw[at];
      bool present = !(isnan(u) || isnan(v) || isnan(w));
      if (WEIGHT) present = present && weight[at] >= arg.weight_min;  // a NaN weight fails the comparison

      // neighbour n = 9 (k+1) + 3 (j+1) + (i+1) without the centre: presence mask and the u list
      unsigned mask = 0;
      float list[26];
      {
#pragma unroll
        for (int dz = 0; dz < 3; ++dz) {
          const int nz = z + (dz - 1) * step;
          const bool in_z = nz >= 0 && nz < g.D;
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
              const int cell = 9 * dz + 3 * dy + dx, n = cell < 13 ? cell : cell - 1;
              if (cell == 13) continue;
              bool there = in_z && in_y[dy] && in_x[dx];
              float a = INFINITY;
              if (there) {
                const size_t i = f3d_row(g, ny[dy], nz) + nx[dx];
                a = du[i];
                const float b = dv[i], c = dw[i];
                there = !(isnan(a) || isnan(b) || isnan(c));
                if (WEIGHT) there = there && weight[i] >= arg.weight_min;
              }
              list[n] = there ? a : INFINITY;
              mask |= (there ? 1u : 0u) << n;
            }
        }
      }
      const int k = __popc(mask);
      float med_u, med_v, med_w, rm_u, rm_v, rm_w;
      median_and_residual(list, k, &med_u, &rm_u);
      // v and w: the same neighbours under the mask (a set bit says the neighbour is inside the volume)
      auto gather = [&](const float* __restrict__ d) {
#pragma unroll
        for (int dz = 0; dz < 3; ++dz) {
          const int nz = z + (dz - 1) * step;
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
              const int cell = 9 * dz + 3 * dy + dx, n = cell < 13 ? cell : cell - 1;
              if (cell == 13) continue;
              float a = INFINITY;
              if ((mask >> n) & 1u) a = d[f3d_row(g, ny[dy], nz) + nx[dx]];
              list[n] = a;
            }
        }
      };
      gather(dv);
      median_and_residual(list, k, &med_v, &rm_v);
      gather(dw);
      median_and_residual(list, k, &med_w, &rm_w);

      const float r_u = fabsf(u - med_u) / (rm_u + arg.eps);
      const float r_v = fabsf(v - med_v) / (rm_v + arg.eps);
      const float r_w = fabsf(w - med_w) / (rm_w + arg.eps);
      const float r = fmaxf(fmaxf(r_u, r_v), r_w);
      const bool enough = k >= arg.min_neighbours;
      const bool tested = present && enough;
      const bool outlier = tested && r > arg.threshold;
      const bool kept = present && !outlier;
      const bool median = !kept && arg.replace && enough;
      // + 0.f: a zero median is stored as +0 (which of several zeros of mixed sign the network leaves in the middle is not defined)
      const float o_u = kept ? u : (median ? med_u + 0.f : nan);
      const float o_v = kept ? v : (median ? med_v + 0.f : nan);
      const float o_w = kept ? w : (median ? med_w + 0.f : nan);
      if (out_r) out_r[at] = tested ? r : nan;
      if (out_u) {
        out_u[at] = o_u;
        out_v[at] = o_v;
        out_w[at] = o_w;
      }
      if (STATS) {
        sum.present += present ? 1 : 0;
        sum.tested += tested ? 1 : 0;
        sum.outliers += outlier ? 1 : 0;
        sum.replaced += median ? 1 : 0;
        sum.undefined += !(kept || median) ? 1 : 0;  // the validated u is NaN exactly there
        if (tested) sum.r_max = fmaxf(sum.r_max, r);
      }
    }
  }

  if (STATS) {
    sum.present = wave_sum(sum.present);
    sum.tested = wave_sum(sum.tested);
    sum.outliers = wave_sum(sum.outliers);
    sum.replaced = wave_sum(sum.replaced);
    sum.undefined = wave_sum(sum.undefined);
    sum.r_max = wave_max(sum.r_max);
    block_partial<ValidatePartial, kBY>(sum, partials);
  }
}

template <bool WEIGHT>
int launch(const float* pu, const float* pv, const float* pw, const float* pm, const ValidateArg& arg, float* const (&o)[4],
           const F3dGeo& g, f3d_validate_stats* stats)
{
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ), block(kBX, kBY, 1);
  if (!stats) {
    hipLaunchKernelGGL((k_validate<WEIGHT, false>), grid, block, 0, f3d::stream(), pu, pv, pw, pm, arg, o[0], o[1], o[2], o[3], g,
                       nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  ValidatePartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](ValidatePartial* d_part) {
        hipLaunchKernelGGL((k_validate<WEIGHT, true>), grid, block, 0, f3d::stream(), pu, pv, pw, pm, arg, o[0], o[1], o[2], o[3], g,
                           d_part);
      }))
    return 1;
  stats->present = r.present;
  stats->tested = r.tested;
  stats->outliers = r.outliers;
  stats->replaced = r.replaced;
  stats->undefined = r.undefined;
  stats->r_max = r.tested ? r.r_max : __builtin_nanf("");
  return 0;
}

}  // namespace

extern "C" {

int f3d_validate_displacement(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr weight, float weight_min, unsigned step, float eps,
                              float threshold, unsigned min_neighbours, unsigned mode, const f3d_devptr out[4], unsigned fields,
                              size_t width, size_t height, size_t depth, f3d_validate_stats* stats)
{
  const char* const who = "f3d_validate_displacement";
  F3D_REQUIRE_READY(who);
  if (!u || !v || !w) return f3d::fail("%s: null input", who);
  if (fields == 0 || (fields & ~(F3D_VALIDATE_R | F3D_VALIDATE_D)))
    return f3d::fail("%s: fields must be a non-empty combination of F3D_VALIDATE_R, F3D_VALIDATE_D (got %u)", who, fields);
  if (!out) return f3d::fail("%s: null output array", who);
  if (mode != F3D_VALIDATE_MARK && mode != F3D_VALIDATE_REPLACE)
    return f3d::fail("%s: mode must be F3D_VALIDATE_MARK or F3D_VALIDATE_REPLACE (got %u)", who, mode);
  if (step < 1 || step > 16) return f3d::fail("%s: step must be 1 .. 16 (got %u)", who, step);
  if (min_neighbours < 1 || min_neighbours > 26) return f3d::fail("%s: min_neighbours must be 1 .. 26 (got %u)", who, min_neighbours);
  if (!(eps > 0.f) || eps - eps != 0.f) return f3d::fail("%s: eps must be finite and above 0", who);
  if (!(threshold >= 0.f)) return f3d::fail("%s: threshold is NaN or negative", who);
  if (weight && weight_min != weight_min) return f3d::fail("%s: weight_min is NaN", who);
  static const char* const names[4] = {"r", "u", "v", "w"};
  static const unsigned groups[4] = {F3D_VALIDATE_R, F3D_VALIDATE_D, F3D_VALIDATE_D, F3D_VALIDATE_D};
  float* o[4];
  if (!f3d::select_outputs(who, "the test reads neighbours", o, out, 4, names, groups, fields, u, v, w)) return 1;
  for (int f = 0; f < 4; ++f)
    if (o[f] && weight && out[f] == weight)
      return f3d::fail("%s: output %d (%s) is also the weight (the test reads neighbours)", who, f, names[f]);
  if (width == 0 || height == 0 || depth == 0) return f3d::fail("%s: empty volume %zux%zux%zu", who, width, height, depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, who)) return 1;
  ValidateArg arg;
  arg.weight_min = weight_min;
  arg.eps = eps;
  arg.threshold = threshold;
  arg.step = static_cast<int>(step);
  arg.min_neighbours = static_cast<int>(min_neighbours);
  arg.replace = mode == F3D_VALIDATE_REPLACE;
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  const float* pm = f3d_ptr<const float>(weight);
  return pm ? launch<true>(pu, pv, pw, pm, arg, o, g, stats) : launch<false>(pu, pv, pw, pm, arg, o, g, stats);
}

}  // extern "C"
