// Per-voxel match quality of two volumes on one grid for gfx950: over the (2r+1)^3 window of every voxel the zero-normalised
// cross-correlation and the RMS difference, from seven window sums formed separably (x, then y, then z) in binary64 with NaN
// samples left out.  The definition, the order of every addition and the float32 tail are those of include/f3d.h
// (f3d_local_correlation); tests/correlation_ref.py restates them in numpy and matches the kernel bit for bit.
//
// Shape: a workgroup of 256 threads owns a tile of kTX x kTY voxels of a plane and marches in z over a run of kZ planes, primed with
// 2r planes.  Per plane:
//   1. the samples of the tile plus an r-wide halo, (kTX + 2r) x (kTY + 2r) pairs (a, b), go through registers into LDS -- they were
//      loaded a step ahead, so their HBM latency overlaps the step before; a point outside the volume is stored as NaN, which makes
//      it absent, and an absent point adds +0 to every sum;
//   2. x sums: a thread takes two neighbouring x of one of the kTY + 2r rows, forms the quantities of the 2r + 2 points they span once
//      and adds each window in ascending x; the sums go back to LDS;
//   3. y sums: every thread adds the 2r + 1 rows of its own column in ascending y and keeps the plane's sums in a register ring of
//      2r + 1 planes (the march is unrolled over the ring, so every index is static);
//   4. z sums: once the ring is full the thread adds its planes in ascending z and finishes the voxel r planes back.
// Nothing is carried from voxel to voxel (no running add / subtract), so a result does not depend on where a march started.  The
// count of present voxels is kept in integers: it is exact in either form.
// Redundancy: the x sums are formed for (kTY + 2r) / kTY of the rows (1.25 ... 2) and the priming adds 2r / kZ planes
// (0.06 ... 0.25); the halo columns are loaded (kTX + 2r) / kTX times, mostly out of L2.  A 32 x 16 tile of 512 threads halves the
// extra rows and measured half as fast again at r = 3: the two barriers of a step stall a workgroup, and what hides that is other
// workgroups on the CU, of which the registers of the ring allow two or three at 256 threads and one at 512.
//
// Statistics (optional): each workgroup reduces its voxels into one partial in a buffer of its own; a one-workgroup kernel then folds
// the partials in a fixed order (f3d_partials.h), so the result does not depend on scheduling (no float atomics).
#include <utility>

#include "f3d_partials.h"

namespace {

using namespace f3d_partials;

constexpr int kTX = 32;  // tile of a plane
constexpr int kTY = 8;
constexpr int kZ = 32;   // planes of a run
constexpr int kWaves = kTX * kTY / 64;

struct CorrelationPartial {
  unsigned long long defined, lost, below;
  float zncc_min, rmsd_max;
  double zncc_sum;

  static __device__ __forceinline__ CorrelationPartial identity() { return {0ull, 0ull, 0ull, INFINITY, -INFINITY, 0.0}; }
  __device__ __forceinline__ void merge(const CorrelationPartial& q)
  {
    defined += q.defined;
    lost += q.lost;
    below += q.below;
    zncc_min = fminf(zncc_min, q.zncc_min);
    rmsd_max = fmaxf(rmsd_max, q.rmsd_max);
    zncc_sum += q.zncc_sum;
  }
};

// the quantities of one point that are summed in binary64 (the count travels as an integer): A, B, A*A, B*B, A*B and, with DD,
// (A - B) * (A - B); all +0 when the point is absent
template <bool DD>
struct Quantities {
  static constexpr int kCount = DD ? 6 : 5;
  double q[kCount];

  __device__ __forceinline__ void of(float a, float b, bool present)
  {
    const double A = present ? static_cast<double>(a) : 0.0;
    const double B = present ? static_cast<double>(b) : 0.0;
    q[0] = A;
    q[1] = B;
    q[2] = A * A;
    q[3] = B * B;
    q[4] = A * B;
    if (DD) {
      const double d = A - B;
      q[kCount - 1] = d * d;
    }
  }
};

// step(integral_constant<P>) for P = 0, 1, ... until one returns false.  The march is unrolled over the ring this way, not by a
// pragma (which the optimizer declines at r = 4, leaving the ring in scratch): P is a constant in each copy of the step.
template <typename Step, int... P>
__device__ __forceinline__ bool ring_steps(Step& step, std::integer_sequence<int, P...>)
{
  return (step(std::integral_constant<int, P>{}) && ...);
}

// include/f3d.h, f3d_local_correlation.  R: the radius; DD: the RMS difference is wanted (stored, or for the statistics); out_zncc and
// out_rmsd are nullable (out_rmsd only with DD); partials only with STATS.
template <int R, bool DD, bool STATS>
__global__ __launch_bounds__(kTX* kTY) void k_local_correlation(const float* __restrict__ a, const float* __restrict__ b,
                                                                float* __restrict__ out_zncc, float* __restrict__ out_rmsd,
                                                                F3dGeo g, float threshold,
                                                                CorrelationPartial* __restrict__ partials)
{
  constexpr int kRing = 2 * R + 1;
  constexpr int kLX = kTX + 2 * R, kLY = kTY + 2 * R;  // the tile with its halo
  constexpr int kThreads = kTX * kTY;
  constexpr int kLoads = (kLX * kLY + kThreads - 1) / kThreads;  // points of the haloed tile per thread
  constexpr int kNQ = Quantities<DD>::kCount;
  constexpr int kCentre = 1 << 16;  // in x_count: the row's own point is present

  __shared__ float2 ab[kLY * kLX];
  __shared__ double x_sum[kNQ][kLY][kTX];
  __shared__ int x_count[kLY][kTX];

  const int tid = threadIdx.y * 64 + threadIdx.x;
  const int tx = tid % kTX, ty = tid / kTX;
  const int x = blockIdx.x * kTX + tx, y = blockIdx.y * kTY + ty;
  const bool owner = x < g.W && y < g.H;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const int steps = z_end - z_begin + 2 * R;  // step s handles plane z_begin - R + s

  // this thread's points of the haloed tile: the offset inside a plane, or -1 outside the volume
  long long load_at[kLoads];
#pragma unroll
  for (int l = 0; l < kLoads; ++l) {
    const int i = tid + l * kThreads;
    const int px = blockIdx.x * kTX - R + i % kLX, py = blockIdx.y * kTY - R + i / kLX;
    const bool in = i < kLX * kLY && px >= 0 && px < g.W && py >= 0 && py < g.H;
    load_at[l] = in ? static_cast<long long>(py) * g.pitch + px : -1;
  }
  float2 next[kLoads];
  auto load_plane = [&](int z) {
    const bool plane = z >= 0 && z < g.D;
    const size_t base = plane ? f3d_row(g, 0, z) : 0;
#pragma unroll
    for (int l = 0; l < kLoads; ++l) {
      const float nan = __builtin_nanf("");
      next[l] = make_float2(nan, nan);
      if (plane && load_at[l] >= 0) {
        next[l].x = a[base + load_at[l]];
        next[l].y = b[base + load_at[l]];
      }
    }
  };

  double ring[kRing][kNQ];  // the y sums of the newest 2r + 1 planes, plane of step s in slot s % kRing
  int ring_count[kRing];
  unsigned centres = 0;     // bit k: this thread's own point k planes back is present
  CorrelationPartial sum = CorrelationPartial::identity();

  load_plane(z_begin - R);
  for (int first = 0; first < steps; first += kRing) {
    auto step = [&](auto slot_of_step) __attribute__((always_inline)) {
      constexpr int p = decltype(slot_of_step)::value;
      const int s = first + p;
      if (s >= steps) return false;  // the same for the whole workgroup
      const int z = z_begin - R + s;

      // 1. the plane's samples into LDS; the next plane's on their way
#pragma unroll
      for (int l = 0; l < kLoads; ++l)
        if (tid + l * kThreads < kLX * kLY) ab[tid + l * kThreads] = next[l];
      if (s + 1 < steps) load_plane(z + 1);
      __syncthreads();

      // 2. x sums of two neighbouring points of one row
      if (tid < kLY * kTX / 2) {
        const int row = tid / (kTX / 2), xp = (tid % (kTX / 2)) * 2;
        double s0[kNQ], s1[kNQ];
        int n0 = 0, n1 = 0, centre0 = 0, centre1 = 0;
#pragma unroll
        for (int i = 0; i < kRing + 1; ++i) {
          const float2 v = ab[row * kLX + xp + i];
          const bool present = !(isnan(v.x) || isnan(v.y));
          Quantities<DD> t;
          t.of(v.x, v.y, present);
          if (i < kRing) n0 += present ? 1 : 0;
          if (i > 0) n1 += present ? 1 : 0;
          if (i == R) centre0 = present ? kCentre : 0;
          if (i == R + 1) centre1 = present ? kCentre : 0;
#pragma unroll
          for (int j = 0; j < kNQ; ++j) {
            if (i == 0) s0[j] = t.q[j];
            else if (i < kRing) s0[j] += t.q[j];
            if (i == 1) s1[j] = t.q[j];
            else if (i > 1) s1[j] += t.q[j];
          }
        }
#pragma unroll
        for (int j = 0; j < kNQ; ++j) {
          x_sum[j][row][xp] = s0[j];
          x_sum[j][row][xp + 1] = s1[j];
        }
        x_count[row][xp] = n0 | centre0;
        x_count[row][xp + 1] = n1 | centre1;
      }
      __syncthreads();

      // 3. y sums of this thread's column into the ring (the next step writes x_sum only behind its first barrier)
      {
        int n = 0;
#pragma unroll
        for (int dy = 0; dy < kRing; ++dy) n += x_count[ty + dy][tx] & (kCentre - 1);
        ring_count[p] = n;
        centres = (centres << 1) | (x_count[ty + R][tx] >= kCentre ? 1u : 0u);
#pragma unroll
        for (int j = 0; j < kNQ; ++j) {
          double t = x_sum[j][ty][tx];
#pragma unroll
          for (int dy = 1; dy < kRing; ++dy) t += x_sum[j][ty + dy][tx];
          ring[p][j] = t;
        }
      }

      // 4. the voxel r planes back: z sums oldest plane first, then the float32 tail
      if (s >= 2 * R) {
        int count = 0;
        double S[kNQ];
#pragma unroll
        for (int k = 0; k < kRing; ++k) {
          const int slot = (p + 1 + k) % kRing;
          count += ring_count[slot];
#pragma unroll
          for (int j = 0; j < kNQ; ++j) {
            if (k == 0) S[j] = ring[slot][j];
            else S[j] += ring[slot][j];
          }
        }
        const bool present = (centres >> R) & 1u;
        float zncc = __builtin_nanf(""), rmsd = __builtin_nanf("");
        if (present) {
          const double n = static_cast<double>(count);
          const double Sa = S[0], Sb = S[1], Saa = S[2], Sbb = S[3], Sab = S[4];
          if (DD) rmsd = sqrtf(static_cast<float>(S[kNQ - 1]) / static_cast<float>(n));
          const double nSaa = n * Saa, nSbb = n * Sbb;
          const double va = nSaa - Sa * Sa;
          const double vb = nSbb - Sb * Sb;
          const double c = n * Sab - Sa * Sb;
          const bool flat = !(va > 0x1p-40 * nSaa) || !(vb > 0x1p-40 * nSbb);
          if (!flat) zncc = static_cast<float>(c) / (sqrtf(static_cast<float>(va)) * sqrtf(static_cast<float>(vb)));
        }
        if (owner) {
          const size_t i = f3d_row(g, y, z - R) + x;
          if (out_zncc) out_zncc[i] = zncc;
          if (DD && out_rmsd) out_rmsd[i] = rmsd;
          if (STATS) {
            if (!present) {
              ++sum.lost;
            } else {
              sum.rmsd_max = fmaxf(sum.rmsd_max, rmsd);
              if (!isnan(zncc)) {
                ++sum.defined;
                sum.below += zncc < threshold ? 1 : 0;
                sum.zncc_min = fminf(sum.zncc_min, zncc);
                sum.zncc_sum += static_cast<double>(zncc);
              }
            }
          }
        }
      }
      return true;
    };
    ring_steps(step, std::make_integer_sequence<int, kRing>{});
  }

  if (STATS) {
    sum.defined = wave_sum(sum.defined);
    sum.lost = wave_sum(sum.lost);
    sum.below = wave_sum(sum.below);
    sum.zncc_min = wave_min(sum.zncc_min);
    sum.rmsd_max = wave_max(sum.rmsd_max);
    sum.zncc_sum = wave_sum(sum.zncc_sum);
    block_partial<CorrelationPartial, kWaves>(sum, partials);
  }
}

template <int R>
int launch(const float* a, const float* b, float* zncc, float* rmsd, const F3dGeo& g, float threshold, f3d_correlation_stats* stats)
{
  const dim3 grid((g.W + kTX - 1) / kTX, (g.H + kTY - 1) / kTY, (g.D + kZ - 1) / kZ), block(64, kWaves, 1);
  if (!stats) {
    if (rmsd)
      hipLaunchKernelGGL((k_local_correlation<R, true, false>), grid, block, 0, f3d::stream(), a, b, zncc, rmsd, g, threshold, nullptr);
    else
      hipLaunchKernelGGL((k_local_correlation<R, false, false>), grid, block, 0, f3d::stream(), a, b, zncc, rmsd, g, threshold, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  CorrelationPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](CorrelationPartial* d_part) {
        hipLaunchKernelGGL((k_local_correlation<R, true, true>), grid, block, 0, f3d::stream(), a, b, zncc, rmsd, g, threshold, d_part);
      }))
    return 1;
  const size_t voxels = static_cast<size_t>(g.W) * g.H * g.D;
  stats->defined = r.defined;
  stats->lost = r.lost;
  stats->below = r.below;
  stats->zncc_min = r.defined ? r.zncc_min : __builtin_nanf("");
  stats->rmsd_max = r.lost < voxels ? r.rmsd_max : __builtin_nanf("");
  stats->zncc_sum = r.zncc_sum;
  return 0;
}

}  // namespace

extern "C" {

int f3d_local_correlation(f3d_devptr a, f3d_devptr b, const f3d_devptr out[2], unsigned fields, unsigned radius, float threshold,
                          size_t width, size_t height, size_t depth, f3d_correlation_stats* stats)
{
  F3D_REQUIRE_READY("f3d_local_correlation");
  if (!a || !b) return f3d::fail("f3d_local_correlation: null input");
  if (fields == 0 || (fields & ~(F3D_CORRELATION_ZNCC | F3D_CORRELATION_RMSD)))
    return f3d::fail("f3d_local_correlation: fields must be a non-empty combination of F3D_CORRELATION_ZNCC, F3D_CORRELATION_RMSD "
                     "(got %u)", fields);
  if (!out) return f3d::fail("f3d_local_correlation: null output array");
  if (radius < 1 || radius > 4) return f3d::fail("f3d_local_correlation: radius must be 1 .. 4 (got %u)", radius);
  if (threshold != threshold) return f3d::fail("f3d_local_correlation: threshold is NaN");
  static const char* const names[2] = {"zncc", "rmsd"};
  static const unsigned groups[2] = {F3D_CORRELATION_ZNCC, F3D_CORRELATION_RMSD};
  float* o[2];
  if (!f3d::select_outputs("f3d_local_correlation", "the window reads neighbours", o, out, 2, names, groups, fields, a, b, b)) return 1;
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_local_correlation")) return 1;
  const float *pa = f3d_ptr<const float>(a), *pb = f3d_ptr<const float>(b);
  switch (radius) {
    case 1: return launch<1>(pa, pb, o[0], o[1], g, threshold, stats);
    case 2: return launch<2>(pa, pb, o[0], o[1], g, threshold, stats);
    case 3: return launch<3>(pa, pb, o[0], o[1], g, threshold, stats);
    default: return launch<4>(pa, pb, o[0], o[1], g, threshold, stats);
  }
}

}  // extern "C"
