// Grey-value histogram and finite value range of a volume for gfx950 (f3d_histogram, f3d_value_range).  The definitions are
// include/f3d.h's, the bin rule and the ordered key of a float are f3d_histogram_bin.h's (the same text the host's bisection runs);
// tests/histogram_ref.py restates them in numpy and every count and counter matches byte for byte.
//
// Everything is an integer function of the input: counts are added with integer atomics, min and max are a max over an ordered integer
// key, so no order has to be fixed and any schedule gives the same bytes.  No float atomic.  No lane ever waits for another lane or
// workgroup: every loop is bounded by the box.
//
// Shape: a wave on 64 consecutive x of one row, a workgroup kBY rows, kZ planes of a 64 x 4 x 32 tile marched kAhead planes at a time
// (their loads are issued together); at most kGroups workgroups, each walking the tiles blockIdx.x, blockIdx.x + gridDim.x, ... so that
// a workgroup flushes once however large the box is.  The workgroup counts in LDS, one 32-bit word per bin (a workgroup sees at most
// 2^27 voxels), and at its end adds every non-zero word to the call's 64-bit accumulator in the library's grow-only buffer.
//
// Contention: tomography frames are mostly two phases, so the lanes of a wave hit one or two words, and LDS atomics on
// one address serialise.  Run merging: the lanes of a wave hold 64 consecutive x; one ballot of "my bin differs from my left
// neighbour's" gives the runs of equal bins, and the first lane of a run adds the run's length.  A constant row is one add per wave
// instead of 64; a ramp along x stays 64 adds to 64 words, which never conflicted.
#include <algorithm>
#include <cmath>

#include "f3d_internal.h"
#define F3D_HIST_FN __host__ __device__ __forceinline__
#include "f3d_histogram_bin.h"

namespace {

using f3d_hist::Rule;

typedef unsigned long long u64;

constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;
constexpr int kAhead = 4;          // planes whose loads are in flight together; divides kZ
constexpr unsigned kGroups = 1024;  // workgroups at most: four per CU
constexpr int kCounters = 8;       // f3d_histogram: the five classes.  f3d_value_range: four classes, then [4] = the two key words
constexpr size_t kMaxVoxels = static_cast<size_t>(1) << 33;

// the tiles of the box in x-fastest order
struct Tiles {
  unsigned nx, ny, count;
};

__device__ __forceinline__ unsigned wave_sum_u(unsigned x)
{
  for (int o = 32; o > 0; o >>= 1) x += static_cast<unsigned>(__shfl_xor(static_cast<int>(x), o));
  return x;
}
__device__ __forceinline__ unsigned wave_max_u(unsigned x)
{
  for (int o = 32; o > 0; o >>= 1) x = max(x, static_cast<unsigned>(__shfl_xor(static_cast<int>(x), o)));
  return x;
}

// A counter of the call goes wave -> workgroup -> device: the wave's sum into the workgroup's tally in LDS (32 bits: a workgroup sees
// at most 2^27 voxels), and after a barrier one global add per workgroup and counter.  With one global add per WAVE and counter (some
// 20 000 adds on a handful of words at 512^3) k_value_range took 0.29 ms there instead of 0.17, k_histogram 0.27 instead of 0.25.
__device__ __forceinline__ void tally_add(unsigned* tally, int lane_count)
{
  const unsigned sum = wave_sum_u(static_cast<unsigned>(lane_count));
  if (threadIdx.x == 0 && sum) __hip_atomic_fetch_add(tally, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Walks the voxels of the workgroup's tiles: voxel(s, m, inside) is called by all 64 lanes of a wave together, `inside` false for a
// lane whose column lies outside the box (s and m are then 0 and were not loaded).  m is the mask word, 1 without a mask.
template <bool MASK, typename Voxel>
__device__ __forceinline__ void walk_tiles(const float* __restrict__ src, const int* __restrict__ mask, const F3dGeo& g, const Tiles& t,
                                           Voxel&& voxel)
{
  for (unsigned tile = blockIdx.x; tile < t.count; tile += gridDim.x) {
    const unsigned bx = tile % t.nx, rest = tile / t.nx;
    const unsigned by = rest % t.ny, bz = rest / t.ny;
    const int x = static_cast<int>(bx) * kBX + static_cast<int>(threadIdx.x);
    const int y = static_cast<int>(by) * kBY + static_cast<int>(threadIdx.y);
    const bool col = x < g.W && y < g.H;
    const int z_begin = static_cast<int>(bz) * kZ;
    const int z_end = min(g.D, z_begin + kZ);
    for (int z = z_begin; z < z_end; z += kAhead) {
      float s[kAhead];
      int m[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        s[k] = 0.f;
        m[k] = 1;
        if (col && z + k < z_end) {
          const size_t i = f3d_row(g, y, z + k) + static_cast<size_t>(x);
          s[k] = src[i];
          if (MASK) m[k] = mask[i];
        }
      }
#pragma unroll
      for (int k = 0; k < kAhead; ++k)
        if (z + k < z_end) voxel(s[k], m[k], col);  // the same for the whole workgroup
    }
  }
}

template <bool MASK>
__global__ __launch_bounds__(kBX* kBY) void k_histogram(const float* __restrict__ src, const int* __restrict__ mask, Rule rule, F3dGeo g,
                                                        Tiles t, u64* __restrict__ acc, u64* __restrict__ counters)
{
  __shared__ unsigned local[f3d_hist::kMaxBins];
  __shared__ unsigned tally[kCounters];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  for (int i = tid; i < rule.bins; i += kBX * kBY) local[i] = 0;
  if (tid < kCounters) tally[tid] = 0;
  __syncthreads();

  const int lane = threadIdx.x;
  int n_masked = 0, n_nan = 0, n_below = 0, n_above = 0, n_used = 0;
  walk_tiles<MASK>(src, mask, g, t, [&](float s, int m, bool inside) {
    int bin = -1;  // not counted
    if (inside) {
      const int c = (MASK && m == 0) ? f3d_hist::kMasked : f3d_hist::class_of(rule, s);
      n_masked += c == f3d_hist::kMasked;
      n_nan += c == f3d_hist::kNan;
      n_below += c == f3d_hist::kBelow;
      n_above += c == f3d_hist::kAbove;
      n_used += c == f3d_hist::kUsed;
      if (c == f3d_hist::kUsed) bin = f3d_hist::bin_of(rule, s);
    }
    // the runs of equal bins along the wave: a lane is the head of a run when its left neighbour holds another bin
    const int left = __shfl_up(bin, 1);
    const bool head = lane == 0 || left != bin;
    const u64 heads = __ballot(head);
    if (head && bin >= 0) {
      const u64 above = (heads >> lane) >> 1;  // the heads to the right of this lane
      const unsigned length = above ? static_cast<unsigned>(__ffsll(static_cast<long long>(above))) : static_cast<unsigned>(kBX - lane);
      __hip_atomic_fetch_add(&local[bin], length, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  });

  tally_add(tally + f3d_hist::kMasked, n_masked);
  tally_add(tally + f3d_hist::kNan, n_nan);
  tally_add(tally + f3d_hist::kBelow, n_below);
  tally_add(tally + f3d_hist::kAbove, n_above);
  tally_add(tally + f3d_hist::kUsed, n_used);

  __syncthreads();
  if (tid < f3d_hist::kClasses && tally[tid])
    __hip_atomic_fetch_add(counters + tid, static_cast<u64>(tally[tid]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int i = tid; i < rule.bins; i += kBX * kBY) {
    const unsigned c = local[i];
    if (c) __hip_atomic_fetch_add(acc + i, static_cast<u64>(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// counters[0..3]: masked, nan, infinite, finite; keys[0]: the largest ~key of a finite value (so ~keys[0] is the smallest key),
// keys[1]: the largest key.  Both start at 0, which no finite value gives (the keys 0 and ~0 are NaNs).
template <bool MASK>
__global__ __launch_bounds__(kBX* kBY) void k_value_range(const float* __restrict__ src, const int* __restrict__ mask, F3dGeo g, Tiles t,
                                                          u64* __restrict__ counters, unsigned* __restrict__ keys)
{
  __shared__ unsigned tally[kCounters];  // [0..3] the counters, [4] and [5] the two keys
  const int tid = threadIdx.y * kBX + threadIdx.x;
  if (tid < kCounters) tally[tid] = 0;
  __syncthreads();
  int n_masked = 0, n_nan = 0, n_infinite = 0, n_finite = 0;
  unsigned low = 0, high = 0;
  walk_tiles<MASK>(src, mask, g, t, [&](float s, int m, bool inside) {
    if (!inside) return;
    const unsigned bits = __float_as_uint(s);
    if (MASK && m == 0) {
      ++n_masked;
    } else if (s != s) {
      ++n_nan;
    } else if ((bits & 0x7f800000u) == 0x7f800000u) {
      ++n_infinite;
    } else {
      ++n_finite;
      const unsigned key = f3d_hist::key_of_bits(bits);
      low = max(low, ~key);
      high = max(high, key);
    }
  });
  tally_add(tally + 0, n_masked);
  tally_add(tally + 1, n_nan);
  tally_add(tally + 2, n_infinite);
  tally_add(tally + 3, n_finite);
  low = wave_max_u(low);
  high = wave_max_u(high);
  if (threadIdx.x == 0 && high) {  // a wave with a finite value
    __hip_atomic_fetch_max(tally + 4, low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_max(tally + 5, high, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  if (tid < 4 && tally[tid]) __hip_atomic_fetch_add(counters + tid, static_cast<u64>(tally[tid]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((tid == 4 || tid == 5) && tally[5])  // a workgroup with a finite value
    __hip_atomic_fetch_max(keys + (tid - 4), tally[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the checks both entries share, in the order of f3d_label_contacts; 0 with the geometry and the tiles
int box_of(const char* who, size_t width, size_t height, size_t depth, F3dGeo* g, Tiles* t)
{
  if (width == 0 || height == 0 || depth == 0) return f3d::fail("%s: empty volume %zux%zux%zu", who, width, height, depth);
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > kMaxVoxels)
    return f3d::fail("%s: volume %zux%zux%zu exceeds 32768 along an axis or 2^33 voxels", who, width, height, depth);
  if (!f3d::make_geo(g, width, height, depth, nullptr, who)) return 1;
  const size_t nx = (width + kBX - 1) / kBX, ny = (height + kBY - 1) / kBY, nz = (depth + kZ - 1) / kZ;
  t->nx = static_cast<unsigned>(nx);
  t->ny = static_cast<unsigned>(ny);
  t->count = static_cast<unsigned>(nx * ny * nz);  // at most 513 * 8193 * 1025 < 2^32 under the limits above
  return 0;
}

}  // namespace

extern "C" {

int f3d_value_range(f3d_devptr src, f3d_devptr mask, size_t width, size_t height, size_t depth, float* min_out, float* max_out,
                    f3d_range_info* info)
{
  F3D_REQUIRE_READY("f3d_value_range");
  if (!src) return f3d::fail("f3d_value_range: null src");
  if (!min_out || !max_out) return f3d::fail("f3d_value_range: null %s", min_out ? "max" : "min");
  if (!info) return f3d::fail("f3d_value_range: null info");
  F3dGeo g;
  Tiles t;
  if (box_of("f3d_value_range", width, height, depth, &g, &t)) return 1;

  void* d_buf;
  if (f3d::scratch_buffer(kCounters * sizeof(u64), &d_buf)) return 1;
  u64* counters = static_cast<u64*>(d_buf);
  unsigned* keys = reinterpret_cast<unsigned*>(counters + 4);
  hipStream_t stream = f3d::stream();
  F3D_HIP(hipMemsetAsync(counters, 0, kCounters * sizeof(u64), stream));
  const dim3 grid(std::min(t.count, kGroups)), block(kBX, kBY, 1);
  if (mask)
    hipLaunchKernelGGL(k_value_range<true>, grid, block, 0, stream, f3d_ptr<const float>(src), f3d_ptr<const int>(mask), g, t, counters, keys);
  else
    hipLaunchKernelGGL(k_value_range<false>, grid, block, 0, stream, f3d_ptr<const float>(src), f3d_ptr<const int>(mask), g, t, counters, keys);
  F3D_HIP(hipGetLastError());
  u64 c[kCounters];
  F3D_HIP(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  F3D_HIP(hipStreamSynchronize(stream));
  info->masked = c[0];
  info->nan = c[1];
  info->infinite = c[2];
  info->finite = c[3];
  const unsigned low = static_cast<unsigned>(c[4] & 0xffffffffull), high = static_cast<unsigned>(c[4] >> 32);
  *min_out = c[3] ? f3d_hist::float_of_key(~low) : INFINITY;
  *max_out = c[3] ? f3d_hist::float_of_key(high) : -INFINITY;
  return 0;
}

int f3d_histogram(f3d_devptr src, f3d_devptr mask, float lo, float hi, size_t bins, size_t width, size_t height, size_t depth,
                  unsigned long long* counts, f3d_histogram_info* info)
{
  F3D_REQUIRE_READY("f3d_histogram");
  if (!src) return f3d::fail("f3d_histogram: null src");
  if (!counts) return f3d::fail("f3d_histogram: null counts");
  if (!info) return f3d::fail("f3d_histogram: null info");
  Rule rule;
  if (const char* why = f3d_hist::make_rule(lo, hi, bins > 0x7fffffff ? 0x7fffffff : static_cast<long long>(bins), &rule))
    return f3d::fail("f3d_histogram: %s (lo %.9g, hi %.9g, bins %zu)", why, static_cast<double>(lo), static_cast<double>(hi), bins);
  F3dGeo g;
  Tiles t;
  if (box_of("f3d_histogram", width, height, depth, &g, &t)) return 1;

  // the accumulator, then the counters
  void* d_buf;
  const size_t words = static_cast<size_t>(rule.bins) + kCounters;
  if (f3d::scratch_buffer(words * sizeof(u64), &d_buf)) return 1;
  u64* acc = static_cast<u64*>(d_buf);
  u64* counters = acc + rule.bins;
  hipStream_t stream = f3d::stream();
  F3D_HIP(hipMemsetAsync(acc, 0, words * sizeof(u64), stream));
  const dim3 grid(std::min(t.count, kGroups)), block(kBX, kBY, 1);
  if (mask)
    hipLaunchKernelGGL(k_histogram<true>, grid, block, 0, stream, f3d_ptr<const float>(src), f3d_ptr<const int>(mask), rule, g, t, acc, counters);
  else
    hipLaunchKernelGGL(k_histogram<false>, grid, block, 0, stream, f3d_ptr<const float>(src), f3d_ptr<const int>(mask), rule, g, t, acc, counters);
  F3D_HIP(hipGetLastError());
  // Accumulator and counters come down in one copy into a buffer on this stack (32 KiB + 64 B), as f3d_label_components brings its
  // sizes down: nothing is copied straight into the caller's heap memory, and nothing of the caller's is written before the wait passed.
  u64 down[f3d_hist::kMaxBins + kCounters];
  F3D_HIP(hipMemcpyAsync(down, acc, words * sizeof(u64), hipMemcpyDeviceToHost, stream));
  F3D_HIP(hipStreamSynchronize(stream));
  std::copy(down, down + rule.bins, counts);
  const u64* c = down + rule.bins;
  info->masked = c[f3d_hist::kMasked];
  info->nan = c[f3d_hist::kNan];
  info->below = c[f3d_hist::kBelow];
  info->above = c[f3d_hist::kAbove];
  info->used = c[f3d_hist::kUsed];
  return 0;
}

}  // extern "C"
