// The three launches of the exact nearest-seed transform (f3d_nearest_seed of include/f3d.h), as templates over where the
// seeds come from and where the result goes, so that f3d_split_components runs the same passes on its own arrays.  Device code only;
// include after f3d_internal.h; everything is in an unnamed namespace inside f3d_near, a copy per translation unit.
//
// The nearest seed of a voxel minimises (squared distance, box index).  z, then y, then x order the box index, so the minimum separates:
//   near_x  per row: the nearest seed of the row, the left one on a tie          -> ax[i] = its x, -1 for a row without seed up to here
//   near_y  per column of a plane: min over y' of (x - ax(y'))^2 + (y - y')^2, the smaller y' on a tie -> axy[i] = sx | sy << 15, or -1
//   near_z  per column along z: min over z' of the plane's squared distance + (z - z')^2, the smaller z' on a tie -> out(...)
// ax, axy and the stacks are indexed by the box index x + W (y + H z); a line's stack entry k lies where the line's voxel k lies, so
// the lanes of a wave, which sit on consecutive x, store and load consecutive words at every step.  12 B per voxel of the box.
// Every line is one lane's (near_y, near_z) or one wave's (near_x) and reads only what an earlier launch wrote: no workgroup reads what
// another writes inside a launch.  No float instruction touches a distance.
#ifndef F3D_NEAREST_PASSES_H_
#define F3D_NEAREST_PASSES_H_

#define F3D_ENV_FN __device__ __forceinline__
#include "f3d_envelope.h"

namespace f3d_near {
namespace {

typedef unsigned long long u64;

constexpr int kLanes = 64;
constexpr int kLines = 4;              // waves of a workgroup: rows (near_x) or rows of lines (near_y, near_z)
constexpr int kRows = 32;              // planes a wave of near_x takes one after another
constexpr int kNoSeedD2 = 0x7fffffff;  // the squared distance of a box without seed
enum { kSeeds = 0, kD2Max, kCounters };

struct Box {
  int W, H, D;
};

__device__ __forceinline__ unsigned box_index(const Box& b, int x, int y, int z)
{
  return static_cast<unsigned>(x) + static_cast<unsigned>(b.W) * (static_cast<unsigned>(y) + static_cast<unsigned>(b.H) * static_cast<unsigned>(z));
}

// A wave takes one row at a time: it marches the row in steps of 64 columns, from the left with the last seed seen as the carry (ax =
// the nearest seed at or left of x), then from the right (the nearest one right of x) and keeps the nearer of the two, the left one on a
// tie.  It does so for the rows (y, z) of kRows consecutive planes and adds its count of seeds once at the end: one atomic per wave on
// the one counter (one per row took 3 ms at 512^3, eight times the rest of the kernel).  Lanes past the row stay in the wave for the
// ballots and touch no memory.  SEED: bool operator()(int x, int y, int z) const.
template <typename SEED>
__global__ __launch_bounds__(kLanes* kLines) void k_near_x(SEED seed, Box b, int* __restrict__ ax, u64* __restrict__ counters)
{
  const int lane = threadIdx.x;
  const int y = blockIdx.x * kLines + threadIdx.y;
  if (y >= b.H) return;  // the whole wave
  const int z_end = min(b.D, static_cast<int>(blockIdx.y + 1) * kRows);
  const int last = (b.W - 1) / kLanes * kLanes;
  unsigned count = 0;  // at most kRows * 32768 = 2^20
  for (int z = blockIdx.y * kRows; z < z_end; ++z) {
    int* __restrict__ row = ax + box_index(b, 0, y, z);
    int carry = -1;
    for (int x0 = 0; x0 <= last; x0 += kLanes) {
      const int x = x0 + lane;
      const bool s = x < b.W && seed(x, y, z);
      const u64 mask = __ballot(s);
      const u64 upto = mask & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);  // this lane and those left of it
      if (x < b.W) row[x] = upto ? x0 + 63 - __clzll(static_cast<long long>(upto)) : carry;
      if (mask) carry = x0 + 63 - __clzll(static_cast<long long>(mask));
      count += static_cast<unsigned>(__popcll(mask));
    }
    carry = -1;
    for (int x0 = last; x0 >= 0; x0 -= kLanes) {
      const int x = x0 + lane;
      const bool s = x < b.W && seed(x, y, z);
      const u64 mask = __ballot(s);
      const u64 beyond = lane == 63 ? 0ull : mask >> (lane + 1);  // bit 0 is the lane to the right
      const int right = beyond ? x + __ffsll(static_cast<long long>(beyond)) : carry;
      if (x < b.W) {
        const int left = row[x];  // this lane's own store of the first march
        if (right >= 0 && (left < 0 || right - x < x - left)) row[x] = right;
      }
      if (mask) carry = x0 + __ffsll(static_cast<long long>(mask)) - 1;
    }
  }
  if (lane == 0 && count) atomicAdd(counters + kSeeds, static_cast<u64>(count));
}

// the line of near_y: the column (x, z) of a plane, positions y
struct LineY {
  const int* __restrict__ ax;  // at the line's first voxel
  int* __restrict__ axy;
  unsigned* __restrict__ stack;
  unsigned step;  // W
  int x;
  __device__ __forceinline__ bool sample(int v, unsigned* f, unsigned* tag) const
  {
    const int sx = ax[static_cast<unsigned>(v) * step];
    if (sx < 0) return false;
    *f = static_cast<unsigned>((x - sx) * (x - sx));
    *tag = static_cast<unsigned>(sx);
    return true;
  }
  __device__ __forceinline__ void push(int k, unsigned e) const { stack[static_cast<unsigned>(k) * step] = e; }
  __device__ __forceinline__ unsigned entry(int k) const { return stack[static_cast<unsigned>(k) * step]; }
  __device__ __forceinline__ void emit(int i, int v, unsigned, unsigned tag) const
  {
    axy[static_cast<unsigned>(i) * step] = v < 0 ? -1 : static_cast<int>(tag | static_cast<unsigned>(v) << f3d_env::kCoordBits);
  }
};

__global__ __launch_bounds__(kLanes* kLines) void k_near_y(Box b, const int* __restrict__ ax, int* __restrict__ axy, unsigned* __restrict__ stack)
{
  const int x = blockIdx.x * kLanes + threadIdx.x;
  const int z = blockIdx.y * kLines + threadIdx.y;
  if (x >= b.W || z >= b.D) return;
  const unsigned first = box_index(b, x, 0, z);
  LineY io = {ax + first, axy + first, stack + first, static_cast<unsigned>(b.W), x};
  f3d_env::line(io, b.H);
}

// the line of near_z: the column (x, y) along z.  OUT: void operator()(int x, int y, int z, int d2, int sx, int sy, int sz) const, with
// d2 = kNoSeedD2 and sx = sy = sz = -1 for a box without seed.
template <typename OUT>
struct LineZ {
  const int* __restrict__ axy;
  unsigned* __restrict__ stack;
  unsigned step;  // W * H
  int x, y;
  unsigned d2_max;
  OUT out;
  __device__ __forceinline__ bool sample(int v, unsigned* f, unsigned* tag) const
  {
    const int p = axy[static_cast<unsigned>(v) * step];
    if (p < 0) return false;
    const int sx = p & static_cast<int>(f3d_env::kCoordMask), sy = p >> f3d_env::kCoordBits;
    *f = static_cast<unsigned>((x - sx) * (x - sx)) + static_cast<unsigned>((y - sy) * (y - sy));
    *tag = static_cast<unsigned>(p);
    return true;
  }
  __device__ __forceinline__ void push(int k, unsigned e) const { stack[static_cast<unsigned>(k) * step] = e; }
  __device__ __forceinline__ unsigned entry(int k) const { return stack[static_cast<unsigned>(k) * step]; }
  __device__ __forceinline__ void emit(int i, int v, unsigned f, unsigned tag)
  {
    if (v < 0) {
      d2_max = static_cast<unsigned>(kNoSeedD2);
      out(x, y, i, kNoSeedD2, -1, -1, -1);
      return;
    }
    const unsigned d2 = f + static_cast<unsigned>((i - v) * (i - v));
    d2_max = d2 > d2_max ? d2 : d2_max;
    out(x, y, i, static_cast<int>(d2), static_cast<int>(tag & f3d_env::kCoordMask), static_cast<int>(tag >> f3d_env::kCoordBits), v);
  }
};

template <typename OUT>
__global__ __launch_bounds__(kLanes* kLines) void k_near_z(Box b, const int* __restrict__ axy, unsigned* __restrict__ stack, OUT out,
                                                            u64* __restrict__ counters)
{
  const int x = blockIdx.x * kLanes + threadIdx.x;
  const int y = blockIdx.y * kLines + threadIdx.y;
  if (y >= b.H) return;  // the whole wave; lanes past the row stay for the cross-lane maximum
  unsigned d2_max = 0;
  if (x < b.W) {
    const unsigned first = box_index(b, x, y, 0);
    LineZ<OUT> io = {axy + first, stack + first, static_cast<unsigned>(b.W) * static_cast<unsigned>(b.H), x, y, 0u, out};
    f3d_env::line(io, b.D);
    d2_max = io.d2_max;
  }
  for (int o = 32; o > 0; o >>= 1) d2_max = max(d2_max, static_cast<unsigned>(__shfl_xor(d2_max, o)));
  if (threadIdx.x == 0 && d2_max) atomicMax(counters + kD2Max, static_cast<u64>(d2_max));
}

// bytes of scratch for a box of n voxels behind the counters: ax, axy and the stacks
inline size_t scratch_words(size_t n) { return 3 * n; }

// the three launches on `stream`; counters (kCounters words) are cleared by the caller.  ax, axy, stack: n words each.
template <typename SEED, typename OUT>
int launch(hipStream_t stream, const Box& b, SEED seed, OUT out, int* ax, int* axy, unsigned* stack, u64* counters)
{
  const dim3 block(kLanes, kLines, 1);
  hipLaunchKernelGGL(k_near_x<SEED>, dim3((b.H + kLines - 1) / kLines, (b.D + kRows - 1) / kRows), block, 0, stream, seed, b, ax, counters);
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_near_y, dim3((b.W + kLanes - 1) / kLanes, (b.D + kLines - 1) / kLines), block, 0, stream, b, ax, axy, stack);
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_near_z<OUT>, dim3((b.W + kLanes - 1) / kLanes, (b.H + kLines - 1) / kLines), block, 0, stream, b, axy, stack, out,
                     counters);
  F3D_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace f3d_near
#endif  // F3D_NEAREST_PASSES_H_
