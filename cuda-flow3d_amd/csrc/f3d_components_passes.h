// The passes of f3d_label_components (include/f3d.h) as they stood in f3d_label_components.hip, moved here so that
// f3d_split_components runs the same text on a mask of its own: k_tile is a template over what makes a voxel foreground,
// everything else is unchanged.  Device code of one translation unit: include after f3d_internal.h; everything is in an unnamed
// namespace inside f3d_cc.
//
// union_passes   k_tile, k_merge<0>, k_flatten<false>, k_merge<1>, k_flatten<true>: parent = the root (the smallest box index) of every
//                foreground voxel, kBackground elsewhere; aux[root] = the size of its body; counters[kForeground], counters[kNan]
// number_passes  k_flag_sums, k_scan_sums, k_number, k_write on any (parent, aux) of that form: the bodies of at least min_voxels
//                voxels numbered in ascending order of root, labels written, the remaining counters
#ifndef F3D_COMPONENTS_PASSES_H_
#define F3D_COMPONENTS_PASSES_H_

#include <algorithm>

#include "f3d_partials.h"

#define F3D_UF_FN __device__ __forceinline__
#include "f3d_union_find.h"

namespace f3d_cc {
namespace {

static_assert(kScanBlock % 64 == 0 && kScanThreads % 64 == 0 && kScanThreads <= 1024 && kScanItems >= 1, "whole waves, one workgroup");

using f3d_partials::wave_sum;
using f3d_uf::kBackground;

typedef unsigned long long u64;

constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;
// kScanBlock, kScanItems and kScanThreads, the shape of the prefix sum, are defined by the translation unit before it includes this
// file: tests read them from f3d_label_components.hip, where they have always stood, and f3d_split_components.hip repeats them
constexpr int kScanSpan = kScanBlock * kScanItems;  // voxels per workgroup: one block sum
constexpr int kCounters = 8;
enum { kForeground = 0, kNan, kComponents, kLabels, kDroppedComponents, kDroppedVoxels, kLargest };

// the parent array as f3d_union_find.h wants it.  The load is a relaxed atomic one so that it is a load every time round a loop; it
// promises nothing about what other compute dies have written since (loads are hints).  fetch_min is the device-scope atomic whose
// return value decides.
struct Parents {
  unsigned* p;
  __device__ __forceinline__ unsigned load(unsigned i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ unsigned fetch_min(unsigned i, unsigned v) const
  {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void store(unsigned i, unsigned v) const { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// the same over the parents of one tile in LDS, which every lane of the workgroup sees as it is
struct TileParents {
  unsigned* p;
  __device__ __forceinline__ unsigned load(unsigned i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ unsigned fetch_min(unsigned i, unsigned v) const
  {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void store(unsigned i, unsigned v) const { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

struct Box {
  int W, H, D;
  unsigned plane;  // W * H
};

__device__ __forceinline__ unsigned box_index(const Box& b, int x, int y, int z)
{
  return static_cast<unsigned>(x) + static_cast<unsigned>(b.W) * (static_cast<unsigned>(y) + static_cast<unsigned>(b.H) * static_cast<unsigned>(z));
}

// A wave is one row of 64 x (threadIdx.y and with it y and z are the same for all its lanes), a workgroup kBY rows, a lane marches over
// kZ planes.  Lanes past the box stay in the wave (the ballots and the cross-lane moves want all of them) and touch no memory.
//
// k_tile: classify (CLASSIFY: bool operator()(int x, int y, int z, unsigned* n_nan) const, which also counts what it calls a NaN),
// count, and label one tile of kBX x kBY x kZ voxels with the union-find over the tile's
// own parents in LDS (32 KiB).  A parent starts as the start of the voxel's run along x inside its wave (a ballot), then the faces
// towards +y and +z inside the tile are joined.  The tile is indexed x + kBX (y + kBY z) inside the tile -- the same order as the box
// index, so the root of a body's part inside the tile is its smallest box index there.  What is stored is the box index of that root:
// k_merge then only has the faces on the seams between tiles left.
template <typename CLASSIFY>
__global__ __launch_bounds__(kBX* kBY) void k_tile(CLASSIFY classify, Box b, unsigned* __restrict__ parent, unsigned* __restrict__ aux,
                                                    u64* __restrict__ counters)
{
  __shared__ unsigned tile[kBX * kBY * kZ];
  const int lane = threadIdx.x, ty = threadIdx.y;
  const int x = blockIdx.x * kBX + lane;
  const int y = blockIdx.y * kBY + ty;
  const int z0 = blockIdx.z * kZ;
  const int nz = min(kZ, b.D - z0);
  const bool col = y < b.H && x < b.W;
  TileParents uf = {tile};
  unsigned n_fg = 0, n_nan = 0;
  for (int lz = 0; lz < nz; ++lz) {
    bool fg = false;
    if (col) fg = classify(x, y, z0 + lz, &n_nan);
    n_fg += fg ? 1u : 0u;
    const u64 mask = __ballot(fg);  // the rows past the box are whole waves, and they are here
    const u64 below = ~mask & ((1ull << lane) - 1ull);
    const int start = below ? 64 - __clzll(static_cast<long long>(below)) : 0;
    const unsigned local = static_cast<unsigned>(lane + kBX * (ty + kBY * lz));
    tile[local] = fg ? local - static_cast<unsigned>(lane - start) : kBackground;
  }
  __syncthreads();
  for (int lz = 0; lz < nz; ++lz) {
    const unsigned local = static_cast<unsigned>(lane + kBX * (ty + kBY * lz));
    const unsigned own = tile[local];  // written before the barrier
    const bool fg = own != kBackground;
    const unsigned far_y = fg && ty + 1 < kBY ? tile[local + kBX] : kBackground;  // a row past the box is background
    const unsigned far_z = fg && lz + 1 < nz ? tile[local + kBX * kBY] : kBackground;
    const bool both_y = far_y != kBackground, both_z = far_z != kBackground;
    const int left_y = __shfl_up(both_y ? 1 : 0, 1), left_z = __shfl_up(both_z ? 1 : 0, 1);
    if (both_y && (lane == 0 || !left_y)) f3d_uf::unite(uf, own, far_y);
    if (both_z && (lane == 0 || !left_z)) f3d_uf::unite(uf, own, far_z);
  }
  __syncthreads();
  if (col) {
    for (int lz = 0; lz < nz; ++lz) {
      const unsigned local = static_cast<unsigned>(lane + kBX * (ty + kBY * lz));
      const unsigned i = box_index(b, x, y, z0 + lz);
      unsigned root = kBackground;
      if (tile[local] != kBackground) {
        const unsigned r = f3d_uf::find(uf, local);  // nothing writes the tile any more
        root = box_index(b, blockIdx.x * kBX + static_cast<int>(r % kBX), blockIdx.y * kBY + static_cast<int>(r / kBX % kBY),
                         z0 + static_cast<int>(r / (kBX * kBY)));
      }
      parent[i] = root;
      aux[i] = 0;
    }
  }
  const u64 fg_sum = wave_sum(static_cast<u64>(n_fg)), nan_sum = wave_sum(static_cast<u64>(n_nan));
  if (lane == 0) {
    if (fg_sum) atomicAdd(counters + kForeground, fg_sum);
    if (nan_sum) atomicAdd(counters + kNan, nan_sum);
  }
}

// The faces on the seams between tiles.  AXIS 0: those towards +y of a tile's last row, and those towards +x between the last lane of a
// wave and the first of the next.  AXIS 1: those towards +z of a tile's last plane.  A face between two foreground voxels whose -x neighbours, in the same wave, are both
// foreground too is left out: the two runs are the same two runs, and the face at the start of their overlap joins them.
template <int AXIS>
__global__ __launch_bounds__(kBX* kBY) void k_merge(Box b, unsigned* __restrict__ parent)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  if (y >= b.H) return;
  const bool col = x < b.W;
  const int lane = threadIdx.x;
  const unsigned step = AXIS == 0 ? static_cast<unsigned>(b.W) : b.plane;
  const int z_end = min(b.D, static_cast<int>(blockIdx.z + 1) * kZ);
  Parents uf = {parent};
  const bool seam = AXIS == 1 || threadIdx.y == kBY - 1;
  for (int z = AXIS == 1 ? z_end - 1 : blockIdx.z * kZ; z < z_end; ++z) {
    const unsigned i = box_index(b, x, y, z);
    const bool has = col && seam && (AXIS == 0 ? y + 1 < b.H : z + 1 < b.D);
    // written by the launch before this one: plain loads see them.  They are the first hints of the walk.
    const unsigned own = col ? parent[i] : kBackground;
    const unsigned far = has && own != kBackground ? parent[i + step] : kBackground;
    const bool both = far != kBackground;
    const int left = __shfl_up(both ? 1 : 0, 1);  // every lane of the wave is here
    if (both && (lane == 0 || !left)) f3d_uf::unite(uf, own, far);
    if (AXIS == 0 && lane == kBX - 1 && own != kBackground && x + 1 < b.W) {
      const unsigned next = parent[i + 1];
      if (next != kBackground) f3d_uf::unite(uf, own, next);
    }
  }
}

// parent = root.  SIZES: the first lane of every run inside the wave adds the length of the run to aux[root] (one root per run).
template <bool SIZES>
__global__ __launch_bounds__(kBX* kBY) void k_flatten(Box b, unsigned* __restrict__ parent, unsigned* __restrict__ aux)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  if (y >= b.H) return;
  const bool col = x < b.W;
  const int lane = threadIdx.x;
  const int z_end = min(b.D, static_cast<int>(blockIdx.z + 1) * kZ);
  Parents uf = {parent};
  // what the lane has seen of one root and not yet added: a body that fills the column of runs this lane heads costs one add, not kZ
  unsigned held_root = kBackground, held = 0;
  for (int z = blockIdx.z * kZ; z < z_end; ++z) {
    const unsigned i = box_index(b, x, y, z);
    const bool fg = col && parent[i] != kBackground;
    unsigned root = 0;
    if (fg) root = f3d_uf::flatten(uf, i);
    if (SIZES) {
      const u64 mask = __ballot(fg);
      if (fg && (lane == 0 || !((mask >> (lane - 1)) & 1ull))) {
        const u64 above = ~mask >> lane;  // bit 0 is this lane: clear
        const int length = above ? __ffsll(static_cast<long long>(above)) - 1 : 64 - lane;
        if (root != held_root) {
          if (held) atomicAdd(aux + held_root, held);
          held_root = root;
          held = 0;
        }
        held += static_cast<unsigned>(length);
      }
    }
  }
  if (SIZES && held) atomicAdd(aux + held_root, held);
}

// whether voxel i is the root of a kept body; *size its size when it is a root at all (0 otherwise)
__device__ __forceinline__ bool kept_root(const unsigned* __restrict__ parent, const unsigned* __restrict__ aux, unsigned i, u64 min_voxels,
                                          unsigned* size)
{
  *size = 0;
  if (parent[i] != i) return false;
  *size = aux[i];
  return static_cast<u64>(*size) >= min_voxels;
}

// The counts of kept roots of kScanSpan consecutive voxels, thread t on voxels [t * kScanItems, (t + 1) * kScanItems) of the span, and
// the exclusive prefix of the thread's count inside the workgroup (wave by cross-lane moves, the four waves through LDS).
__device__ __forceinline__ unsigned block_exclusive(unsigned mine, unsigned* total)
{
  __shared__ unsigned wave_total[kScanBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kScanBlock / 64; ++k) {
    before += k < wave ? wave_total[k] : 0u;
    all += wave_total[k];
  }
  *total = all;
  return before + incl - mine;
}

// what k_flag_sums leaves per span of kScanSpan voxels: the kept roots (which k_scan_sums turns into their exclusive prefix), all roots,
// the largest size and the voxels of the dropped roots.  No atomics: k_scan_sums adds them up in its own fixed order.
struct SpanStats {
  unsigned* kept;
  unsigned* roots;
  unsigned* largest;
  u64* dropped_voxels;
};

__global__ __launch_bounds__(kScanBlock) void k_flag_sums(const unsigned* __restrict__ parent, const unsigned* __restrict__ aux, unsigned n,
                                                          u64 min_voxels, SpanStats stats)
{
  __shared__ u64 wave_voxels_part[kScanBlock / 64];
  __shared__ unsigned wave_roots_part[kScanBlock / 64], wave_largest_part[kScanBlock / 64];
  const unsigned first = blockIdx.x * static_cast<unsigned>(kScanSpan) + threadIdx.x * kScanItems;
  unsigned kept = 0, roots = 0, largest = 0;
  u64 dropped_voxels = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const unsigned i = first + k;
    if (i >= n) break;
    unsigned size;
    const bool keep = kept_root(parent, aux, i, min_voxels, &size);
    kept += keep ? 1u : 0u;
    roots += size ? 1u : 0u;
    dropped_voxels += keep ? 0u : size;
    largest = max(largest, size);
  }
  unsigned total;
  block_exclusive(kept, &total);
  const u64 wave_roots = wave_sum(static_cast<u64>(roots)), wave_voxels = wave_sum(dropped_voxels);
  unsigned wave_largest = largest;
  for (int o = 32; o > 0; o >>= 1) wave_largest = max(wave_largest, static_cast<unsigned>(__shfl_xor(wave_largest, o)));
  if ((threadIdx.x & 63) == 0) {
    wave_roots_part[threadIdx.x >> 6] = static_cast<unsigned>(wave_roots);
    wave_voxels_part[threadIdx.x >> 6] = wave_voxels;
    wave_largest_part[threadIdx.x >> 6] = wave_largest;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all_roots = 0, all_largest = 0;
    u64 all_voxels = 0;
    for (int k = 0; k < kScanBlock / 64; ++k) {
      all_roots += wave_roots_part[k];
      all_voxels += wave_voxels_part[k];
      all_largest = max(all_largest, wave_largest_part[k]);
    }
    stats.kept[blockIdx.x] = total;
    stats.roots[blockIdx.x] = all_roots;
    stats.largest[blockIdx.x] = all_largest;
    stats.dropped_voxels[blockIdx.x] = all_voxels;
  }
}

// one workgroup: kept[0 .. count) becomes its own exclusive prefix, kScanThreads entries per trip with the carry of the trips before;
// the other three statistics are added up on the way (integers: the order does not show) and the counters of the info written
__global__ __launch_bounds__(kScanThreads) void k_scan_sums(SpanStats stats, unsigned count, u64* __restrict__ counters)
{
  __shared__ unsigned wave_total[kScanThreads / 64];
  __shared__ u64 roots_part[kScanThreads / 64], voxels_part[kScanThreads / 64];
  __shared__ unsigned largest_part[kScanThreads / 64];
  unsigned* __restrict__ sums = stats.kept;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0, my_largest = 0;
  u64 my_roots = 0, my_voxels = 0;
  for (unsigned base = 0; base < count; base += kScanThreads) {
    const unsigned at = base + threadIdx.x;
    const unsigned mine = at < count ? sums[at] : 0u;
    if (at < count) {
      my_roots += stats.roots[at];
      my_voxels += stats.dropped_voxels[at];
      my_largest = max(my_largest, stats.largest[at]);
    }
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; ++k) {
      before += k < wave ? wave_total[k] : 0u;
      all += wave_total[k];
    }
    if (at < count) sums[at] = carry + before + incl - mine;
    carry += all;
    __syncthreads();  // wave_total is written again in the next trip
  }
  const u64 wave_roots = wave_sum(my_roots), wave_voxels = wave_sum(my_voxels);
  for (int o = 32; o > 0; o >>= 1) my_largest = max(my_largest, static_cast<unsigned>(__shfl_xor(my_largest, o)));
  if (lane == 0) {
    roots_part[wave] = wave_roots;
    voxels_part[wave] = wave_voxels;
    largest_part[wave] = my_largest;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 roots = 0, voxels = 0;
    unsigned largest = 0;
    for (int k = 0; k < kScanThreads / 64; ++k) {
      roots += roots_part[k];
      voxels += voxels_part[k];
      largest = max(largest, largest_part[k]);
    }
    counters[kLabels] = carry;
    counters[kComponents] = roots;
    counters[kDroppedComponents] = roots - carry;
    counters[kDroppedVoxels] = voxels;
    counters[kLargest] = largest;
  }
}

__global__ __launch_bounds__(kScanBlock) void k_number(const unsigned* __restrict__ parent, unsigned* __restrict__ aux, unsigned n,
                                                       u64 min_voxels, const unsigned* __restrict__ sums, unsigned* __restrict__ sizes,
                                                       unsigned sizes_room)
{
  const unsigned first = blockIdx.x * static_cast<unsigned>(kScanSpan) + threadIdx.x * kScanItems;
  unsigned size[kScanItems];
  bool keep[kScanItems];
  unsigned kept = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const unsigned i = first + k;
    size[k] = 0;
    keep[k] = i < n && kept_root(parent, aux, i, min_voxels, &size[k]);
    kept += keep[k] ? 1u : 0u;
  }
  unsigned total;
  unsigned number = sums[blockIdx.x] + block_exclusive(kept, &total);  // the kept roots before this thread's first voxel
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (!size[k]) continue;  // not a root
    const unsigned i = first + k;
    if (keep[k]) {
      if (number < sizes_room) sizes[number] = size[k];
      aux[i] = ++number;
    } else {
      aux[i] = 0;
    }
  }
}

__global__ __launch_bounds__(kBX* kBY) void k_write(F3dGeo g, Box b, const unsigned* __restrict__ parent, const unsigned* __restrict__ aux,
                                                     int* __restrict__ labels)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  if (y >= b.H || x >= b.W) return;
  const int z_end = min(b.D, static_cast<int>(blockIdx.z + 1) * kZ);
  for (int z = blockIdx.z * kZ; z < z_end; ++z) {
    const unsigned root = parent[box_index(b, x, y, z)];
    labels[f3d_row(g, y, z) + x] = root == kBackground ? 0 : static_cast<int>(aux[root]);
  }
}

// the float threshold of f3d_label_components: lo <= s && s <= hi, false for a NaN, which is counted
struct Threshold {
  const float* __restrict__ src;
  float lo, hi;
  F3dGeo g;
  __device__ __forceinline__ bool operator()(int x, int y, int z, unsigned* n_nan) const
  {
    const float s = src[f3d_row(g, y, z) + x];
    *n_nan += s != s ? 1u : 0u;
    return lo <= s && s <= hi;
  }
};

inline dim3 tile_grid(const Box& b) { return dim3((b.W + kBX - 1) / kBX, (b.H + kBY - 1) / kBY, (b.D + kZ - 1) / kZ); }

template <typename CLASSIFY>
int union_passes(hipStream_t stream, CLASSIFY classify, const Box& b, unsigned* parent, unsigned* aux, u64* counters)
{
  const dim3 tiles = tile_grid(b), tile(kBX, kBY, 1);
  hipLaunchKernelGGL(k_tile<CLASSIFY>, tiles, tile, 0, stream, classify, b, parent, aux, counters);
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_merge<0>, tiles, tile, 0, stream, b, parent);
  F3D_HIP(hipGetLastError());
  if (b.D > 1) {
    hipLaunchKernelGGL(k_flatten<false>, tiles, tile, 0, stream, b, parent, aux);
    F3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_merge<1>, tiles, tile, 0, stream, b, parent);
    F3D_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_flatten<true>, tiles, tile, 0, stream, b, parent, aux);
  F3D_HIP(hipGetLastError());
  return 0;
}

// the four statistics per span of kScanSpan voxels in one block of memory: bytes, and the pointers into it
inline size_t span_count(size_t n) { return (n + kScanSpan - 1) / kScanSpan; }
inline size_t span_stats_bytes(size_t n)
{
  const size_t words = (span_count(n) * sizeof(unsigned) + 255) / 256 * 256;
  return 3 * words + (span_count(n) * sizeof(u64) + 255) / 256 * 256;
}
inline SpanStats span_stats_at(char* at, size_t n)
{
  const size_t words = (span_count(n) * sizeof(unsigned) + 255) / 256 * 256;
  SpanStats stats;
  stats.kept = reinterpret_cast<unsigned*>(at);
  stats.roots = reinterpret_cast<unsigned*>(at + words);
  stats.largest = reinterpret_cast<unsigned*>(at + 2 * words);
  stats.dropped_voxels = reinterpret_cast<u64*>(at + 3 * words);
  return stats;
}

inline int number_passes(hipStream_t stream, const F3dGeo& g, const Box& b, size_t n, u64 min_voxels, const unsigned* parent, unsigned* aux,
                         SpanStats stats, unsigned* d_sizes, size_t sizes_room, int* labels, u64* counters)
{
  const unsigned n_sums = static_cast<unsigned>(span_count(n)), count = static_cast<unsigned>(n);
  hipLaunchKernelGGL(k_flag_sums, dim3(n_sums), dim3(kScanBlock), 0, stream, parent, aux, count, min_voxels, stats);
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kScanThreads), 0, stream, stats, n_sums, counters);
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_number, dim3(n_sums), dim3(kScanBlock), 0, stream, parent, aux, count, min_voxels, stats.kept, d_sizes,
                     static_cast<unsigned>(sizes_room));
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_write, tile_grid(b), dim3(kBX, kBY, 1), 0, stream, g, b, parent, aux, labels);
  F3D_HIP(hipGetLastError());
  return 0;
}

// a size is below 2^31: it comes down as one word and is widened here, through a buffer of 64 KiB whatever the number of labels
inline int download_sizes(hipStream_t stream, const unsigned* d_sizes, size_t handed, unsigned long long* sizes)
{
  unsigned narrow[16384];
  for (size_t done = 0; done < handed; done += 16384) {
    const size_t part = std::min<size_t>(16384, handed - done);
    F3D_HIP(hipMemcpyAsync(narrow, d_sizes + done, part * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    F3D_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < part; ++i) sizes[done + i] = narrow[i];
  }
  return 0;
}

}  // namespace
}  // namespace f3d_cc
#endif  // F3D_COMPONENTS_PASSES_H_
