// Bodies of a thresholded volume with touching bodies taken apart, for gfx950 (f3d_split_components): the foreground is eroded to its
// cores (squared distance to the background of at least core_d2), the cores are labelled, and every foreground voxel goes to the core
// nearest to it (exact Euclidean, ties by box index) when that core lies in its own component, else to the remainder of its component.
// The definition is include/f3d.h's; tests/nearest_ref.py restates it in numpy and every label, size and counter matches bit for bit.
//
// A fixed list of launches on the library stream, each reading only what an earlier launch wrote or what an atomic returned to it:
//   union passes (f3d_components_passes.h) on the threshold          -> comp = the root of every foreground voxel's component
//   nearest passes (f3d_nearest_passes.h), seeds = the background    -> d2
//   union passes on the core mask, comp is set and d2 >= core_d2     -> core = the root of every core voxel's core body
//   nearest passes, seeds = the core voxels                          -> cls = the class of every foreground voxel: the root of a core
//                                                                       body, or the root of its component with kRemainder set
//   k_class_min     the smallest box index of every class, integer atomicMin into a table at the class's root (one table for the core
//                   bodies, one for the remainders: a component's root may be a core body's root too)
//   k_class_root    cls = that smallest index, which makes (cls, aux) the (parent, aux) of a labelling; sizes by integer atomicAdd
//   number passes   flag, scan, number, write, as for f3d_label_components
// A wave is a row of 64 x; a run of equal classes inside it costs one atomic, and a lane that meets the same class plane after plane
// holds its count back.  No spin loop, no flag, no lane waits for another.  Scratch: eight words per voxel of the box (comp, core, d2,
// the three of the nearest passes, the class, and the table that does not fit into one of those that are free by then) = 32 B, the
// statistics of the prefix sum and the sizes handed out, in the calling thread's grow-only buffer.
#include <algorithm>
#include <cmath>

#include "f3d_internal.h"

namespace f3d_cc {
namespace {
constexpr int kScanBlock = 256;    // as in f3d_label_components.hip
constexpr int kScanItems = 4;
constexpr int kScanThreads = 1024;
}  // namespace
}  // namespace f3d_cc
#include "f3d_components_passes.h"
#include "f3d_nearest_passes.h"

namespace {

using namespace f3d_cc;

constexpr unsigned kRemainder = 0x80000000u;  // a box index is below 2^31 - 1: the bit is free, and the result is never kBackground
enum { kConnected = 0, kCores, kRemainderBodies, kRemainderVoxels, kSplitCounters };

struct BackgroundSeeds {
  const unsigned* __restrict__ comp;
  f3d_near::Box b;
  __device__ __forceinline__ bool operator()(int x, int y, int z) const { return comp[f3d_near::box_index(b, x, y, z)] == kBackground; }
};

struct StoreD2 {
  int* __restrict__ d2;
  f3d_near::Box b;
  __device__ __forceinline__ void operator()(int x, int y, int z, int dist, int, int, int) const { d2[f3d_near::box_index(b, x, y, z)] = dist; }
};

struct CoreMask {
  const unsigned* __restrict__ comp;
  const int* __restrict__ d2;
  u64 core_d2;
  f3d_near::Box b;
  __device__ __forceinline__ bool operator()(int x, int y, int z, unsigned*) const
  {
    const unsigned i = f3d_near::box_index(b, x, y, z);
    return comp[i] != kBackground && static_cast<u64>(d2[i]) >= core_d2;
  }
};

struct CoreSeeds {
  const unsigned* __restrict__ core;
  f3d_near::Box b;
  __device__ __forceinline__ bool operator()(int x, int y, int z) const { return core[f3d_near::box_index(b, x, y, z)] != kBackground; }
};

struct StoreClass {
  const unsigned* __restrict__ comp;
  const unsigned* __restrict__ core;
  unsigned* __restrict__ cls;
  f3d_near::Box b;
  __device__ __forceinline__ void operator()(int x, int y, int z, int, int sx, int sy, int sz) const
  {
    const unsigned i = f3d_near::box_index(b, x, y, z);
    const unsigned mine = comp[i];
    unsigned c = kBackground;
    if (mine != kBackground) {
      c = mine | kRemainder;
      if (sx >= 0) {
        const unsigned s = f3d_near::box_index(b, sx, sy, sz);
        if (comp[s] == mine) c = core[s];  // the nearest core voxel lies in this voxel's component
      }
    }
    cls[i] = c;
  }
};

__device__ __forceinline__ unsigned* class_slot(unsigned c, unsigned* core_table, unsigned* remainder_table)
{
  return c & kRemainder ? remainder_table + (c & ~kRemainder) : core_table + c;
}

// The smallest box index of every class.  Inside a wave the first lane of a run of one class holds the run's smallest index, and a lane
// that marches up z meets a class first at its smallest index there: it asks again only when the class changes.
__global__ __launch_bounds__(kBX* kBY) void k_class_min(Box b, const unsigned* __restrict__ cls, unsigned* __restrict__ core_min,
                                                         unsigned* __restrict__ remainder_min)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  if (y >= b.H) return;
  const bool col = x < b.W;
  const int lane = threadIdx.x;
  const int z_end = min(b.D, static_cast<int>(blockIdx.z + 1) * kZ);
  unsigned held = kBackground;
  for (int z = blockIdx.z * kZ; z < z_end; ++z) {
    const unsigned i = box_index(b, x, y, z);
    const unsigned c = col ? cls[i] : kBackground;
    const unsigned left = __shfl_up(c, 1);  // every lane of the wave is here
    if (c != kBackground && (lane == 0 || left != c) && c != held) {
      held = c;
      atomicMin(class_slot(c, core_min, remainder_min), i);
    }
  }
}

// cls = the smallest index of the voxel's class; aux[that index] += the voxels of the class, a run of one class inside the wave at a
// time; and the four counters of the split that are sums over voxels.
__global__ __launch_bounds__(kBX* kBY) void k_class_root(Box b, unsigned* __restrict__ cls, const unsigned* __restrict__ core_min,
                                                          const unsigned* __restrict__ remainder_min, unsigned* __restrict__ aux,
                                                          const unsigned* __restrict__ comp, const unsigned* __restrict__ core,
                                                          u64* __restrict__ counters)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  if (y >= b.H) return;
  const bool col = x < b.W;
  const int lane = threadIdx.x;
  const int z_end = min(b.D, static_cast<int>(blockIdx.z + 1) * kZ);
  unsigned held_root = kBackground, held = 0;
  unsigned n_connected = 0, n_cores = 0, n_remainder_bodies = 0, n_remainder = 0;
  for (int z = blockIdx.z * kZ; z < z_end; ++z) {
    const unsigned i = box_index(b, x, y, z);
    const unsigned c = col ? cls[i] : kBackground;
    unsigned root = kBackground;
    if (c != kBackground) {
      root = c & kRemainder ? remainder_min[c & ~kRemainder] : core_min[c];
      cls[i] = root;
      n_connected += comp[i] == i ? 1u : 0u;
      n_cores += core[i] == i ? 1u : 0u;
      n_remainder += c & kRemainder ? 1u : 0u;
      n_remainder_bodies += (c & kRemainder) && root == i ? 1u : 0u;
    }
    const unsigned left = __shfl_up(root, 1);
    const bool first = lane == 0 || left != root;
    const u64 firsts = __ballot(first);
    if (first && root != kBackground) {
      const u64 above = lane == 63 ? 0ull : firsts >> (lane + 1);  // bit 0 is the lane to the right
      const int length = above ? __ffsll(static_cast<long long>(above)) : 64 - lane;
      if (root != held_root) {
        if (held) atomicAdd(aux + held_root, held);
        held_root = root;
        held = 0;
      }
      held += static_cast<unsigned>(length);
    }
  }
  if (held) atomicAdd(aux + held_root, held);
  const u64 sums[kSplitCounters] = {wave_sum(static_cast<u64>(n_connected)), wave_sum(static_cast<u64>(n_cores)),
                                    wave_sum(static_cast<u64>(n_remainder_bodies)), wave_sum(static_cast<u64>(n_remainder))};
  if (lane == 0)
    for (int k = 0; k < kSplitCounters; ++k)
      if (sums[k]) atomicAdd(counters + k, sums[k]);
}

size_t round_up(size_t n, size_t to) { return (n + to - 1) / to * to; }

}  // namespace

extern "C" {

int f3d_split_components(f3d_devptr src, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels, f3d_devptr labels_out,
                         size_t width, size_t height, size_t depth, unsigned long long* sizes, size_t capacity, f3d_split_info* info)
{
  F3D_REQUIRE_READY("f3d_split_components");
  if (!src) return f3d::fail("f3d_split_components: null src");
  if (!labels_out) return f3d::fail("f3d_split_components: null labels_out");
  if (!info) return f3d::fail("f3d_split_components: null info");
  if (src == labels_out) return f3d::fail("f3d_split_components: labels_out is the container of src");
  if (std::isnan(lo) || std::isnan(hi)) return f3d::fail("f3d_split_components: %s is NaN", std::isnan(lo) ? "lo" : "hi");
  if (lo > hi) return f3d::fail("f3d_split_components: lo %g is above hi %g", static_cast<double>(lo), static_cast<double>(hi));
  if (core_d2 == 0) return f3d::fail("f3d_split_components: core_d2 must be at least 1");
  if (min_voxels == 0) return f3d::fail("f3d_split_components: min_voxels must be at least 1");
  if (sizes && capacity == 0) return f3d::fail("f3d_split_components: sizes given with a capacity of 0");
  if (width == 0 || height == 0 || depth == 0) return f3d::fail("f3d_split_components: empty box %zux%zux%zu", width, height, depth);
  const size_t most = (static_cast<size_t>(1) << 31) - 1;
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > most)
    return f3d::fail("f3d_split_components: box %zux%zux%zu exceeds 32768 along an axis or 2^31 - 1 voxels", width, height, depth);
  if (width * width + height * height + depth * depth > most)
    return f3d::fail("f3d_split_components: box %zux%zux%zu has a squared diagonal above 2^31 - 1", width, height, depth);
  if (depth > f3d::container().depth)
    return f3d::fail("f3d_split_components: box %zux%zux%zu is deeper than the container (%zu planes)", width, height, depth,
                     f3d::container().depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_split_components")) return 1;

  const size_t n = width * height * depth;
  const size_t sizes_room = sizes ? std::min(capacity, n) : 0;  // a class need not be connected: every voxel may be one
  // counters | eight words per voxel | the four statistics per span | sizes, each part on a 256-byte boundary
  enum {
    kFinal = 0,
    kOfCores = kCounters,
    kOfNearest = 2 * kCounters,
    kOfSplit = 2 * kCounters + f3d_near::kCounters,
    kAllCounters = kOfSplit + kSplitCounters
  };
  const size_t at_words = round_up(kAllCounters * sizeof(u64), 256);
  const size_t part = round_up(n * sizeof(unsigned), 256);
  const size_t at_sums = at_words + 8 * part;
  const size_t at_sizes = at_sums + span_stats_bytes(n);
  const size_t bytes = at_sizes + round_up(sizes_room * sizeof(unsigned), 256);
  void* d_buf;
  if (f3d::scratch_buffer(bytes, &d_buf)) return 1;
  char* base = static_cast<char*>(d_buf);
  u64* counters = reinterpret_cast<u64*>(base);
  unsigned* word[8];
  for (int k = 0; k < 8; ++k) word[k] = reinterpret_cast<unsigned*>(base + at_words + k * part);
  unsigned* comp = word[0];
  unsigned* comp_aux = word[1];  // the sizes of the components, which nobody asks for; later the table of the core bodies
  int* d2 = reinterpret_cast<int*>(word[2]);  // later the table of the remainders
  int* ax = reinterpret_cast<int*>(word[3]);  // later the sizes and numbers of the classes
  int* axy = reinterpret_cast<int*>(word[4]);
  unsigned* stack = word[5];
  unsigned* core = word[6];
  unsigned* cls = word[7];  // first the sizes of the core bodies, which nobody asks for
  unsigned* core_min = comp_aux;
  unsigned* remainder_min = word[2];
  unsigned* aux = word[3];
  const SpanStats stats = span_stats_at(base + at_sums, n);
  unsigned* d_sizes = reinterpret_cast<unsigned*>(base + at_sizes);

  hipStream_t stream = f3d::stream();
  F3D_HIP(hipMemsetAsync(counters, 0, kAllCounters * sizeof(u64), stream));
  const Box b = {g.W, g.H, g.D, static_cast<unsigned>(width * height)};
  const f3d_near::Box nb = {g.W, g.H, g.D};
  const dim3 tiles = tile_grid(b), tile(kBX, kBY, 1);

  const Threshold threshold = {f3d_ptr<const float>(src), lo, hi, g};
  if (union_passes(stream, threshold, b, comp, comp_aux, counters + kFinal)) return 1;
  const BackgroundSeeds background = {comp, nb};
  const StoreD2 store_d2 = {d2, nb};
  if (f3d_near::launch(stream, nb, background, store_d2, ax, axy, stack, counters + kOfNearest)) return 1;
  const CoreMask core_mask = {comp, d2, core_d2, nb};
  if (union_passes(stream, core_mask, b, core, cls, counters + kOfCores)) return 1;
  const CoreSeeds core_seeds = {core, nb};
  const StoreClass store_class = {comp, core, cls, nb};
  if (f3d_near::launch(stream, nb, core_seeds, store_class, ax, axy, stack, counters + kOfNearest)) return 1;
  F3D_HIP(hipMemsetAsync(core_min, 0xff, n * sizeof(unsigned), stream));
  F3D_HIP(hipMemsetAsync(remainder_min, 0xff, n * sizeof(unsigned), stream));
  F3D_HIP(hipMemsetAsync(aux, 0, n * sizeof(unsigned), stream));
  hipLaunchKernelGGL(k_class_min, tiles, tile, 0, stream, b, cls, core_min, remainder_min);
  F3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_class_root, tiles, tile, 0, stream, b, cls, core_min, remainder_min, aux, comp, core, counters + kOfSplit);
  F3D_HIP(hipGetLastError());
  if (number_passes(stream, g, b, n, min_voxels, cls, aux, stats, d_sizes, sizes_room, f3d_ptr<int>(labels_out), counters + kFinal)) return 1;

  u64 c[kAllCounters];
  F3D_HIP(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  F3D_HIP(hipStreamSynchronize(stream));
  const size_t handed = sizes ? static_cast<size_t>(std::min<u64>(c[kLabels], sizes_room)) : 0;
  if (download_sizes(stream, d_sizes, handed, sizes)) return 1;
  info->foreground = c[kForeground];
  info->background = static_cast<u64>(n) - c[kForeground];
  info->nan = c[kNan];
  info->n_components = c[kComponents];
  info->n_labels = c[kLabels];
  info->dropped_components = c[kDroppedComponents];
  info->dropped_voxels = c[kDroppedVoxels];
  info->largest = c[kLargest];
  info->connected_components = c[kOfSplit + kConnected];
  info->core_voxels = c[kOfCores + kForeground];
  info->n_cores = c[kOfSplit + kCores];
  info->remainder_bodies = c[kOfSplit + kRemainderBodies];
  info->remainder_voxels = c[kOfSplit + kRemainderVoxels];
  return 0;
}

}  // extern "C"
