// Exact squared Euclidean distance and nearest-seed (feature) transform for gfx950 (f3d_nearest_seed): for every voxel of the box the
// seed that minimises (squared distance, box index), its squared distance, box index and value.  The definition is include/f3d.h's;
// tests/nearest_ref.py restates it in numpy and every word matches bit for bit.
//
// Three launches (f3d_nearest_passes.h), each line of each the work of one wave or one lane and independent of every other line:
//   k_near_x   a wave per row, 64 columns a step, one ballot per step and a carry from either side
//   k_near_y   a lane per column of a plane, the lower envelope of the parabolas with a stack (f3d_envelope.h)
//   k_near_z   a lane per column along z, the same; writes the outputs and takes the largest distance
// Scratch, in the grow-only buffer of the calling thread (f3d::scratch_buffer): 12 B per voxel of the box (the row result, the plane
// result, the stacks) and two counters.  All integers: no float instruction touches a distance, and the float form of d2_out is one conversion at the store.
#include "f3d_internal.h"
#include "f3d_nearest_passes.h"

namespace {

using f3d_near::Box;
using f3d_near::u64;

struct SeedsOfContainer {
  const int* __restrict__ seeds;
  F3dGeo g;
  bool nonzero;
  __device__ __forceinline__ bool operator()(int x, int y, int z) const { return (seeds[f3d_row(g, y, z) + x] != 0) == nonzero; }
};

struct OutputsOfContainer {
  const int* __restrict__ seeds;
  int* d2;
  int* index;
  int* value;
  F3dGeo g;
  int W, H;
  bool as_float;
  __device__ __forceinline__ void operator()(int x, int y, int z, int dist, int sx, int sy, int sz) const
  {
    const size_t at = f3d_row(g, y, z) + x;
    if (d2) d2[at] = as_float ? __float_as_int(static_cast<float>(dist)) : dist;  // to nearest even: the one float instruction
    if (index) index[at] = sx < 0 ? -1 : sx + W * (sy + H * sz);
    if (value) value[at] = sx < 0 ? 0 : seeds[f3d_row(g, sy, sz) + sx];
  }
};

size_t round_up(size_t n, size_t to) { return (n + to - 1) / to * to; }

}  // namespace

extern "C" {

int f3d_nearest_seed(f3d_devptr seeds, unsigned mode, unsigned flags, f3d_devptr d2_out, f3d_devptr index_out, f3d_devptr value_out,
                     size_t width, size_t height, size_t depth, f3d_nearest_info* info)
{
  F3D_REQUIRE_READY("f3d_nearest_seed");
  if (!seeds) return f3d::fail("f3d_nearest_seed: null seeds");
  if (!info) return f3d::fail("f3d_nearest_seed: null info");
  if (!d2_out && !index_out && !value_out) return f3d::fail("f3d_nearest_seed: no output selected");
  const f3d_devptr outs[3] = {d2_out, index_out, value_out};
  const char* const names[3] = {"d2_out", "index_out", "value_out"};
  for (int i = 0; i < 3; ++i) {
    if (outs[i] && outs[i] == seeds) return f3d::fail("f3d_nearest_seed: %s is the container of seeds", names[i]);
    for (int k = 0; k < i; ++k)
      if (outs[i] && outs[i] == outs[k]) return f3d::fail("f3d_nearest_seed: %s is the container of %s", names[i], names[k]);
  }
  if (mode != F3D_SEED_NONZERO && mode != F3D_SEED_ZERO) return f3d::fail("f3d_nearest_seed: unknown mode %u", mode);
  if (flags & ~static_cast<unsigned>(F3D_NEAREST_D2_FLOAT)) return f3d::fail("f3d_nearest_seed: unknown flags 0x%x", flags);
  if (width == 0 || height == 0 || depth == 0) return f3d::fail("f3d_nearest_seed: empty box %zux%zux%zu", width, height, depth);
  const size_t most = (static_cast<size_t>(1) << 31) - 1;
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > most)
    return f3d::fail("f3d_nearest_seed: box %zux%zux%zu exceeds 32768 along an axis or 2^31 - 1 voxels", width, height, depth);
  if (width * width + height * height + depth * depth > most)
    return f3d::fail("f3d_nearest_seed: box %zux%zux%zu has a squared diagonal above 2^31 - 1", width, height, depth);
  if (depth > f3d::container().depth)
    return f3d::fail("f3d_nearest_seed: box %zux%zux%zu is deeper than the container (%zu planes)", width, height, depth,
                     f3d::container().depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_nearest_seed")) return 1;

  const size_t n = width * height * depth;
  const size_t at_words = round_up(f3d_near::kCounters * sizeof(u64), 256);
  const size_t part = round_up(n * sizeof(int), 256);
  void* d_buf;
  if (f3d::scratch_buffer(at_words + 3 * part, &d_buf)) return 1;
  char* base = static_cast<char*>(d_buf);
  u64* counters = reinterpret_cast<u64*>(base);
  int* ax = reinterpret_cast<int*>(base + at_words);
  int* axy = reinterpret_cast<int*>(base + at_words + part);
  unsigned* stack = reinterpret_cast<unsigned*>(base + at_words + 2 * part);

  hipStream_t stream = f3d::stream();
  F3D_HIP(hipMemsetAsync(counters, 0, f3d_near::kCounters * sizeof(u64), stream));
  const Box b = {g.W, g.H, g.D};
  const SeedsOfContainer seed = {f3d_ptr<const int>(seeds), g, mode == F3D_SEED_NONZERO};
  const OutputsOfContainer out = {f3d_ptr<const int>(seeds), f3d_ptr<int>(d2_out),  f3d_ptr<int>(index_out), f3d_ptr<int>(value_out), g,
                                  g.W,                       g.H,                   (flags & F3D_NEAREST_D2_FLOAT) != 0};
  if (f3d_near::launch(stream, b, seed, out, ax, axy, stack, counters)) return 1;
  u64 c[f3d_near::kCounters];
  F3D_HIP(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  F3D_HIP(hipStreamSynchronize(stream));
  info->seeds = c[f3d_near::kSeeds];
  info->d2_max = c[f3d_near::kD2Max];
  info->unreached = c[f3d_near::kSeeds] ? 0 : static_cast<u64>(n);
  return 0;
}

}  // extern "C"
