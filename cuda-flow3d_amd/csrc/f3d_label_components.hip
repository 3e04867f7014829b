// Connected bodies of a thresholded volume for gfx950 (f3d_label_components): the foreground voxels of the box are joined over their
// six faces and every body of at least min_voxels voxels gets a number, in ascending order of its smallest linear index.  The
// definition is include/f3d.h's; tests/components_ref.py restates it in numpy and every label, size and counter matches bit for bit.
//
// A union-find over one 32-bit parent per voxel (f3d_union_find.h: find, unite, flatten; DESIGN.md §22 argues termination and what the
// result rests on).  Indices are linear in the BOX, x + W (y + H z), not in the container: the root of a body is then its smallest
// index by construction, because a root only ever hangs below a smaller one.  Scratch, in a grow-only buffer of the calling thread:
// parent (4 B per voxel), aux (4 B per voxel: the size of a body at its root, later its number), 20 B per 1024 voxels for the prefix
// sum and the counters, and 4 B per size handed out.
//
// Launches, all on the library stream, each reading only what an earlier launch wrote or what an atomic returned to it:
//   k_tile      classify, count, and the union-find of one 64 x 4 x 32 tile in LDS; parent = the box index of the root inside the tile
//   k_merge<0>  the faces on the seams between tiles towards +y and +x         \  a face whose -x neighbour face joins the same two runs
//   k_flatten<false>  parent = root: the walks of the next launch start at a root   >  is left out: that one does the work
//   k_merge<1>  the faces on the seams towards +z                              /
//   k_flatten<true>   parent = root; the head of every run adds the run's length to aux[root]
//   k_flag_sums   per 1024 voxels in linear order: how many roots of at least min_voxels, and what the counters of the info need
//   k_scan_sums   one workgroup, kScanThreads sums per trip: exclusive prefix of those counts (the total is n_labels); the counters
//   k_number      aux[root] = its number (0 when dropped), sizes by number
//   k_write       labels_out = aux[parent], 0 for background
// No lane waits for another lane or workgroup: every loop is bounded at compile time, by the box, or walks a strictly decreasing index.
// No float instruction touches a label: labels_out is written as int.  The kernels are in f3d_components_passes.h, which
// f3d_split_components shares; the scratch buffer is the one every labelled-body entry of the calling thread uses (f3d::scratch_buffer).
#include <algorithm>
#include <cmath>

#include "f3d_internal.h"

namespace f3d_cc {
namespace {
constexpr int kScanBlock = 256;    // threads of k_flag_sums and k_number
constexpr int kScanItems = 4;      // consecutive voxels per thread
constexpr int kScanThreads = 1024;  // block sums per trip of k_scan_sums
}  // namespace
}  // namespace f3d_cc
#include "f3d_components_passes.h"

namespace f3d {

// the calling thread's device buffer of at least `bytes` (grow-only), shared by the entries that run one after another on it
int scratch_buffer(size_t bytes, void** buffer)
{
  static thread_local void* d_buf = nullptr;
  static thread_local size_t d_bytes = 0;
  if (d_bytes < bytes) {
    if (d_buf) F3D_HIP(hipFree(d_buf));
    d_buf = nullptr;
    d_bytes = 0;
    F3D_HIP(hipMalloc(&d_buf, bytes));
    d_bytes = bytes;
  }
  *buffer = d_buf;
  return 0;
}

}  // namespace f3d

namespace {

using namespace f3d_cc;

size_t round_up(size_t n, size_t to) { return (n + to - 1) / to * to; }

}  // namespace

extern "C" {

int f3d_label_components(f3d_devptr src, float lo, float hi, unsigned long long min_voxels, f3d_devptr labels_out, size_t width,
                         size_t height, size_t depth, unsigned long long* sizes, size_t capacity, f3d_component_info* info)
{
  F3D_REQUIRE_READY("f3d_label_components");
  if (!src) return f3d::fail("f3d_label_components: null src");
  if (!labels_out) return f3d::fail("f3d_label_components: null labels_out");
  if (!info) return f3d::fail("f3d_label_components: null info");
  if (src == labels_out) return f3d::fail("f3d_label_components: labels_out is the container of src");
  if (std::isnan(lo) || std::isnan(hi)) return f3d::fail("f3d_label_components: %s is NaN", std::isnan(lo) ? "lo" : "hi");
  if (lo > hi) return f3d::fail("f3d_label_components: lo %g is above hi %g", static_cast<double>(lo), static_cast<double>(hi));
  if (min_voxels == 0) return f3d::fail("f3d_label_components: min_voxels must be at least 1");
  if (sizes && capacity == 0) return f3d::fail("f3d_label_components: sizes given with a capacity of 0");
  if (width == 0 || height == 0 || depth == 0) return f3d::fail("f3d_label_components: empty box %zux%zux%zu", width, height, depth);
  const size_t most = (static_cast<size_t>(1) << 31) - 1;
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > most)
    return f3d::fail("f3d_label_components: box %zux%zux%zu exceeds 32768 along an axis or 2^31 - 1 voxels", width, height, depth);
  if (depth > f3d::container().depth)
    return f3d::fail("f3d_label_components: box %zux%zux%zu is deeper than the container (%zu planes)", width, height, depth,
                     f3d::container().depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_label_components")) return 1;

  const size_t n = width * height * depth;
  const size_t sizes_room = sizes ? std::min(capacity, (n + 1) / 2) : 0;  // two face neighbours are one body: at most every other voxel is one
  // counters | parent | aux | the four statistics per span | sizes, each part on a 256-byte boundary
  const size_t at_parent = round_up(kCounters * sizeof(u64), 256);
  const size_t at_aux = at_parent + round_up(n * sizeof(unsigned), 256);
  const size_t at_sums = at_aux + round_up(n * sizeof(unsigned), 256);
  const size_t at_sizes = at_sums + f3d_cc::span_stats_bytes(n);
  const size_t bytes = at_sizes + round_up(sizes_room * sizeof(unsigned), 256);
  void* d_buf;
  if (f3d::scratch_buffer(bytes, &d_buf)) return 1;
  char* base = static_cast<char*>(d_buf);
  u64* counters = reinterpret_cast<u64*>(base);
  unsigned* parent = reinterpret_cast<unsigned*>(base + at_parent);
  unsigned* aux = reinterpret_cast<unsigned*>(base + at_aux);
  const SpanStats stats = f3d_cc::span_stats_at(base + at_sums, n);
  unsigned* d_sizes = reinterpret_cast<unsigned*>(base + at_sizes);

  hipStream_t stream = f3d::stream();
  F3D_HIP(hipMemsetAsync(counters, 0, kCounters * sizeof(u64), stream));
  const Box b = {g.W, g.H, g.D, static_cast<unsigned>(width * height)};
  const f3d_cc::Threshold classify = {f3d_ptr<const float>(src), lo, hi, g};
  if (f3d_cc::union_passes(stream, classify, b, parent, aux, counters)) return 1;
  if (f3d_cc::number_passes(stream, g, b, n, min_voxels, parent, aux, stats, d_sizes, sizes_room, f3d_ptr<int>(labels_out), counters)) return 1;

  u64 c[kCounters];
  F3D_HIP(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  F3D_HIP(hipStreamSynchronize(stream));
  const size_t handed = sizes ? static_cast<size_t>(std::min<u64>(c[kLabels], sizes_room)) : 0;
  if (f3d_cc::download_sizes(stream, d_sizes, handed, sizes)) return 1;
  info->foreground = c[kForeground];
  info->background = static_cast<u64>(n) - c[kForeground];
  info->nan = c[kNan];
  info->n_components = c[kComponents];
  info->n_labels = c[kLabels];
  info->dropped_components = c[kDroppedComponents];
  info->dropped_voxels = c[kDroppedVoxels];
  info->largest = c[kLargest];
  return 0;
}

}  // extern "C"
