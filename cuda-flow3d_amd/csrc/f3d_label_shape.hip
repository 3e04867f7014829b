// Shape sums of labelled bodies for gfx950 (f3d_label_shape_sums): per label the voxel count, the extents, the first and second
// coordinate moments, the equal-label pairs along 13 directions, the unit squares, the 2x2x2 blocks and the voxels on the box border.
// The definitions are those of include/f3d.h; tests/label_shape_ref.py restates them in numpy and every word matches bit for bit.  The
// solve from these sums to axes, surface and Euler number is host code (host/label_shape.cpp, f3d_label_shape_solve).
//
// The sums are exact integers, so no order has to be fixed: integer atomics give the same bytes whatever the schedule.  No float
// instruction touches a label.  No lane ever waits for another lane or workgroup: every loop has a compile-time bound, a claimed
// slot's words start at zero and the adds and maxima to them commute, so a claim and the updates of other lanes need no ordering.
//
// Shape: k_label_contacts' (f3d_label_contacts.hip).  A wave on 64 consecutive x of one row, a workgroup kBY rows, a lane marching over
// kZ planes of its own column with the next plane's loads in flight.  A voxel at plane z owns 13 pairs: four inside its plane, towards
// (1,0,0) (0,1,0) (1,1,0) (1,-1,0), and nine to plane z + 1, one per (dx, dy) in {-1,0,1}^2; together each of the 13 directions once
// (a direction the header writes with dz = -1 is counted at its end in the lower plane).  It owns the three unit squares and the
// 2x2x2 block that start at it towards +x, +y, +z.
// A lane therefore holds rows y-1, y, y+1 of two planes at x-1, x, x+1: 18 labels.  It loads its own x of the three rows (of which
// two are rows its own workgroup's waves load too: L2 hits; the halo rows are half of the 4 B per voxel again), x-1 and x+1 come by
// cross-lane moves, and lanes 0 and 63 load their outer neighbour themselves.  No LDS staging and so no barrier inside the march: the
// alternative, the (64+2) x (4+2) rows of a plane in LDS, was not built.  A neighbour outside the box is read as 0, which never equals
// the label of a body; container padding is never loaded.  A wave-uniform fast path (a ballot that finds everything the wave holds of
// both planes equal, then constants instead of compares) was built and measured slower on both timed volumes, and is not here
// (LABBOOK.md has the numbers).
//
// A lane accumulates in 32-bit registers while the label of its column stays the same (background and foreign voxels do not end a
// run), with z relative to the tile, and closes the run into the workgroup's LDS table keyed on the label: kSlots slots, claimed by
// atomicCAS within kProbes steps; 6 words of 64 bits (s2: a tile's sum reaches 2^43) and 30 of 32 bits (everything else stays below
// 2^28 over the 2^13 voxels of a tile), the extents among them as atomicMax of x and of N-1-x so that zero is the identity.  A run
// that finds no slot goes straight to the label's global row (slow, correct).  At the end of a tile every occupied slot is flushed,
// 36 lanes one word each to consecutive addresses.
// Global row of a label, 36 words = 288 B:  [0] n  [1..3] max(N-1-x)  [4..6] max(x)  [7..9] s1  [10..15] s2 (xx yy zz xy xz yz)
//   [16..28] pairs  [29..31] squares (xy xz yz)  [32] cubes  [33..35] border.  Then the three counters of f3d_label_shape_info.
#include <vector>

#include "f3d_internal.h"
#include "f3d_partials.h"

namespace {

using namespace f3d_partials;

constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;
constexpr int kSlots = 128;  // a power of two
constexpr int kSlotBits = 7;
constexpr int kProbes = 16;
constexpr int kRowWords = 36;
constexpr int kWide = 6;      // the s2 words of a slot, 64 bits
constexpr int kWideAt = 10;   // where they lie in a row
constexpr int kNarrow = kRowWords - kWide;
constexpr int kExtentAt = 1, kExtents = 6;  // words 1 .. 6 of a row are maxima, every other word a sum
constexpr int kInfoWords = 3;
constexpr size_t kMaxLabels = static_cast<size_t>(1) << 22;

typedef unsigned long long u64;

// the labels of one plane around a lane's column: r[dy + 1][dx + 1], 0 outside the box
struct Plane {
  int r[3][3];
};

// what a lane loaded of one plane: its own x of rows y-1, y, y+1, and (lanes 0 and 63 only) the neighbour outside the wave
struct Raw {
  int c[3], e[3];
};

// what a lane has gathered of one label since it last changed; z is relative to the tile
struct Run {
  int n, sz, szz, z_first, z_last, border_z, pairs[13], squares[3], cubes;
  __device__ __forceinline__ void clear(int z)
  {
    n = sz = szz = border_z = cubes = 0;
    z_first = z_last = z;
    for (int k = 0; k < 13; ++k) pairs[k] = 0;
    for (int k = 0; k < 3; ++k) squares[k] = 0;
  }
};

__device__ __forceinline__ bool is_extent(int word) { return word >= kExtentAt && word < kExtentAt + kExtents; }

// one word into a label's global row
__device__ __forceinline__ void to_row(u64* row, int word, u64 v)
{
  if (v == 0) return;
  if (is_extent(word))
    atomicMax(row + word, v);
  else
    atomicAdd(row + word, v);
}

// the slot of `label` in the workgroup's table, claimed if need be; -1 when none is free within kProbes steps
__device__ __forceinline__ int find_slot(int label, int* keys)
{
  unsigned at = (static_cast<unsigned>(label) * 2654435761u) >> (32 - kSlotBits);
  for (int probe = 0; probe < kProbes; ++probe) {
    // labels here are 1 .. n_labels: 0 is a free slot.  A key never changes once set and most runs meet their own
    int seen = __atomic_load_n(&keys[at], __ATOMIC_RELAXED);
    if (seen == 0) seen = atomicCAS(&keys[at], 0, label);
    if (seen == 0 || seen == label) return static_cast<int>(at);
    at = (at + 1) & (kSlots - 1);
  }
  return -1;
}

// the 36 words of a closed run of the column (x, y) whose tile starts at plane z0
__device__ __forceinline__ void run_words(const Run& s, int x, int y, int z0, const F3dGeo& g, u64 out[kRowWords])
{
  const u64 n = s.n, X = x, Y = y, Z0 = z0;
  const u64 sz = Z0 * n + s.sz;                                // sum (z0 + zr)
  const u64 szz = Z0 * Z0 * n + 2 * Z0 * s.sz + s.szz;         // sum (z0 + zr)^2
  out[0] = n;
  out[1] = g.W - 1 - x;
  out[2] = g.H - 1 - y;
  out[3] = g.D - 1 - (z0 + s.z_first);
  out[4] = X;
  out[5] = Y;
  out[6] = Z0 + s.z_last;
  out[7] = X * n;
  out[8] = Y * n;
  out[9] = sz;
  out[10] = X * X * n;
  out[11] = Y * Y * n;
  out[12] = szz;
  out[13] = X * Y * n;
  out[14] = X * sz;
  out[15] = Y * sz;
#pragma unroll
  for (int k = 0; k < 13; ++k) out[16 + k] = s.pairs[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) out[29 + k] = s.squares[k];
  out[32] = s.cubes;
  out[33] = n * ((x == 0 ? 1 : 0) + (x == g.W - 1 ? 1 : 0));
  out[34] = n * ((y == 0 ? 1 : 0) + (y == g.H - 1 ? 1 : 0));
  out[35] = s.border_z;
}

__device__ __forceinline__ void close_run(const Run& s, int label, int x, int y, int z0, const F3dGeo& g, int* keys, u64* wide,
                                          unsigned* narrow, u64* table)
{
  u64 words[kRowWords];
  run_words(s, x, y, z0, g, words);
  const int slot = find_slot(label, keys);
  if (slot < 0) {
    u64* row = table + static_cast<size_t>(label - 1) * kRowWords;
#pragma unroll
    for (int i = 0; i < kRowWords; ++i) to_row(row, i, words[i]);
    return;
  }
#pragma unroll
  for (int i = 0; i < kRowWords; ++i) {
    if (words[i] == 0) continue;
    if (i >= kWideAt && i < kWideAt + kWide) {
      atomicAdd(wide + slot * kWide + (i - kWideAt), words[i]);
    } else {
      unsigned* at = narrow + slot * kNarrow + (i < kWideAt ? i : i - kWide);
      if (is_extent(i))
        atomicMax(at, static_cast<unsigned>(words[i]));
      else
        atomicAdd(at, static_cast<unsigned>(words[i]));
    }
  }
}

// include/f3d.h, f3d_label_shape_sums.  table: n_labels rows of kRowWords, then the kInfoWords counters of f3d_label_shape_info.
// A wave is one row of 64 x: threadIdx.y and with it `row` are the same for all its lanes, so every lane of a wave reaches every
// cross-lane move.
__global__ __launch_bounds__(kBX* kBY) void k_label_shape_sums(const int* __restrict__ labels, int n_labels, F3dGeo g,
                                                               u64* __restrict__ table)
{
  __shared__ u64 wide[kSlots * kWide];
  __shared__ unsigned narrow[kSlots * kNarrow];
  __shared__ int keys[kSlots];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  for (int i = tid; i < kSlots * kWide; i += kBX * kBY) wide[i] = 0;
  for (int i = tid; i < kSlots * kNarrow; i += kBX * kBY) narrow[i] = 0;
  for (int i = tid; i < kSlots; i += kBX * kBY) keys[i] = 0;
  __syncthreads();

  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const bool row = y < g.H;
  const bool col = row && x < g.W;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  // the outer neighbour a lane loads itself: lane 0 the voxel to its left, lane 63 the one to its right, when inside the box
  const int ex = threadIdx.x == 0 ? x - 1 : (threadIdx.x == kBX - 1 ? x + 1 : -1);
  const bool has_e = row && ex >= 0 && ex < g.W;

  // what the lane loads of plane z: nothing but voxels of the box
  auto load = [&](int z) {
    Raw p = {{0, 0, 0}, {0, 0, 0}};
    if (z >= g.D) return p;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int yy = y + j - 1;
      if (!row || yy < 0 || yy >= g.H) continue;
      const size_t at = f3d_row(g, yy, z);
      if (col) p.c[j] = labels[at + x];
      if (has_e) p.e[j] = labels[at + ex];
    }
    return p;
  };
  // the 3 x 3 labels around the lane's column from what the wave loaded; every lane of the wave is here
  auto spread = [&](const Raw& p) {
    Plane q;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      int left = __shfl_up(p.c[j], 1), right = __shfl_down(p.c[j], 1);
      if (threadIdx.x == 0) left = p.e[j];
      if (threadIdx.x == kBX - 1) right = p.e[j];
      q.r[j][0] = left;
      q.r[j][1] = p.c[j];
      q.r[j][2] = right;
    }
    return q;
  };

  Run run;
  run.clear(0);
  int current = 0;  // the label of the open run, 0: none
  int background = 0, foreign = 0, labelled = 0;

  if (row) {
    Plane cur = spread(load(z_begin));
    Raw ahead = load(z_begin + 1);
    for (int z = z_begin; z < z_end; ++z) {
      const Raw coming = load(z + 2 <= z_end ? z + 2 : g.D);  // in flight while this plane is counted; none beyond the next tile's first
      const Plane up = spread(ahead);
      const int a = cur.r[1][1];
      if (col) {
        if (a == 0) {
          ++background;
        } else if (a < 0 || a > n_labels) {
          ++foreign;
        } else {
          ++labelled;
          const int zr = z - z_begin;
          if (a != current) {
            if (current != 0) close_run(run, current, x, y, z_begin, g, keys, wide, narrow, table);
            run.clear(zr);
            current = a;
          }
          // r[dy + 1][dx + 1]
          const bool px = cur.r[1][2] == a, py = cur.r[2][1] == a, pxy = cur.r[2][2] == a, pz = up.r[1][1] == a;
          const bool pxz = up.r[1][2] == a, pyz = up.r[2][1] == a, pxyz = up.r[2][2] == a;
          ++run.n;
          run.sz += zr;
          run.szz += zr * zr;
          run.z_last = zr;
          run.border_z += (z == 0 ? 1 : 0) + (z == g.D - 1 ? 1 : 0);
          run.pairs[0] += px;                  // ( 1, 0, 0)
          run.pairs[1] += py;                  // ( 0, 1, 0)
          run.pairs[2] += pz;                  // ( 0, 0, 1)
          run.pairs[3] += pxy;                 // ( 1, 1, 0)
          run.pairs[4] += cur.r[0][2] == a;    // ( 1,-1, 0)
          run.pairs[5] += pxz;                 // ( 1, 0, 1)
          run.pairs[6] += up.r[1][0] == a;     // ( 1, 0,-1) from its lower end: (-1, 0, 1)
          run.pairs[7] += pyz;                 // ( 0, 1, 1)
          run.pairs[8] += up.r[0][1] == a;     // ( 0, 1,-1) from its lower end: ( 0,-1, 1)
          run.pairs[9] += pxyz;                // ( 1, 1, 1)
          run.pairs[10] += up.r[0][0] == a;    // ( 1, 1,-1) from its lower end: (-1,-1, 1)
          run.pairs[11] += up.r[0][2] == a;    // ( 1,-1, 1)
          run.pairs[12] += up.r[2][0] == a;    // ( 1,-1,-1) from its lower end: (-1, 1, 1)
          const bool sxy = px && py && pxy, sxz = px && pz && pxz, syz = py && pz && pyz;
          run.squares[0] += sxy;
          run.squares[1] += sxz;
          run.squares[2] += syz;
          run.cubes += sxy && pz && pxz && pyz && pxyz;
        }
      }
      cur = up;
      ahead = coming;
    }
    if (current != 0) close_run(run, current, x, y, z_begin, g, keys, wide, narrow, table);
  }

  // the counters: one add per wave and counter
  const u64 counts[kInfoWords] = {wave_sum(static_cast<u64>(background)), wave_sum(static_cast<u64>(foreign)),
                                  wave_sum(static_cast<u64>(labelled))};
  if (threadIdx.x == 0) {
    u64* info = table + static_cast<size_t>(n_labels) * kRowWords;
    for (int i = 0; i < kInfoWords; ++i)
      if (counts[i]) atomicAdd(info + i, counts[i]);
  }

  // every occupied slot to its label's row: 36 lanes of a wave, one word each, consecutive addresses
  __syncthreads();
  for (int slot = threadIdx.y; slot < kSlots; slot += kBY) {
    const int key = keys[slot];
    if (key == 0 || threadIdx.x >= kRowWords) continue;
    const int word = threadIdx.x;
    const bool is_wide = word >= kWideAt && word < kWideAt + kWide;
    const u64 value = is_wide ? wide[slot * kWide + (word - kWideAt)] : narrow[slot * kNarrow + (word < kWideAt ? word : word - kWide)];
    to_row(table + static_cast<size_t>(key - 1) * kRowWords, word, value);
  }
}

// the calling thread's device buffer of at least `bytes` (grow-only)
int device_buffer(size_t bytes, void** buffer)
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

}  // namespace

extern "C" {

int f3d_label_shape_sums(f3d_devptr labels, size_t n_labels, size_t width, size_t height, size_t depth, struct f3d_label_shape_sums* out,
                         f3d_label_shape_info* info)
{
  F3D_REQUIRE_READY("f3d_label_shape_sums");
  if (!labels) return f3d::fail("f3d_label_shape_sums: null labels");
  if (!out) return f3d::fail("f3d_label_shape_sums: null out");
  if (n_labels == 0 || n_labels > kMaxLabels)
    return f3d::fail("f3d_label_shape_sums: n_labels %zu is outside 1 .. %zu", n_labels, kMaxLabels);
  if (width == 0 || height == 0 || depth == 0) return f3d::fail("f3d_label_shape_sums: empty box %zux%zux%zu", width, height, depth);
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > 0x7fffffffull)
    return f3d::fail("f3d_label_shape_sums: box %zux%zux%zu exceeds 32768 along an axis or 2^31 - 1 voxels", width, height, depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_label_shape_sums")) return 1;
  if (depth > f3d::container().depth)
    return f3d::fail("f3d_label_shape_sums: box %zux%zux%zu is deeper than the container's %zu planes", width, height, depth,
                     f3d::container().depth);

  const size_t words = n_labels * kRowWords + kInfoWords;
  void* d_table;
  if (device_buffer(words * sizeof(u64), &d_table)) return 1;
  F3D_HIP(hipMemsetAsync(d_table, 0, words * sizeof(u64), f3d::stream()));
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ);
  hipLaunchKernelGGL(k_label_shape_sums, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), f3d_ptr<const int>(labels),
                     static_cast<int>(n_labels), g, static_cast<u64*>(d_table));
  F3D_HIP(hipGetLastError());
  std::vector<u64> host(words);
  F3D_HIP(hipMemcpyAsync(host.data(), d_table, words * sizeof(u64), hipMemcpyDeviceToHost, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  const long long dims[3] = {g.W, g.H, g.D};
  for (size_t l = 0; l < n_labels; ++l) {
    const u64* r = host.data() + l * kRowWords;
    struct f3d_label_shape_sums& s = out[l];
    s.n = r[0];
    for (int i = 0; i < 3; ++i) {
      s.lo[i] = s.n ? dims[i] - 1 - static_cast<long long>(r[1 + i]) : 0;
      s.hi[i] = s.n ? static_cast<long long>(r[4 + i]) : -1;
      s.s1[i] = r[7 + i];
      s.squares[i] = r[29 + i];
      s.border[i] = r[33 + i];
    }
    for (int i = 0; i < 6; ++i) s.s2[i] = r[10 + i];
    for (int i = 0; i < 13; ++i) s.pairs[i] = r[16 + i];
    s.cubes = r[32];
  }
  if (info) {
    const u64* c = host.data() + n_labels * kRowWords;
    info->background = c[0];
    info->foreign = c[1];
    info->labelled = c[2];
  }
  return 0;
}

}  // extern "C"
