// Overlap of two labelled volumes through a displacement for gfx950 (f3d_label_overlap), and the relabelling that follows a track
// (f3d_relabel_labels).  The classes, the keys, the sums and the table are those of include/f3d.h; tests/overlap_ref.py restates them
// in numpy and every field matches bit for bit.  The solve from the rows to the tracks is host code (host/label_track.cpp).
//
// The sums are exact integers, so no order has to be fixed: integer atomics give the same bytes whatever the schedule.  The only float
// instructions are the header's: one add per axis for the position, the comparisons of `inside`, the add of 0.5f and the floor.  No
// lane ever waits for another lane or workgroup: every loop has a compile-time bound, a claimed slot's words start at zero and the adds
// to them commute, so a claim and the adds of other lanes need no ordering.
//
// Shape: k_label_contacts' and k_label_shape_sums'.  A wave on 64 consecutive x of one row, a workgroup kBY rows, a lane marching over
// kZ planes of its own column.  Three stages are in flight per lane: the label of A and u, v, w of plane z + 2 are being loaded, the
// label of B at the target of plane z + 1 is being gathered (a plain 4-B load per lane: under a smooth flow the lanes of a wave read
// neighbouring words of one or two rows), and plane z is counted.  Nothing is staged in LDS.
// Unlike a contact, every foreground voxel carries a key, so the atomics are taken off the voxel: a lane keeps its key and the sums
// since the key last changed in 32-bit registers (z relative to the tile; voxels without a key do not end a run) and closes the run
// into the workgroup's LDS table: kSlots slots of a 64-bit key and kWords = 7 words of 64 bits (8 KiB), claimed by a 64-bit atomicCAS
// within kProbes steps.  A run that finds no LDS slot goes straight to the global table (slow, correct).  At the end of a tile every
// occupied slot is flushed: one lane finds the global row, seven add consecutive words.  The global table is f3d_label_contacts': a
// power of two of at least 2 * capacity rows of key + 7 words (64 B), zeroed on the stream, a row claimed by a 64-bit global atomicCAS
// within kGlobalProbes linear steps.  Voxels whose run or slot finds no row are counted in table_lost, and the entry then hands out no
// table at all.  k_compact_overlap packs the occupied rows into a dense list, so the download is n_pairs rows; the host sorts them.
//
// Key: (a << 32) | (b + 1) with b = -1 for the lost part of a body.  (0, 0) and (0, -1) are classes without a key, so no key is 0, and
// the order of the keys as unsigned 64-bit numbers is the order of (a, b) as signed ints.
// Row words after the key: [0] n  [1..3] ca2  [4..6] cb2.
// Counters (8 words in front of the table): foreign_a, lost_background, lost_body, foreign_b, background, overlap, table_lost, occupied.
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "f3d_gather.h"
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
constexpr int kGlobalProbes = 256;
constexpr int kWords = 7;
constexpr int kRowWords = kWords + 1;  // a global row: the key, then the words
constexpr int kCounters = 8;
constexpr int kClasses = 6;
constexpr int kTableLost = 6, kOccupied = 7;
constexpr size_t kMaxLabels = static_cast<size_t>(1) << 22;
constexpr size_t kMaxCapacity = static_cast<size_t>(1) << 24;
constexpr unsigned long long kHash = 0x9E3779B97F4A7C15ull;

typedef unsigned long long u64;

struct GlobalTable {
  u64* counters;  // kCounters words
  u64* slots;     // (mask + 1) rows of kRowWords
  unsigned mask;
  int shift;  // 64 - log2(mask + 1)
};

// what a lane loads of one plane of its column
struct Source {
  float u, v, w;
  int a;
};

// a voxel of A after the header's first two steps: its class so far and, when it goes on to B, where it lands
struct Target {
  int a;        // the label of A
  int state;    // kOutside, kForeignA, kLost or kLanded
  int yx, yy, yz;  // the voxel of B, kLanded only
};
constexpr int kOutside = 0, kForeignA = 1, kLost = 2, kLanded = 3;

// what a lane has gathered of one key since it last changed; z is relative to the tile, the coordinates of B are doubled about the centre
struct Run {
  int n, sz, cb[3];
  __device__ __forceinline__ void clear() { n = sz = cb[0] = cb[1] = cb[2] = 0; }
};

__device__ __forceinline__ void add_word(u64* p, long long v)
{
  if (v != 0) atomicAdd(p, static_cast<u64>(v));  // two's complement: the wrapped sum is the signed one
}

// the slot of `key` in the workgroup's table, claimed if need be; -1 when none is free within kProbes steps
__device__ __forceinline__ int find_slot(u64 key, u64* keys)
{
  unsigned at = static_cast<unsigned>((key * kHash) >> (64 - kSlotBits));
  for (int probe = 0; probe < kProbes; ++probe) {
    // no key is 0: 0 is a free slot.  A key never changes once set and most runs meet their own
    u64 seen = __atomic_load_n(&keys[at], __ATOMIC_RELAXED);
    if (seen == 0) seen = atomicCAS(&keys[at], 0ull, key);
    if (seen == 0 || seen == key) return static_cast<int>(at);
    at = (at + 1) & (kSlots - 1);
  }
  return -1;
}

// the row of `key` in the global table, claimed if need be; null when none is free within kGlobalProbes steps
__device__ __forceinline__ u64* find_row(u64 key, const GlobalTable& t)
{
  unsigned at = static_cast<unsigned>((key * kHash) >> t.shift) & t.mask;
  for (int probe = 0; probe < kGlobalProbes; ++probe) {
    u64* row = t.slots + static_cast<size_t>(at) * kRowWords;
    u64 seen = __atomic_load_n(row, __ATOMIC_RELAXED);  // a key never changes once set: most flushes meet their own
    if (seen == 0) seen = atomicCAS(row, 0ull, key);
    if (seen == 0 || seen == key) return row;
    at = (at + 1) & t.mask;
  }
  return nullptr;
}

// the closed run of the column (x, y) whose tile starts at plane z0 into the workgroup's table, or past it into the call's
__device__ __forceinline__ void close_run(const Run& s, u64 key, int x, int y, int z0, const F3dGeo& g, u64* keys, u64* slots,
                                          const GlobalTable& t)
{
  const long long n = s.n;
  const long long words[kWords] = {n,
                                   n * (2 * x - (g.W - 1)),
                                   n * (2 * y - (g.H - 1)),
                                   2ll * s.sz + n * (2 * z0 - (g.D - 1)),  // sum (2 (z0 + zr) - (D - 1))
                                   s.cb[0],
                                   s.cb[1],
                                   s.cb[2]};
  const int slot = find_slot(key, keys);
  u64* to = slot >= 0 ? slots + slot * kWords : nullptr;
  if (!to) {
    u64* row = find_row(key, t);
    if (!row) {
      atomicAdd(t.counters + kTableLost, static_cast<u64>(n));
      return;
    }
    to = row + 1;
  }
#pragma unroll
  for (int i = 0; i < kWords; ++i) add_word(to + i, words[i]);
}

// include/f3d.h, f3d_label_overlap.  A wave is one row of 64 x: threadIdx.y and with it `row` are the same for all its lanes.
template <bool FLOW>
__global__ __launch_bounds__(kBX* kBY) void k_label_overlap(const int* __restrict__ labels_a, int n_a, const int* __restrict__ labels_b,
                                                            int n_b, const float* __restrict__ du, const float* __restrict__ dv,
                                                            const float* __restrict__ dw, F3dGeo g, GlobalTable t)
{
  __shared__ u64 slots[kSlots * kWords];
  __shared__ u64 keys[kSlots];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  for (int i = tid; i < kSlots * kWords; i += kBX * kBY) slots[i] = 0;
  for (int i = tid; i < kSlots; i += kBX * kBY) keys[i] = 0;
  __syncthreads();

  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const bool col = y < g.H && x < g.W;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);

  // plane z of the lane's column: nothing but voxels of the box, and of this tile
  auto load = [&](int z) {
    Source p = {0.f, 0.f, 0.f, 0};
    if (col && z < z_end) {
      const size_t i = f3d_row(g, y, z) + x;
      if (FLOW) {
        p.u = du[i];
        p.v = dv[i];
        p.w = dw[i];
      }
      p.a = labels_a[i];
    }
    return p;
  };
  // the header's steps 1 and 2 of the voxel (x, y, z)
  auto aim = [&](const Source& p, int z) {
    Target q = {p.a, kOutside, 0, 0, 0};
    if (!col || z >= z_end) return q;
    if (p.a < 0 || p.a > n_a) {
      q.state = kForeignA;
      return q;
    }
    if (FLOW) {
      const float x_f = static_cast<float>(x) + p.u, y_f = static_cast<float>(y) + p.v, z_f = static_cast<float>(z) + p.w;
      if (!f3d_gather::inside(g, x_f, y_f, z_f)) {
        q.state = kLost;
        return q;
      }
      q.yx = min(g.W - 1, static_cast<int>(floorf(x_f + 0.5f)));
      q.yy = min(g.H - 1, static_cast<int>(floorf(y_f + 0.5f)));
      q.yz = min(g.D - 1, static_cast<int>(floorf(z_f + 0.5f)));
    } else {
      q.yx = x;
      q.yy = y;
      q.yz = z;
    }
    q.state = kLanded;
    return q;
  };
  // the label of B where the voxel lands: inside the box by `inside` and the clamp
  auto gather = [&](const Target& q) { return q.state == kLanded ? labels_b[f3d_row(g, q.yy, q.yz) + q.yx] : 0; };

  Run run;
  run.clear();
  u64 current = 0;  // the key of the open run, 0: none
  int counts[kClasses] = {0, 0, 0, 0, 0, 0};

  Target cur = aim(load(z_begin), z_begin);
  int cur_b = gather(cur);
  Source ahead = load(z_begin + 1);
  for (int z = z_begin; z < z_end; ++z) {
    const Source coming = load(z + 2);           // in flight while this plane is counted
    const Target next = aim(ahead, z + 1);
    const int next_b = gather(next);             // in flight too
    if (cur.state == kForeignA) {
      ++counts[0];
    } else if (cur.state != kOutside) {
      const int a = cur.a;
      const bool lost = cur.state == kLost;
      int b = -1;
      bool keyed = false;
      if (lost) {
        ++counts[a == 0 ? 1 : 2];
        keyed = a != 0;
      } else if (cur_b < 0 || cur_b > n_b) {
        ++counts[3];
      } else if (a == 0 && cur_b == 0) {
        ++counts[4];
      } else {
        ++counts[5];
        b = cur_b;
        keyed = true;
      }
      if (keyed) {
        const u64 key = (static_cast<u64>(static_cast<unsigned>(a)) << 32) | static_cast<u64>(static_cast<unsigned>(b + 1));
        if (key != current) {
          if (current != 0) close_run(run, current, x, y, z_begin, g, keys, slots, t);
          run.clear();
          current = key;
        }
        ++run.n;
        run.sz += z - z_begin;
        if (!lost) {
          run.cb[0] += 2 * cur.yx - (g.W - 1);
          run.cb[1] += 2 * cur.yy - (g.H - 1);
          run.cb[2] += 2 * cur.yz - (g.D - 1);
        }
      }
    }
    cur = next;
    cur_b = next_b;
    ahead = coming;
  }
  if (current != 0) close_run(run, current, x, y, z_begin, g, keys, slots, t);

  // the counters: one add per wave and counter
#pragma unroll
  for (int i = 0; i < kClasses; ++i) {
    const u64 sum = wave_sum(static_cast<u64>(counts[i]));
    if (threadIdx.x == 0 && sum) atomicAdd(t.counters + i, sum);
  }

  // every occupied slot to its row of the global table: lane 0 finds the row, seven lanes add one word each to consecutive addresses
  __syncthreads();
  for (int slot = threadIdx.y; slot < kSlots; slot += kBY) {
    const u64 key = keys[slot];  // the same for the whole wave
    if (key == 0) continue;
    const int lane = threadIdx.x;
    const long long value = lane < kWords ? static_cast<long long>(slots[slot * kWords + lane]) : 0;
    u64* found = nullptr;
    if (lane == 0) {
      found = find_row(key, t);
      if (!found) atomicAdd(t.counters + kTableLost, static_cast<u64>(value));  // word 0: the voxels of the slot
    }
    const u64 at = __shfl(reinterpret_cast<u64>(found), 0);
    if (at != 0 && lane < kWords) add_word(reinterpret_cast<u64*>(at) + 1 + lane, value);
  }
}

// the occupied rows of the table into a dense list of at most `capacity` rows, in any order; counters[kOccupied] counts them all
__global__ __launch_bounds__(256) void k_compact_overlap(GlobalTable t, u64* __restrict__ dense, unsigned capacity)
{
  const size_t rows = static_cast<size_t>(t.mask) + 1;
  for (size_t r = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < rows; r += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const u64* row = t.slots + r * kRowWords;
    if (row[0] == 0) continue;
    const u64 at = atomicAdd(t.counters + kOccupied, 1ull);
    if (at < capacity)
      for (int i = 0; i < kRowWords; ++i) dense[at * kRowWords + i] = row[i];
  }
}

// include/f3d.h, f3d_relabel_labels: each voxel reads and writes its own word, so out may be labels
__global__ __launch_bounds__(kBX* kBY) void k_relabel_labels(const int* labels, int n, const int* __restrict__ map, int* out, F3dGeo g,
                                                             u64* __restrict__ foreign)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z = blockIdx.z;
  int is_foreign = 0;
  if (x < g.W && y < g.H) {
    const size_t i = f3d_row(g, y, z) + x;
    const int l = labels[i];
    is_foreign = l < 0 || l > n;
    out[i] = (l >= 1 && l <= n) ? map[l - 1] : 0;
  }
  const u64 sum = wave_sum(static_cast<u64>(is_foreign));
  if (threadIdx.x == 0 && sum) atomicAdd(foreign, sum);
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

int f3d_label_overlap(f3d_devptr labels_a, size_t n_a, f3d_devptr labels_b, size_t n_b, f3d_devptr u, f3d_devptr v, f3d_devptr w,
                      size_t width, size_t height, size_t depth, size_t capacity, struct f3d_overlap* out, f3d_overlap_info* info)
{
  F3D_REQUIRE_READY("f3d_label_overlap");
  if (!labels_a) return f3d::fail("f3d_label_overlap: null labels_a");
  if (!labels_b) return f3d::fail("f3d_label_overlap: null labels_b");
  if (!out) return f3d::fail("f3d_label_overlap: null out");
  if (!info) return f3d::fail("f3d_label_overlap: null info");
  const bool flow = u && v && w;
  if (!flow && (u || v || w)) return f3d::fail("f3d_label_overlap: u, v and w must be given all three or not at all");
  if (labels_a == labels_b) return f3d::fail("f3d_label_overlap: labels_a and labels_b are one container");
  for (int s = 0; flow && s < 2; ++s) {
    const f3d_devptr l = s == 0 ? labels_a : labels_b;
    if (u == l || v == l || w == l)
      return f3d::fail("f3d_label_overlap: %s is the container of labels_%c", u == l ? "u" : v == l ? "v" : "w", s == 0 ? 'a' : 'b');
  }
  if (n_a == 0 || n_a > kMaxLabels) return f3d::fail("f3d_label_overlap: n_a %zu is outside 1 .. %zu", n_a, kMaxLabels);
  if (n_b == 0 || n_b > kMaxLabels) return f3d::fail("f3d_label_overlap: n_b %zu is outside 1 .. %zu", n_b, kMaxLabels);
  if (capacity == 0 || capacity > kMaxCapacity)
    return f3d::fail("f3d_label_overlap: capacity %zu is outside 1 .. %zu", capacity, kMaxCapacity);
  if (width == 0 || height == 0 || depth == 0) return f3d::fail("f3d_label_overlap: empty volume %zux%zux%zu", width, height, depth);
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > (static_cast<size_t>(1) << 33))
    return f3d::fail("f3d_label_overlap: volume %zux%zux%zu exceeds 32768 along an axis or 2^33 voxels", width, height, depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_label_overlap")) return 1;

  int bits = 1;
  while ((static_cast<size_t>(1) << bits) < 2 * capacity) ++bits;
  const size_t rows = static_cast<size_t>(1) << bits;
  const size_t table_words = kCounters + rows * kRowWords;
  const size_t words = table_words + capacity * kRowWords;
  void* d_buf;
  if (device_buffer(words * sizeof(u64), &d_buf)) return 1;
  GlobalTable t;
  t.counters = static_cast<u64*>(d_buf);
  t.slots = t.counters + kCounters;
  t.mask = static_cast<unsigned>(rows - 1);
  t.shift = 64 - bits;
  u64* dense = t.counters + table_words;
  F3D_HIP(hipMemsetAsync(d_buf, 0, table_words * sizeof(u64), f3d::stream()));

  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ);
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  const int *pa = f3d_ptr<const int>(labels_a), *pb = f3d_ptr<const int>(labels_b);
  const int na = static_cast<int>(n_a), nb = static_cast<int>(n_b);
  if (flow)
    hipLaunchKernelGGL(k_label_overlap<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pa, na, pb, nb, pu, pv, pw, g, t);
  else
    hipLaunchKernelGGL(k_label_overlap<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pa, na, pb, nb, pu, pv, pw, g, t);
  F3D_HIP(hipGetLastError());
  const unsigned compact_blocks = static_cast<unsigned>(std::min<size_t>((rows + 255) / 256, 2048));
  hipLaunchKernelGGL(k_compact_overlap, dim3(compact_blocks), dim3(256), 0, f3d::stream(), t, dense, static_cast<unsigned>(capacity));
  F3D_HIP(hipGetLastError());

  u64 counters[kCounters];
  F3D_HIP(hipMemcpyAsync(counters, t.counters, sizeof(counters), hipMemcpyDeviceToHost, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  const bool complete = counters[kTableLost] == 0 && counters[kOccupied] <= capacity;
  // a dense row is a key and the seven words in f3d_overlap's order: the rows come down straight into `out` and only the key is
  // rewritten below
  static_assert(sizeof(struct f3d_overlap) == kRowWords * sizeof(u64), "a row of the dense list is a f3d_overlap with the key in front");
  struct Row {
    u64 w[kRowWords];
  };
  Row* rows_out = reinterpret_cast<Row*>(out);
  const size_t count = complete ? static_cast<size_t>(counters[kOccupied]) : 0;
  if (count) {
    F3D_HIP(hipMemcpyAsync(rows_out, dense, count * sizeof(Row), hipMemcpyDeviceToHost, f3d::stream()));
    F3D_HIP(hipStreamSynchronize(f3d::stream()));
  }
  info->foreign_a = counters[0];
  info->lost_background = counters[1];
  info->lost_body = counters[2];
  info->foreign_b = counters[3];
  info->background = counters[4];
  info->overlap = counters[5];
  info->table_lost = counters[kTableLost];
  info->n_pairs = counters[kOccupied];
  info->complete = complete ? 1 : 0;
  if (!complete) return 0;
  // the order of the list depends on the schedule: sorted by key it does not.  (key, index) pairs are sorted, not the 64-B rows; then
  // every row moves once, along the cycles of the permutation
  std::vector<std::pair<u64, size_t>> order(count);
  for (size_t i = 0; i < count; ++i) order[i] = {rows_out[i].w[0], i};
  std::sort(order.begin(), order.end());  // the keys are distinct
  for (size_t start = 0; start < count; ++start) {
    if (order[start].second == start) continue;
    const Row held = rows_out[start];
    size_t to = start;
    for (size_t from = order[to].second; from != start; from = order[to].second) {
      rows_out[to] = rows_out[from];
      order[to].second = to;
      to = from;
    }
    rows_out[to] = held;
    order[to].second = to;
  }
  for (size_t i = 0; i < count; ++i) {
    u64 key;
    std::memcpy(&key, &out[i], sizeof(key));
    out[i].a = static_cast<int>(key >> 32);
    out[i].b = static_cast<int>(key & 0xffffffffull) - 1;
  }
  return 0;
}

int f3d_relabel_labels(f3d_devptr labels, size_t n, const int* map, f3d_devptr out, size_t width, size_t height, size_t depth,
                       unsigned long long* foreign)
{
  F3D_REQUIRE_READY("f3d_relabel_labels");
  if (!labels) return f3d::fail("f3d_relabel_labels: null labels");
  if (!map) return f3d::fail("f3d_relabel_labels: null map");
  if (!out) return f3d::fail("f3d_relabel_labels: null out");
  if (n == 0 || n > kMaxLabels) return f3d::fail("f3d_relabel_labels: n %zu is outside 1 .. %zu", n, kMaxLabels);
  for (size_t l = 0; l < n; ++l)
    if (map[l] < 0) return f3d::fail("f3d_relabel_labels: map[%zu] is %d (label %zu to a negative number)", l, map[l], l + 1);
  if (width > 32768 || height > 32768 || depth > 32768)
    return f3d::fail("f3d_relabel_labels: volume %zux%zux%zu exceeds 32768 along an axis", width, height, depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_relabel_labels")) return 1;

  // the counter, then the map; a buffer of its own, so that a table of f3d_label_overlap on the stream is not disturbed
  static thread_local void* d_buf = nullptr;
  static thread_local size_t d_bytes = 0;
  const size_t bytes = sizeof(u64) + n * sizeof(int);
  if (d_bytes < bytes) {
    if (d_buf) F3D_HIP(hipFree(d_buf));
    d_buf = nullptr;
    d_bytes = 0;
    F3D_HIP(hipMalloc(&d_buf, bytes));
    d_bytes = bytes;
  }
  u64* d_foreign = static_cast<u64*>(d_buf);
  int* d_map = reinterpret_cast<int*>(d_foreign + 1);
  F3D_HIP(hipMemsetAsync(d_foreign, 0, sizeof(u64), f3d::stream()));
  F3D_HIP(hipMemcpyAsync(d_map, map, n * sizeof(int), hipMemcpyHostToDevice, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));  // the caller's map may go once the call returns
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, g.D);
  hipLaunchKernelGGL(k_relabel_labels, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), f3d_ptr<const int>(labels), static_cast<int>(n),
                     d_map, f3d_ptr<int>(out), g, d_foreign);
  F3D_HIP(hipGetLastError());
  if (foreign) {
    u64 count = 0;
    F3D_HIP(hipMemcpyAsync(&count, d_foreign, sizeof(count), hipMemcpyDeviceToHost, f3d::stream()));
    F3D_HIP(hipStreamSynchronize(f3d::stream()));
    *foreign = count;
  }
  return 0;
}

}  // extern "C"
