// Statistics of a scalar field per labelled body for gfx950 (f3d_label_field_sums), and the painting of a per-label value back into
// a volume (f3d_paint_labels).  The classes, the quantisation, the row and the bins are those of include/f3d.h; the bin rule and the
// ordered key of a float are f3d_histogram_bin.h's; tests/label_field_ref.py restates them in numpy and every word, count and counter
// matches bit for bit.  The solve from the rows to mean, deviation and quantiles is host code (host/label_field.cpp).
//
// Every sum is an exact integer of the quantised value q = (int)rintf(s * 2^shift), the extremes are maxima over the ordered integer
// key of the raw bits, the counts are integers: integer atomics give the same bytes whatever the schedule.  No float atomic.  No lane
// ever waits for another lane or workgroup: every loop has a compile-time bound, a claimed slot's words start at zero and the adds
// and maxima to them commute, so a claim and the updates of other lanes need no ordering.
//
// Shape: k_label_shape_sums' (f3d_label_shape.hip) without the neighbour planes.  A wave on 64 consecutive x of one row, a workgroup
// kBY rows, a lane marching over the kZ planes of its own column, kAhead planes at a time whose two loads each (label, field) are
// issued together.  A lane accumulates in registers while the label of its column stays the same -- n, sum q, the two key maxima,
// below and above in 32 bits (|sum q| <= 32 * 2^24), sum q^2 in 64 -- and voxels that do not take part do not end a run.  It closes
// the run into the workgroup's LDS table keyed on the label: kSlots slots claimed by atomicCAS within kProbes steps, two words of 64
// bits (sum q, |.| <= 2^37 over the 2^13 voxels of a tile; sum q^2 < 2^61) and five of 32.  A run that finds no slot goes straight to
// the label's global row (slow, correct).  At the end of a tile every occupied slot is flushed, eight lanes one word each; sum q^2 is
// split into its two limbs there.
// Global row of a label, 8 words of 64 bits:  [0] n  [1] max(0xffffffff - key)  [2] max(key)  [3] sum q (two's complement)
//   [4] [5] sum q^2: the low 32 bits of every addend, and the rest  [6] below  [7] above.  Then the five counters of
// f3d_label_field_info, then the 32-bit counts, n_labels rows of `bins`.
//
// The histogram (HIST, a template parameter: bins == 0 pays nothing).  A lane merges its run of equal (label, bin) along z and closes
// it into a second LDS table keyed on (label << 8) | bin, kHSlots slots of one 32-bit count, in front of the 32-bit global adds; a run
// without a slot is added to the global count directly.  DESIGN.md §27 has what was measured of it.
#include <algorithm>
#include <cstring>
#include <vector>

#include "f3d_internal.h"
#include "f3d_partials.h"
#define F3D_HIST_FN __host__ __device__ __forceinline__
#include "f3d_histogram_bin.h"

namespace {

using namespace f3d_partials;
using f3d_hist::Rule;

constexpr int kBX = 64;
constexpr int kBY = 4;
constexpr int kZ = 32;
constexpr int kAhead = 4;  // planes whose loads are in flight together; divides kZ
constexpr int kSlots = 128;  // a power of two
constexpr int kSlotBits = 7;
constexpr int kProbes = 16;
constexpr int kHSlots = 1024;  // a power of two
constexpr int kHSlotBits = 10;
constexpr int kRowWords = 8;
constexpr int kNarrow = 5;     // n, low key, high key, below, above
constexpr int kInfoWords = 5;  // background, foreign, nan, out_of_range, used
constexpr int kMaxFieldBins = 256;
constexpr size_t kMaxLabels = static_cast<size_t>(1) << 22;
constexpr size_t kMaxCounts = static_cast<size_t>(1) << 26;
constexpr unsigned kQuietNan = 0x7fc00000u;
// The other route of the histogram, for timing alone (tools/label_field_bench.py): built with -DF3D_LABEL_FIELD_DIRECT every merged
// run of equal (label, bin) is added to its global count and the second LDS table stays empty.  The counts are the same bytes.
#ifdef F3D_LABEL_FIELD_DIRECT
constexpr bool kHistDirect = true;
#else
constexpr bool kHistDirect = false;
#endif

typedef unsigned long long u64;

// what a lane has gathered of one label since it last changed
struct Run {
  int n, sq, below, above;
  unsigned low, high;  // max(0xffffffff - key), max(key)
  u64 sqq;
  __device__ __forceinline__ void clear()
  {
    n = sq = below = above = 0;
    low = high = 0;
    sqq = 0;
  }
};

// the slot of `key` (never 0) in a table of 2^bits slots, claimed if need be; -1 when none is free within kProbes steps
template <int BITS>
__device__ __forceinline__ int find_slot(unsigned key, unsigned* keys)
{
  unsigned at = (key * 2654435761u) >> (32 - BITS);
  for (int probe = 0; probe < kProbes; ++probe) {
    // 0 is a free slot.  A key never changes once set and most runs meet their own
    unsigned seen = __atomic_load_n(&keys[at], __ATOMIC_RELAXED);
    if (seen == 0) seen = atomicCAS(&keys[at], 0u, key);
    if (seen == 0 || seen == key) return static_cast<int>(at);
    at = (at + 1) & ((1u << BITS) - 1);
  }
  return -1;
}

__device__ __forceinline__ void close_run(const Run& s, int label, unsigned* keys, u64* wide, unsigned* narrow, u64* table)
{
  const u64 sq = static_cast<u64>(static_cast<long long>(s.sq));  // sign-extended: the adds are modulo 2^64
  const int slot = find_slot<kSlotBits>(static_cast<unsigned>(label), keys);
  if (slot < 0) {
    u64* row = table + static_cast<size_t>(label - 1) * kRowWords;
    atomicAdd(row + 0, static_cast<u64>(s.n));
    atomicMax(row + 1, static_cast<u64>(s.low));
    atomicMax(row + 2, static_cast<u64>(s.high));
    if (sq) atomicAdd(row + 3, sq);
    if (s.sqq) {
      atomicAdd(row + 4, s.sqq & 0xffffffffull);
      atomicAdd(row + 5, s.sqq >> 32);
    }
    if (s.below) atomicAdd(row + 6, static_cast<u64>(s.below));
    if (s.above) atomicAdd(row + 7, static_cast<u64>(s.above));
    return;
  }
  if (sq) atomicAdd(wide + slot * 2 + 0, sq);
  if (s.sqq) atomicAdd(wide + slot * 2 + 1, s.sqq);
  unsigned* at = narrow + slot * kNarrow;
  atomicAdd(at + 0, static_cast<unsigned>(s.n));
  atomicMax(at + 1, s.low);
  atomicMax(at + 2, s.high);
  if (s.below) atomicAdd(at + 3, static_cast<unsigned>(s.below));
  if (s.above) atomicAdd(at + 4, static_cast<unsigned>(s.above));
}

// `length` voxels of (label, bin): into the workgroup's second table, or straight to the count
__device__ __forceinline__ void close_bin_run(int label, int bin, int length, int bins, unsigned* hkeys, unsigned* hcounts,
                                              unsigned* counts)
{
  const unsigned key = (static_cast<unsigned>(label) << 8) | static_cast<unsigned>(bin);
  const int slot = kHistDirect ? -1 : find_slot<kHSlotBits>(key, hkeys);
  if (slot < 0)
    atomicAdd(counts + static_cast<size_t>(label - 1) * bins + bin, static_cast<unsigned>(length));
  else
    atomicAdd(hcounts + slot, static_cast<unsigned>(length));
}

// include/f3d.h, f3d_label_field_sums.  table: n_labels rows of kRowWords, then the kInfoWords counters; counts: n_labels rows of
// rule.bins 32-bit words (HIST only).
template <bool HIST>
__global__ __launch_bounds__(kBX* kBY) void k_label_field_sums(const float* __restrict__ field, const int* __restrict__ labels,
                                                               int n_labels, float scale, Rule rule, F3dGeo g, u64* __restrict__ table,
                                                               unsigned* __restrict__ counts)
{
  __shared__ u64 wide[kSlots * 2];
  __shared__ unsigned narrow[kSlots * kNarrow];
  __shared__ unsigned keys[kSlots];
  __shared__ unsigned hkeys[HIST ? kHSlots : 1];
  __shared__ unsigned hcounts[HIST ? kHSlots : 1];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  for (int i = tid; i < kSlots * 2; i += kBX * kBY) wide[i] = 0;
  for (int i = tid; i < kSlots * kNarrow; i += kBX * kBY) narrow[i] = 0;
  for (int i = tid; i < kSlots; i += kBX * kBY) keys[i] = 0;
  if (HIST)
    for (int i = tid; i < kHSlots; i += kBX * kBY) hkeys[i] = hcounts[i] = 0;
  __syncthreads();

  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const bool col = y < g.H && x < g.W;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);

  Run run;
  run.clear();
  int current = 0;                         // the label of the open run, 0: none
  int bin_label = 0, bin_at = 0, bin_n = 0;  // the open run of equal (label, bin), bin_n == 0: none
  int background = 0, foreign = 0, nan = 0, out_of_range = 0, used = 0;

  if (col) {
#pragma unroll 1
    for (int z = z_begin; z < z_end; z += kAhead) {
      int l[kAhead];
      float s[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        l[k] = 0;
        s[k] = 0.f;
        if (z + k < z_end) {  // nothing but voxels of the box is loaded
          const size_t i = f3d_row(g, y, z + k) + static_cast<size_t>(x);
          l[k] = labels[i];
          s[k] = field[i];
        }
      }
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        if (z + k >= z_end) continue;
        const int a = l[k];
        const float v = s[k];
        if (a == 0) {
          ++background;
          continue;
        }
        if (a < 0 || a > n_labels) {
          ++foreign;
          continue;
        }
        if (v != v) {
          ++nan;
          continue;
        }
        const float t = v * scale;  // one float32 product
        if (!(fabsf(t) <= 16777216.0f)) {
          ++out_of_range;
          continue;
        }
        ++used;
        const int q = static_cast<int>(rintf(t));  // to nearest, ties to even: |q| <= 2^24
        if (a != current) {
          if (current != 0) close_run(run, current, keys, wide, narrow, table);
          run.clear();
          current = a;
        }
        const unsigned key = f3d_hist::key_of_bits(__float_as_uint(v));
        ++run.n;
        run.sq += q;
        run.sqq += static_cast<u64>(static_cast<long long>(q) * static_cast<long long>(q));
        run.low = max(run.low, 0xffffffffu - key);
        run.high = max(run.high, key);
        if (HIST) {
          if (v < rule.lo) {
            ++run.below;
          } else if (v > rule.hi) {
            ++run.above;
          } else {
            const int bin = f3d_hist::bin_of(rule, v);
            if (bin_n != 0 && (a != bin_label || bin != bin_at)) {
              close_bin_run(bin_label, bin_at, bin_n, rule.bins, hkeys, hcounts, counts);
              bin_n = 0;
            }
            bin_label = a;
            bin_at = bin;
            ++bin_n;
          }
        }
      }
    }
    if (current != 0) close_run(run, current, keys, wide, narrow, table);
    if (HIST && bin_n != 0) close_bin_run(bin_label, bin_at, bin_n, rule.bins, hkeys, hcounts, counts);
  }

  // the counters: one add per wave and counter
  const u64 tally[kInfoWords] = {wave_sum(static_cast<u64>(background)), wave_sum(static_cast<u64>(foreign)),
                                 wave_sum(static_cast<u64>(nan)), wave_sum(static_cast<u64>(out_of_range)),
                                 wave_sum(static_cast<u64>(used))};
  if (threadIdx.x == 0) {
    u64* info = table + static_cast<size_t>(n_labels) * kRowWords;
    for (int i = 0; i < kInfoWords; ++i)
      if (tally[i]) atomicAdd(info + i, tally[i]);
  }

  // every occupied slot to its label's row: eight lanes of a wave, one word each, consecutive addresses
  __syncthreads();
  for (int slot = threadIdx.y * (kBX / kRowWords) + threadIdx.x / kRowWords; slot < kSlots; slot += kBY * (kBX / kRowWords)) {
    const unsigned key = keys[slot];
    if (key == 0) continue;
    const int word = threadIdx.x % kRowWords;
    const unsigned* nar = narrow + slot * kNarrow;
    const u64 sqq = wide[slot * 2 + 1];
    u64* at = table + static_cast<size_t>(key - 1) * kRowWords + word;
    switch (word) {
      case 0: atomicAdd(at, static_cast<u64>(nar[0])); break;
      case 1: atomicMax(at, static_cast<u64>(nar[1])); break;
      case 2: atomicMax(at, static_cast<u64>(nar[2])); break;
      case 3: if (wide[slot * 2]) atomicAdd(at, wide[slot * 2]); break;
      case 4: if (sqq & 0xffffffffull) atomicAdd(at, sqq & 0xffffffffull); break;
      case 5: if (sqq >> 32) atomicAdd(at, sqq >> 32); break;
      case 6: if (nar[3]) atomicAdd(at, static_cast<u64>(nar[3])); break;
      default: if (nar[4]) atomicAdd(at, static_cast<u64>(nar[4])); break;
    }
  }
  if (HIST)
    for (int slot = tid; slot < kHSlots; slot += kBX * kBY) {
      const unsigned key = hkeys[slot];
      if (key == 0) continue;
      atomicAdd(counts + static_cast<size_t>((key >> 8) - 1) * rule.bins + (key & 0xffu), hcounts[slot]);
    }
}

// include/f3d.h, f3d_paint_labels: each voxel reads and writes its own word, so out may be labels.  The values travel as their bits.
__global__ __launch_bounds__(kBX* kBY) void k_paint_labels(const int* labels, int n, const unsigned* __restrict__ values, unsigned* out,
                                                           F3dGeo g)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z = blockIdx.z;
  if (x < g.W && y < g.H) {
    const size_t i = f3d_row(g, y, z) + x;
    const int l = labels[i];
    out[i] = (l >= 1 && l <= n) ? values[l - 1] : kQuietNan;
  }
}

// a device buffer of at least `bytes` of the calling thread's (grow-only); each entry has its own
int grow(void** d_buf, size_t* d_bytes, size_t bytes)
{
  if (*d_bytes < bytes) {
    if (*d_buf) F3D_HIP(hipFree(*d_buf));
    *d_buf = nullptr;
    *d_bytes = 0;
    F3D_HIP(hipMalloc(d_buf, bytes));
    *d_bytes = bytes;
  }
  return 0;
}

int box_of(const char* who, size_t width, size_t height, size_t depth, F3dGeo* g)
{
  if (width == 0 || height == 0 || depth == 0) return f3d::fail("%s: empty box %zux%zux%zu", who, width, height, depth);
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > 0x7fffffffull)
    return f3d::fail("%s: box %zux%zux%zu exceeds 32768 along an axis or 2^31 - 1 voxels", who, width, height, depth);
  if (!f3d::make_geo(g, width, height, depth, nullptr, who)) return 1;
  return 0;
}

}  // namespace

extern "C" {

int f3d_label_field_sums(f3d_devptr field, f3d_devptr labels, size_t n_labels, int shift, float lo, float hi, size_t bins, size_t width,
                         size_t height, size_t depth, struct f3d_label_field_sums* out, unsigned* counts, f3d_label_field_info* info)
{
  const char* who = "f3d_label_field_sums";
  F3D_REQUIRE_READY(who);
  if (!field) return f3d::fail("%s: null field", who);
  if (!labels) return f3d::fail("%s: null labels", who);
  if (!out) return f3d::fail("%s: null out", who);
  if (field == labels) return f3d::fail("%s: field and labels are one container", who);
  if (shift < -100 || shift > 100) return f3d::fail("%s: shift %d is outside -100 .. 100", who, shift);
  if (bins > kMaxFieldBins) return f3d::fail("%s: bins %zu is outside 0 .. %d", who, bins, kMaxFieldBins);
  if (bins == 0 && counts) return f3d::fail("%s: counts given with bins == 0", who);
  if (bins != 0 && !counts) return f3d::fail("%s: null counts with bins %zu", who, bins);
  Rule rule = {0.f, 0.f, 0.f, 0};
  if (bins != 0)
    if (const char* why = f3d_hist::make_rule(lo, hi, static_cast<long long>(bins), &rule))
      return f3d::fail("%s: %s (lo %.9g, hi %.9g, bins %zu)", who, why, static_cast<double>(lo), static_cast<double>(hi), bins);
  if (n_labels == 0 || n_labels > kMaxLabels) return f3d::fail("%s: n_labels %zu is outside 1 .. %zu", who, n_labels, kMaxLabels);
  if (n_labels * bins > kMaxCounts) return f3d::fail("%s: n_labels * bins = %zu exceeds 2^26 counts", who, n_labels * bins);
  F3dGeo g;
  if (box_of(who, width, height, depth, &g)) return 1;

  // the rows, the counters, then the counts
  static thread_local void* d_buf = nullptr;
  static thread_local size_t d_bytes = 0;
  const size_t words = n_labels * kRowWords + kInfoWords, n_counts = n_labels * bins;
  const size_t bytes = words * sizeof(u64) + n_counts * sizeof(unsigned);
  if (grow(&d_buf, &d_bytes, bytes)) return 1;
  u64* d_table = static_cast<u64*>(d_buf);
  unsigned* d_counts = reinterpret_cast<unsigned*>(d_table + words);
  hipStream_t stream = f3d::stream();
  F3D_HIP(hipMemsetAsync(d_buf, 0, bytes, stream));
  const float scale = ldexpf(1.0f, shift);
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ), block(kBX, kBY, 1);
  if (bins != 0)
    hipLaunchKernelGGL(k_label_field_sums<true>, grid, block, 0, stream, f3d_ptr<const float>(field), f3d_ptr<const int>(labels),
                       static_cast<int>(n_labels), scale, rule, g, d_table, d_counts);
  else
    hipLaunchKernelGGL(k_label_field_sums<false>, grid, block, 0, stream, f3d_ptr<const float>(field), f3d_ptr<const int>(labels),
                       static_cast<int>(n_labels), scale, rule, g, d_table, d_counts);
  F3D_HIP(hipGetLastError());
  // everything comes down in one copy into memory of this call's; nothing of the caller's is written before the wait passed
  std::vector<u64> host((bytes + sizeof(u64) - 1) / sizeof(u64));
  F3D_HIP(hipMemcpyAsync(host.data(), d_buf, bytes, hipMemcpyDeviceToHost, stream));
  F3D_HIP(hipStreamSynchronize(stream));
  for (size_t l = 0; l < n_labels; ++l) {
    const u64* r = host.data() + l * kRowWords;
    struct f3d_label_field_sums& s = out[l];
    s.n = r[0];
    s.min_key = 0xffffffffull - r[1];
    s.max_key = r[2];
    s.iq = static_cast<long long>(r[3]);
    s.iqq_lo = r[4] & 0xffffffffull;  // the carry: which voxels shared an addend depends on the schedule, the sum does not
    s.iqq_hi = r[5] + (r[4] >> 32);
    s.below = r[6];
    s.above = r[7];
  }
  if (n_counts) std::memcpy(counts, host.data() + words, n_counts * sizeof(unsigned));
  if (info) {
    const u64* c = host.data() + n_labels * kRowWords;
    info->background = c[0];
    info->foreign = c[1];
    info->nan = c[2];
    info->out_of_range = c[3];
    info->used = c[4];
  }
  return 0;
}

int f3d_paint_labels(f3d_devptr labels, size_t n_labels, const float* values, f3d_devptr out, size_t width, size_t height, size_t depth)
{
  const char* who = "f3d_paint_labels";
  F3D_REQUIRE_READY(who);
  if (!labels) return f3d::fail("%s: null labels", who);
  if (!values) return f3d::fail("%s: null values", who);
  if (!out) return f3d::fail("%s: null out", who);
  if (n_labels == 0 || n_labels > kMaxLabels) return f3d::fail("%s: n_labels %zu is outside 1 .. %zu", who, n_labels, kMaxLabels);
  F3dGeo g;
  if (box_of(who, width, height, depth, &g)) return 1;

  // a buffer of its own, so that the rows of f3d_label_field_sums on the stream are not disturbed
  static thread_local void* d_buf = nullptr;
  static thread_local size_t d_bytes = 0;
  if (grow(&d_buf, &d_bytes, n_labels * sizeof(float))) return 1;
  F3D_HIP(hipMemcpyAsync(d_buf, values, n_labels * sizeof(float), hipMemcpyHostToDevice, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));  // the caller's values may go once the call returns
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, g.D);
  hipLaunchKernelGGL(k_paint_labels, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), f3d_ptr<const int>(labels), static_cast<int>(n_labels),
                     static_cast<const unsigned*>(d_buf), f3d_ptr<unsigned>(out), g);
  F3D_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
