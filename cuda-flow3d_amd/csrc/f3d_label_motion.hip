// Per-label motion of a displacement for gfx950: the moment sums of every label of a segmentation in one pass
// (f3d_label_motion_sums) and the subtraction of one fit per label (f3d_remove_label_motion).  The definitions, the presence rule, the
// quantisation and the evaluation order are those of include/f3d.h; the solve between the two is host code (host/motion_fit.cpp,
// f3d_motion_solve_labels).  tests/label_motion_ref.py restates both in numpy: sums and residuals match bit for bit.
//
// The sums are exact integers (q = rint(d * 2^14), doubled coordinates), so no summation order has to be fixed: integer atomics give
// the same bytes whatever the schedule.  No float atomic, no float instruction on a label.
//
// Shape: k_motion_sums' (f3d_motion.hip).  A wave on 64 consecutive x of one row, a workgroup kBY rows, a lane marching over kZ planes
// of its own column with the next plane's loads issued ahead; loads are full 256-B rows of u, v, w, labels and optionally the weight.
//
// Widths (limits of the entry: at most 32768 along an axis, |q| <= 2^24, |x2| < 2^16, a tile of 64 x 4 x 32 = 2^13 voxels):
//   a lane's run (32 voxels):   sum q < 2^29 (int), sum z2 < 2^21 (int), sum z2^2 < 2^37, sum z2 q < 2^45, sum q^2 < 2^53 (64 bits)
//   a tile (2^13 voxels):       sum q^2 < 2^61, sum |x2 q| < 2^53, coordinate sums < 2^45: every LDS word is a signed 64-bit integer
//   a label (up to 2^33 voxels): Idd reaches 2^81, so the fifteen displacement sums cross tiles as two signed 64-bit limbs: a value v
//   adds v & 0xffffffff to lo and v >> 32 (arithmetic) to hi; v == hi * 2^32 + lo holds for either sign.  lo only receives addends
//   in [0, 2^32) and the host reads it as unsigned: two segments of one label in a lane's run have another label's voxel between
//   them, so a label has at most 2^32 segments and lo stays below 2^64 even when every one of them goes straight to the global row.
//   The ten coordinate sums stay single words as in f3d_motion_sums.
// Global accumulator row of a label, 40 words = 320 B:  [0] n  [1..3] sum x2  [4..9] sum x2 x2 (xx yy zz xy xz yz)
//   [10..24] lo of Id[3], Ixd[9], Idd[3]   [25..39] hi of the same.
//
// LDS table: kSlots slots of 25 words (the tile's sums are single words; the limbs are split when a slot is flushed) and one key
// each, addressed openly on the label: claims by atomicCAS on the key, adds by 64-bit integer LDS atomics.  kSlots = 128: 25.5 KiB
// per workgroup, six workgroups (six waves per SIMD) of the CU's 160 KiB, which is what the 20 B per voxel of loads in flight need;
// a tile of a segmentation whose bodies are tens of voxels across meets a handful of labels, and 128 leaves the probe sequences
// short.  A lane that finds no slot within kProbes steps adds its run-segment straight to the global row (slow, correct).
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
constexpr int kSlotWords = 25;
constexpr int kRowWords = 40;
constexpr int kInfoWords = 5;
constexpr size_t kMaxLabels = static_cast<size_t>(1) << 22;

typedef unsigned long long u64;

// what a lane has gathered of one label since it last changed: the column's x2 and y2 are multiplied in when it is closed
struct Segment {
  int n, sz2, q[3];
  long long szz4, zq[3], qq[3];
  __device__ __forceinline__ void clear()
  {
    n = sz2 = 0;
    szz4 = 0;
    for (int j = 0; j < 3; ++j) q[j] = 0, zq[j] = 0, qq[j] = 0;
  }
};

// the 25 sums of a closed segment in the order of a slot (and of the first 25 meanings of a global row)
__device__ __forceinline__ void segment_words(const Segment& s, long long x2, long long y2, long long out[kSlotWords])
{
  const long long n = s.n, sz2 = s.sz2;
  out[0] = n;
  out[1] = x2 * n;
  out[2] = y2 * n;
  out[3] = sz2;
  out[4] = x2 * x2 * n;
  out[5] = y2 * y2 * n;
  out[6] = s.szz4;
  out[7] = x2 * y2 * n;
  out[8] = x2 * sz2;
  out[9] = y2 * sz2;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    out[10 + j] = s.q[j];
    out[13 + j] = x2 * s.q[j];
    out[16 + j] = y2 * s.q[j];
    out[19 + j] = s.zq[j];
    out[22 + j] = s.qq[j];
  }
}

__device__ __forceinline__ void add_word(u64* p, long long v)
{
  if (v != 0) atomicAdd(p, static_cast<u64>(v));  // two's complement: the wrapped sum is the signed one
}

// a word of a slot into its place(s) of a global row
__device__ __forceinline__ void add_to_row(u64* row, int word, long long v)
{
  if (word < 10) {
    add_word(row + word, v);
  } else {
    add_word(row + word, v & 0xffffffffll);
    add_word(row + word + 15, v >> 32);
  }
}

// the slot of `label` in the workgroup's table, claimed if need be; -1 when none is free within kProbes steps
__device__ __forceinline__ int find_slot(int label, int* keys)
{
  unsigned at = (static_cast<unsigned>(label) * 2654435761u) >> (32 - kSlotBits);
  for (int probe = 0; probe < kProbes; ++probe) {
    const int seen = atomicCAS(&keys[at], 0, label);  // labels here are 1 .. n_labels: 0 is a free slot
    if (seen == 0 || seen == label) return static_cast<int>(at);
    at = (at + 1) & (kSlots - 1);
  }
  return -1;
}

// one of the 25 sums of a closed segment into the slot, or straight to the label's global row when there is none (slow, correct)
__device__ __forceinline__ void add_sum(int slot, int label, int word, long long v, u64* slots, u64* table)
{
  if (slot >= 0)
    add_word(slots + slot * kSlotWords + word, v);
  else
    add_to_row(table + static_cast<size_t>(label - 1) * kRowWords, word, v);
}

__device__ __forceinline__ void close_segment(const Segment& s, int label, long long x2, long long y2, int* keys, u64* slots, u64* table)
{
  long long words[kSlotWords];
  segment_words(s, x2, y2, words);
  const int slot = find_slot(label, keys);
#pragma unroll
  for (int i = 0; i < kSlotWords; ++i) add_sum(slot, label, i, words[i], slots, table);
}

// include/f3d.h, f3d_label_motion_sums.  table: n_labels rows of kRowWords, then the kInfoWords counters of f3d_label_info.
template <bool WEIGHT>
__global__ __launch_bounds__(kBX* kBY) void k_label_motion_sums(const float* __restrict__ du, const float* __restrict__ dv,
                                                                const float* __restrict__ dw, const int* __restrict__ labels,
                                                                int n_labels, const float* __restrict__ weight, float weight_min,
                                                                F3dGeo g, u64* __restrict__ table)
{
  __shared__ u64 slots[kSlots * kSlotWords];
  __shared__ int keys[kSlots];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  for (int i = tid; i < kSlots * kSlotWords; i += kBX * kBY) slots[i] = 0;
  for (int i = tid; i < kSlots; i += kBX * kBY) keys[i] = 0;
  __syncthreads();

  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const bool col = x < g.W && y < g.H;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const long long x2 = 2 * x - (g.W - 1), y2 = 2 * y - (g.H - 1);
  const float nan = __builtin_nanf("");

  Segment seg;
  seg.clear();
  int current = 0;  // the label of the open segment, 0: none
  int background = 0, foreign = 0, absent = 0, out_of_range = 0, used = 0;

  // the plane one step ahead; a lane without a column runs an empty loop
  float u = nan, v = nan, w = nan, m = 0.f;
  int label = 0;
  if (col) {
    const size_t i = f3d_row(g, y, z_begin) + x;
    u = du[i];
    v = dv[i];
    w = dw[i];
    label = labels[i];
    if (WEIGHT) m = weight[i];
  }
  for (int z = z_begin; col && z < z_end; ++z) {
    float nu = nan, nv = nan, nw = nan, nm = 0.f;
    int nlabel = 0;
    if (z + 1 < z_end) {
      const size_t i = f3d_row(g, y, z + 1) + x;
      nu = du[i];
      nv = dv[i];
      nw = dw[i];
      nlabel = labels[i];
      if (WEIGHT) nm = weight[i];
    }
    bool present = !(isnan(u) || isnan(v) || isnan(w));
    if (WEIGHT) present = present && m >= weight_min;  // a NaN weight fails the comparison
    const bool ranged = fabsf(u) < 1024.f && fabsf(v) < 1024.f && fabsf(w) < 1024.f;  // false for an infinity
    if (label == 0) {
      ++background;
    } else if (label < 0 || label > n_labels) {
      ++foreign;
    } else if (!present) {
      ++absent;
    } else if (!ranged) {
      ++out_of_range;
    } else {
      ++used;
      if (label != current) {
        if (current != 0) close_segment(seg, current, x2, y2, keys, slots, table);
        seg.clear();
        current = label;
      }
      const int z2 = 2 * z - (g.D - 1);
      const int q[3] = {static_cast<int>(rintf(u * 16384.0f)), static_cast<int>(rintf(v * 16384.0f)),
                        static_cast<int>(rintf(w * 16384.0f))};  // the product is exact, the rounding to nearest even
      ++seg.n;
      seg.sz2 += z2;
      seg.szz4 += static_cast<long long>(z2) * z2;
      for (int j = 0; j < 3; ++j) {
        seg.q[j] += q[j];
        seg.zq[j] += static_cast<long long>(z2) * q[j];
        seg.qq[j] += static_cast<long long>(q[j]) * q[j];
      }
    }
    u = nu;
    v = nv;
    w = nw;
    m = nm;
    label = nlabel;
  }
  if (current != 0) close_segment(seg, current, x2, y2, keys, slots, table);

  // the counters: one add per wave and counter
  const u64 counts[kInfoWords] = {wave_sum(static_cast<u64>(background)), wave_sum(static_cast<u64>(foreign)),
                                  wave_sum(static_cast<u64>(absent)), wave_sum(static_cast<u64>(out_of_range)),
                                  wave_sum(static_cast<u64>(used))};
  if (threadIdx.x == 0) {
    u64* info = table + static_cast<size_t>(n_labels) * kRowWords;
    for (int i = 0; i < kInfoWords; ++i)
      if (counts[i]) atomicAdd(info + i, counts[i]);
  }

  // every occupied slot to its label's row: 40 lanes of a wave, one word each, consecutive addresses
  __syncthreads();
  for (int slot = threadIdx.y; slot < kSlots; slot += kBY) {
    const int key = keys[slot];
    if (key == 0 || threadIdx.x >= kRowWords) continue;
    const int word = threadIdx.x;
    const long long value = static_cast<long long>(slots[slot * kSlotWords + (word < kSlotWords ? word : word - 15)]);
    const long long part = word < 10 ? value : (word < kSlotWords ? (value & 0xffffffffll) : (value >> 32));
    add_word(table + static_cast<size_t>(key - 1) * kRowWords + word, part);
  }
}

struct ResidualPartial {
  unsigned long long present;
  double sum_sq;
  float max_abs, pad;

  static __device__ __forceinline__ ResidualPartial identity() { return {0ull, 0.0, -INFINITY, 0.f}; }
  __device__ __forceinline__ void merge(const ResidualPartial& q)
  {
    present += q.present;
    sum_sq += q.sum_sq;
    max_abs = fmaxf(max_abs, q.max_abs);
  }
};

// a row of the table f3d_remove_label_motion uploads: ok is 0 for a label whose status is not F3D_LABEL_OK
struct LabelFitRow {
  double centre[3], t[3], M[9], ok;
};

// include/f3d.h, f3d_remove_label_motion.  out_* may be the inputs themselves (a lane reads its voxel before it writes it), so nothing
// here is __restrict__.  A lane keeps the row of its last label: along a column inside a body the gather happens once.
template <bool STATS>
__global__ __launch_bounds__(kBX* kBY) void k_remove_label_motion(const float* du, const float* dv, const float* dw, const int* labels,
                                                                  int n_labels, const LabelFitRow* rows, float* out_u, float* out_v,
                                                                  float* out_w, F3dGeo g, ResidualPartial* partials)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const bool col = x < g.W && y < g.H;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const float nan = __builtin_nanf("");

  ResidualPartial sum = ResidualPartial::identity();
  LabelFitRow fit;
  int held = 0;  // the label whose row `fit` is, 0: none
  float u = nan, v = nan, w = nan;
  int label = 0;
  if (col) {
    const size_t i = f3d_row(g, y, z_begin) + x;
    u = du[i];
    v = dv[i];
    w = dw[i];
    label = labels[i];
  }
  for (int z = z_begin; col && z < z_end; ++z) {
    float nu = nan, nv = nan, nw = nan;
    int nlabel = 0;
    if (z + 1 < z_end) {
      const size_t i = f3d_row(g, y, z + 1) + x;
      nu = du[i];
      nv = dv[i];
      nw = dw[i];
      nlabel = labels[i];
    }
    float ru = nan, rv = nan, rw = nan;
    if (label >= 1 && label <= n_labels) {
      if (label != held) {
        fit = rows[label - 1];
        held = label;
      }
      if (fit.ok != 0.0) {
        const double X = static_cast<double>(x) - fit.centre[0], Y = static_cast<double>(y) - fit.centre[1];
        const double Z = static_cast<double>(z) - fit.centre[2];
        ru = static_cast<float>(static_cast<double>(u) - (fit.t[0] + ((fit.M[0] * X + fit.M[1] * Y) + fit.M[2] * Z)));
        rv = static_cast<float>(static_cast<double>(v) - (fit.t[1] + ((fit.M[3] * X + fit.M[4] * Y) + fit.M[5] * Z)));
        rw = static_cast<float>(static_cast<double>(w) - (fit.t[2] + ((fit.M[6] * X + fit.M[7] * Y) + fit.M[8] * Z)));
      }
    }
    const size_t i = f3d_row(g, y, z) + x;
    out_u[i] = ru;
    out_v[i] = rv;
    out_w[i] = rw;
    if (STATS && !(isnan(ru) || isnan(rv) || isnan(rw))) {
      ++sum.present;
      sum.sum_sq += static_cast<double>(ru) * static_cast<double>(ru);
      sum.sum_sq += static_cast<double>(rv) * static_cast<double>(rv);
      sum.sum_sq += static_cast<double>(rw) * static_cast<double>(rw);
      sum.max_abs = fmaxf(sum.max_abs, fmaxf(fmaxf(fabsf(ru), fabsf(rv)), fabsf(rw)));
    }
    u = nu;
    v = nv;
    w = nw;
    label = nlabel;
  }

  if (STATS) {
    sum.present = wave_sum(sum.present);
    sum.sum_sq = wave_sum(sum.sum_sq);
    sum.max_abs = wave_max(sum.max_abs);
    block_partial<ResidualPartial, kBY>(sum, partials);
  }
}

dim3 label_grid(const F3dGeo& g) { return dim3((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, (g.D + kZ - 1) / kZ); }

// the calling thread's device buffer of at least `bytes` (grow-only; Tag keeps the two users apart)
template <int Tag>
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

// hi * 2^32 + lo (lo read as unsigned, see the widths above) rounded to binary64 once, to nearest even (the conversion of a 128-bit
// integer does that), then scaled: exact
double limbs_scaled(long long lo, long long hi, double scale)
{
  const __int128 total =
      static_cast<__int128>(hi) * (static_cast<__int128>(1) << 32) + static_cast<__int128>(static_cast<unsigned long long>(lo));
  return static_cast<double>(total) * scale;
}

}  // namespace

extern "C" {

int f3d_label_motion_sums(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr labels, size_t n_labels, f3d_devptr weight,
                          float weight_min, size_t width, size_t height, size_t depth, struct f3d_motion_sums* out,
                          f3d_label_info* info)
{
  F3D_REQUIRE_READY("f3d_label_motion_sums");
  if (!u || !v || !w) return f3d::fail("f3d_label_motion_sums: null input");
  if (!labels) return f3d::fail("f3d_label_motion_sums: null labels");
  if (!out) return f3d::fail("f3d_label_motion_sums: null out");
  if (n_labels == 0 || n_labels > kMaxLabels)
    return f3d::fail("f3d_label_motion_sums: n_labels %zu is outside 1 .. %zu", n_labels, kMaxLabels);
  if (weight && weight_min != weight_min) return f3d::fail("f3d_label_motion_sums: weight_min is NaN");
  if (width == 0 || height == 0 || depth == 0)
    return f3d::fail("f3d_label_motion_sums: empty volume %zux%zux%zu", width, height, depth);
  if (width > 32768 || height > 32768 || depth > 32768 || width * height * depth > (static_cast<size_t>(1) << 33))
    return f3d::fail("f3d_label_motion_sums: volume %zux%zux%zu exceeds 32768 along an axis or 2^33 voxels", width, height, depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_label_motion_sums")) return 1;
  const dim3 grid = label_grid(g);
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  const int* pl = f3d_ptr<const int>(labels);
  const float* pm = f3d_ptr<const float>(weight);
  const size_t words = n_labels * kRowWords + kInfoWords;
  void* d_table;
  if (device_buffer<0>(words * sizeof(u64), &d_table)) return 1;
  F3D_HIP(hipMemsetAsync(d_table, 0, words * sizeof(u64), f3d::stream()));
  const int n = static_cast<int>(n_labels);
  if (pm)
    hipLaunchKernelGGL(k_label_motion_sums<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, pl, n, pm, weight_min, g,
                       static_cast<u64*>(d_table));
  else
    hipLaunchKernelGGL(k_label_motion_sums<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, pl, n, pm, weight_min, g,
                       static_cast<u64*>(d_table));
  F3D_HIP(hipGetLastError());
  std::vector<long long> host(words);
  F3D_HIP(hipMemcpyAsync(host.data(), d_table, words * sizeof(u64), hipMemcpyDeviceToHost, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  for (size_t l = 0; l < n_labels; ++l) {
    const long long* r = host.data() + l * kRowWords;
    struct f3d_motion_sums& s = out[l];
    s.n = static_cast<unsigned long long>(r[0]);
    for (int i = 0; i < 3; ++i) s.Sx[i] = 0.5 * static_cast<double>(r[1 + i]);
    for (int i = 0; i < 6; ++i) s.Sxx[i] = 0.25 * static_cast<double>(r[4 + i]);
    for (int i = 0; i < 3; ++i) s.Sd[i] = limbs_scaled(r[10 + i], r[25 + i], 0x1p-14);
    for (int i = 0; i < 9; ++i) s.Sxd[i] = limbs_scaled(r[13 + i], r[28 + i], 0x1p-15);
    for (int i = 0; i < 3; ++i) s.Sdd[i] = limbs_scaled(r[22 + i], r[37 + i], 0x1p-28);
  }
  if (info) {
    const long long* c = host.data() + n_labels * kRowWords;
    info->background = static_cast<unsigned long long>(c[0]);
    info->foreign = static_cast<unsigned long long>(c[1]);
    info->absent = static_cast<unsigned long long>(c[2]);
    info->out_of_range = static_cast<unsigned long long>(c[3]);
    info->used = static_cast<unsigned long long>(c[4]);
  }
  return 0;
}

int f3d_remove_label_motion(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr labels, size_t n_labels, const f3d_motion_fit* fits,
                            const int* status, f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w, size_t width, size_t height,
                            size_t depth, f3d_motion_residual* stats)
{
  F3D_REQUIRE_READY("f3d_remove_label_motion");
  if (!u || !v || !w) return f3d::fail("f3d_remove_label_motion: null input");
  if (!labels) return f3d::fail("f3d_remove_label_motion: null labels");
  if (!out_u || !out_v || !out_w) return f3d::fail("f3d_remove_label_motion: null output");
  if (!fits || !status) return f3d::fail("f3d_remove_label_motion: null fits or status");
  if (n_labels == 0 || n_labels > kMaxLabels)
    return f3d::fail("f3d_remove_label_motion: n_labels %zu is outside 1 .. %zu", n_labels, kMaxLabels);
  const f3d_devptr in[3] = {u, v, w}, out[3] = {out_u, out_v, out_w};
  static const char* const names[3] = {"u", "v", "w"};
  for (int i = 0; i < 3; ++i) {
    if (out[i] == labels) return f3d::fail("f3d_remove_label_motion: out_%s is the label container", names[i]);
    if (in[i] == labels) return f3d::fail("f3d_remove_label_motion: %s is the label container", names[i]);
    for (int j = 0; j < 3; ++j) {
      if (i != j && out[i] == in[j])
        return f3d::fail("f3d_remove_label_motion: out_%s is the input %s (in place means out_%s == %s)", names[i], names[j], names[i],
                         names[i]);
      if (i < j && out[i] == out[j])
        return f3d::fail("f3d_remove_label_motion: out_%s and out_%s are the same container", names[i], names[j]);
      if (i < j && in[i] == in[j]) return f3d::fail("f3d_remove_label_motion: %s and %s are the same container", names[i], names[j]);
    }
  }
  std::vector<LabelFitRow> rows(n_labels);
  for (size_t l = 0; l < n_labels; ++l) {
    LabelFitRow& r = rows[l];
    const bool ok = status[l] == F3D_LABEL_OK;
    bool finite = true;
    for (int i = 0; i < 3; ++i) r.centre[i] = ok ? fits[l].centre[i] : 0.0;
    for (int i = 0; i < 3; ++i) r.t[i] = ok ? fits[l].t[i] : 0.0;
    for (int i = 0; i < 9; ++i) r.M[i] = ok ? fits[l].M[i] : 0.0;
    r.ok = ok ? 1.0 : 0.0;
    for (double e : r.centre) finite = finite && e - e == 0.0;  // false for an infinity and for a NaN
    for (double e : r.t) finite = finite && e - e == 0.0;
    for (double e : r.M) finite = finite && e - e == 0.0;
    if (!finite)
      return f3d::fail("f3d_remove_label_motion: the fit of label %zu has an entry of centre, t or M that is not finite", l + 1);
  }
  if (width == 0 || height == 0 || depth == 0)
    return f3d::fail("f3d_remove_label_motion: empty volume %zux%zux%zu", width, height, depth);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_remove_label_motion")) return 1;
  void* d_rows;
  if (device_buffer<1>(n_labels * sizeof(LabelFitRow), &d_rows)) return 1;
  // the table goes up per call; the wait lets the host copy go when this call returns
  F3D_HIP(hipMemcpyAsync(d_rows, rows.data(), n_labels * sizeof(LabelFitRow), hipMemcpyHostToDevice, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  const dim3 grid = label_grid(g);
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  const int* pl = f3d_ptr<const int>(labels);
  const LabelFitRow* pr = static_cast<const LabelFitRow*>(d_rows);
  float *qu = f3d_ptr<float>(out_u), *qv = f3d_ptr<float>(out_v), *qw = f3d_ptr<float>(out_w);
  const int n = static_cast<int>(n_labels);
  if (!stats) {
    hipLaunchKernelGGL(k_remove_label_motion<false>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, pl, n, pr, qu, qv, qw, g,
                       nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  ResidualPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](ResidualPartial* d_part) {
        hipLaunchKernelGGL(k_remove_label_motion<true>, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), pu, pv, pw, pl, n, pr, qu, qv, qw,
                           g, d_part);
      }))
    return 1;
  stats->present = r.present;
  stats->sum_sq = r.sum_sq;
  stats->max_abs = r.present ? r.max_abs : __builtin_nanf("");
  return 0;
}

}  // extern "C"
