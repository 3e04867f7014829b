// Coarse block matching for gfx950 (include/f3d_block_match.h): on a grid of nodes, the integer shift that maximises
// the zero-normalised cross-correlation of a (2W+1)^3 window of frame 0 against frame 1, and the expansion of node vectors to a
// dense field.  The guess a solve of a large motion starts from (f3d_initial_flow) comes from here.
//
// k_block_match: one workgroup of 256 lanes per node.  The window of a and the (2(W+r)+1)^3 region of b around the node's centre
// are quantised to 8-bit codes on the way into LDS (at most 17^2 rows of 20 B and 33^2 rows of 40 B: 5.8 + 43.6 KB, sized per call);
// voxels of the region outside the box are never read and hold 0, and no candidate that is evaluated reads them.  Lanes own candidate
// shifts, dx fastest.  A candidate walks the (2W+1)^2 rows of its window: the row of a is kAw aligned dwords (zero padded, the same
// address in every lane: a broadcast), the row of b starts at any byte, so kAw + 1 aligned dwords are read and v_alignbyte_b32 cuts
// the four codes out; three v_dot4_u32_u8 per dword give sab, sb and sbb in int32.  Everything but the score is an integer, the
// score is binary64 with every operation rounded on its own (contraction is off in this build), and (score, index) is a total
// order, so the tree over the 256 lanes gives the same bytes as any other shape.
//
// k_expand_nodes: shape of k_initial_flow (one voxel per lane, a wave64 on 64 consecutive x of one row), three stores per voxel.
#include "f3d_gather.h"

#define F3D_HIST_FN __host__ __device__ __forceinline__
#include "f3d_histogram_bin.h"

#include <climits>
#include <cstdlib>

#include "f3d_block_match.h"

namespace {

using f3d_gather::kBX;
using f3d_gather::kBY;

constexpr int kLanes = 256;
constexpr int kRecordWords = 32;
constexpr int kCentreLimit = 1 << 20;
static_assert(sizeof(f3d_block_match_record) == kRecordWords * sizeof(int), "a record is 32 int32");

struct MatchArgs {
  f3d_hist::Rule rule;
  f3d_block_match_grid grid;
  int side;       // 2W + 1
  int ex, ey, ez; // extent of the region of b: 2 (W + r) + 1
  int b_pitch;    // bytes per row of the region in LDS: a multiple of 4, at least ex + 4
  int a_bytes;    // of the window of a in LDS (side^2 rows of 4 kAw bytes)
  int b_bytes;    // of the region of b in LDS, with the 8 bytes behind the last row that the last candidate's last read reaches
};

__device__ __forceinline__ unsigned code_of(const f3d_hist::Rule& r, float s, bool* is_nan)
{
  *is_nan = s != s;
  if (s != s || s < r.lo) return 0u;
  if (s > r.hi) return static_cast<unsigned>(r.bins - 1);
  return static_cast<unsigned>(f3d_hist::bin_of(r, s));
}

struct Sums {
  int sb, sbb, sab;
};

// the three sums of the candidate whose window starts at byte (bx, by, bz) of the region
template <int kAw>
__device__ __forceinline__ Sums candidate_sums(const unsigned* a_lds, const unsigned* b_lds, const MatchArgs& m, int bx, int by, int bz)
{
  const unsigned tail = (1u << (8 * (m.side & 3))) - 1u;  // side is odd: 1 or 3 codes in the last dword
  const unsigned shift = static_cast<unsigned>(bx) & 3u;
  const int pitch_words = m.b_pitch >> 2;
  unsigned sb = 0, sbb = 0, sab = 0;
  for (int wz = 0; wz < m.side; ++wz) {
    const unsigned* a_row = a_lds + wz * m.side * kAw;
    const unsigned* b_row = b_lds + ((bz + wz) * m.ey + by) * pitch_words + (bx >> 2);
    for (int wy = 0; wy < m.side; ++wy, a_row += kAw, b_row += pitch_words) {
      unsigned lo = b_row[0];
#pragma unroll
      for (int k = 0; k < kAw; ++k) {
        const unsigned hi = b_row[k + 1];
        unsigned codes = __builtin_amdgcn_alignbyte(hi, lo, shift);
        if (k == kAw - 1) codes &= tail;
        sab = __builtin_amdgcn_udot4(a_row[k], codes, sab, false);
        sb = __builtin_amdgcn_udot4(codes, 0x01010101u, sb, false);
        sbb = __builtin_amdgcn_udot4(codes, codes, sbb, false);
        lo = hi;
      }
    }
  }
  return {static_cast<int>(sb), static_cast<int>(sbb), static_cast<int>(sab)};
}

__device__ __forceinline__ bool better(double s, int i, double t, int j) { return s > t || (s == t && i < j); }

// every store to `records` is a vector store by the lane that owns the words
template <int kAw>
__global__ __launch_bounds__(kLanes) void k_block_match(const float* __restrict__ a, const float* __restrict__ b, F3dGeo g, MatchArgs m,
                                                        const int* __restrict__ centre, int* __restrict__ records)
{
  extern __shared__ unsigned lds[];
  __shared__ double best_score[kLanes];
  __shared__ int best_index[kLanes];
  __shared__ int counters[8];  // sa, saa, nan, evaluated, outside, flat
  unsigned* a_lds = lds;
  unsigned* b_lds = lds + (m.a_bytes >> 2);
  unsigned char* a_codes = reinterpret_cast<unsigned char*>(a_lds);
  unsigned char* b_codes = reinterpret_cast<unsigned char*>(b_lds);
  const int tid = threadIdx.x;
  const int node = blockIdx.x;
  const f3d_block_match_grid& q = m.grid;
  const int W = q.window, side = m.side;
  const int px = q.ox + (node % q.nx) * q.step;
  const int py = q.oy + ((node / q.nx) % q.ny) * q.step;
  const int pz = q.oz + (node / (q.nx * q.ny)) * q.step;
  const int cx = centre ? centre[3 * static_cast<size_t>(node)] : 0;
  const int cy = centre ? centre[3 * static_cast<size_t>(node) + 1] : 0;
  const int cz = centre ? centre[3 * static_cast<size_t>(node) + 2] : 0;

  for (int i = tid; i < ((m.a_bytes + m.b_bytes) >> 2); i += kLanes) lds[i] = 0u;
  if (tid < 8) counters[tid] = 0;
  __syncthreads();

  // the window of a: inside the box (the entry has checked it)
  int sa = 0, saa = 0, nans = 0;
  for (int i = tid; i < side * side * side; i += kLanes) {
    const int wx = i % side, wy = (i / side) % side, wz = i / (side * side);
    bool is_nan;
    const unsigned c = code_of(m.rule, a[f3d_row(g, py - W + wy, pz - W + wz) + static_cast<size_t>(px - W + wx)], &is_nan);
    a_codes[(wz * side + wy) * (4 * kAw) + wx] = static_cast<unsigned char>(c);
    sa += static_cast<int>(c);
    saa += static_cast<int>(c * c);
    nans += is_nan ? 1 : 0;
  }
  if (sa) atomicAdd(&counters[0], sa);
  if (saa) atomicAdd(&counters[1], saa);
  if (nans) atomicAdd(&counters[2], nans);
  // the region of b: its corner is the node + the centre - (W + r); what lies outside the box keeps its 0
  const int x0 = px + cx - W - q.rx, y0 = py + cy - W - q.ry, z0 = pz + cz - W - q.rz;
  for (int i = tid; i < m.ex * m.ey * m.ez; i += kLanes) {
    const int rx = i % m.ex, ry = (i / m.ex) % m.ey, rz = i / (m.ex * m.ey);
    const int x = x0 + rx, y = y0 + ry, z = z0 + rz;
    if (x >= 0 && x < g.W && y >= 0 && y < g.H && z >= 0 && z < g.D) {
      bool is_nan;
      b_codes[(rz * m.ey + ry) * m.b_pitch + rx] =
          static_cast<unsigned char>(code_of(m.rule, b[f3d_row(g, y, z) + static_cast<size_t>(x)], &is_nan));
    }
  }
  __syncthreads();

  const long long n = static_cast<long long>(side) * side * side;
  const long long Sa = counters[0], Saa = counters[1];
  const long long da = n * Saa - Sa * Sa;
  const int kx = 2 * q.rx + 1, ky = 2 * q.ry + 1, kz = 2 * q.rz + 1;
  // a candidate (ix, iy, iz) of the search, 0 .. 2r per axis: is its window inside the box?
  auto inside = [&](int ix, int iy, int iz) {
    const int x = x0 + ix, y = y0 + iy, z = z0 + iz;  // first voxel of the target window
    return x >= 0 && x + side <= g.W && y >= 0 && y + side <= g.H && z >= 0 && z + side <= g.D;
  };

  double score = -__builtin_huge_val();
  int index = INT_MAX;
  int evaluated = 0, outside = 0, flat = 0;
  if (da != 0) {
    for (int c = tid; c < kx * ky * kz; c += kLanes) {
      const int ix = c % kx, iy = (c / kx) % ky, iz = c / (kx * ky);
      if (!inside(ix, iy, iz)) {
        ++outside;
        continue;
      }
      const Sums s = candidate_sums<kAw>(a_lds, b_lds, m, ix, iy, iz);
      const long long db = n * s.sbb - static_cast<long long>(s.sb) * s.sb;
      if (db == 0) {
        ++flat;
        continue;
      }
      ++evaluated;
      const double num = static_cast<double>(n * s.sab - Sa * s.sb);
      const double squared = num * fabs(num);
      const double t = squared / static_cast<double>(db);
      if (better(t, c, score, index)) {
        score = t;
        index = c;
      }
    }
    if (evaluated) atomicAdd(&counters[3], evaluated);
    if (outside) atomicAdd(&counters[4], outside);
    if (flat) atomicAdd(&counters[5], flat);
  }
  best_score[tid] = score;
  best_index[tid] = index;
  __syncthreads();
  for (int half = kLanes / 2; half > 0; half >>= 1) {
    if (tid < half && better(best_score[tid + half], best_index[tid + half], best_score[tid], best_index[tid])) {
      best_score[tid] = best_score[tid + half];
      best_index[tid] = best_index[tid + half];
    }
    __syncthreads();
  }

  if (tid >= 64) return;  // the first wave writes the record: lane 0 the head, lanes 0 .. 6 the sums at the best shift and round it
  int* rec = records + static_cast<size_t>(node) * kRecordWords;
  const int best = best_index[0];
  const bool found = best != INT_MAX;
  const int ix = found ? best % kx : 0, iy = found ? (best / kx) % ky : 0, iz = found ? best / (kx * ky) : 0;
  bool valid = false;
  Sums s = {0, 0, 0};
  if (found && tid < 7) {
    int jx = ix, jy = iy, jz = iz;
    if (tid == 1) --jx;
    if (tid == 2) ++jx;
    if (tid == 3) --jy;
    if (tid == 4) ++jy;
    if (tid == 5) --jz;
    if (tid == 6) ++jz;
    if (jx >= 0 && jx < kx && jy >= 0 && jy < ky && jz >= 0 && jz < kz && inside(jx, jy, jz)) {
      s = candidate_sums<kAw>(a_lds, b_lds, m, jx, jy, jz);
      valid = n * s.sbb - static_cast<long long>(s.sb) * s.sb != 0;
      if (!valid) s = {0, 0, 0};
    }
  }
  const unsigned long long votes = __ballot(valid);
  if (tid < 7) {
    rec[9 + 3 * tid] = s.sb;
    rec[10 + 3 * tid] = s.sbb;
    rec[11 + 3 * tid] = s.sab;
  }
  if (tid == 0) {
    rec[0] = found ? cx + ix - q.rx : 0;
    rec[1] = found ? cy + iy - q.ry : 0;
    rec[2] = found ? cz + iz - q.rz : 0;
    rec[3] = da == 0 ? F3D_BLOCK_MATCH_FLAT : (found ? F3D_BLOCK_MATCH_OK : F3D_BLOCK_MATCH_NONE);
    rec[4] = counters[3];
    rec[5] = counters[4];
    rec[6] = counters[5];
    rec[7] = counters[0];
    rec[8] = counters[1];
    rec[30] = static_cast<int>((votes >> 1) & 63u);
    rec[31] = counters[2];
  }
}

// one axis of the expansion: the lower node and the fraction (include/f3d_block_match.h)
__device__ __forceinline__ void cell_of_axis(int x, int origin, int step, int count, int* i, float* f)
{
  const float t = (static_cast<float>(x) - static_cast<float>(origin)) / static_cast<float>(step);
  const int lower = f3d_clampi(static_cast<int>(floorf(t)), 0, count - 2);
  const float fraction = t - static_cast<float>(lower);
  *i = count > 1 ? lower : 0;
  *f = fraction < 0.f ? 0.f : (fraction > 1.f ? 1.f : fraction);
}

__device__ __forceinline__ float lerp_nodes(float p, float q, float f)
{
  const float step = q - p;
  const float part = f * step;
  return p + part;
}

struct ExpandArgs {
  int ox, oy, oz, step, nx, ny, nz;
};

__global__ __launch_bounds__(kBX* kBY) void k_expand_nodes(const float* __restrict__ nodes, ExpandArgs e, float* __restrict__ out_u,
                                                           float* __restrict__ out_v, float* __restrict__ out_w, F3dGeo g)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z = g.z_lo + blockIdx.z;
  if (x >= g.W || y >= g.H) return;
  int i, j, k;
  float fx, fy, fz;
  cell_of_axis(x, e.ox, e.step, e.nx, &i, &fx);
  cell_of_axis(y, e.oy, e.step, e.ny, &j, &fy);
  cell_of_axis(z, e.oz, e.step, e.nz, &k, &fz);
  const size_t count = static_cast<size_t>(e.nx) * e.ny * e.nz;
  const int i1 = e.nx > 1 ? i + 1 : i, j1 = e.ny > 1 ? j + 1 : j, k1 = e.nz > 1 ? k + 1 : k;
  float* const out[3] = {out_u, out_v, out_w};
  const size_t at = f3d_row(g, y, z) + static_cast<size_t>(x);
  for (int c = 0; c < 3; ++c) {
    const float* f = nodes + c * count;
    auto along_x = [&](int jj, int kk) {
      const size_t row = (static_cast<size_t>(kk) * e.ny + jj) * e.nx;
      return e.nx > 1 ? lerp_nodes(f[row + i], f[row + i1], fx) : f[row + i];
    };
    auto along_y = [&](int kk) { return e.ny > 1 ? lerp_nodes(along_x(j, kk), along_x(j1, kk), fy) : along_x(j, kk); };
    out[c][at] = e.nz > 1 ? lerp_nodes(along_y(k), along_y(k1), fz) : along_y(k);
  }
}

template <int kAw>
void launch_match(int nodes, size_t lds_bytes, const float* a, const float* b, const F3dGeo& g, const MatchArgs& m, const int* centre,
                  int* records)
{
  hipLaunchKernelGGL(k_block_match<kAw>, dim3(nodes), dim3(kLanes), lds_bytes, f3d::stream(), a, b, g, m, centre, records);
}

}  // namespace

extern "C" {

int f3d_block_match(f3d_devptr a, f3d_devptr b, float lo, float hi, size_t bins, size_t width, size_t height, size_t depth,
                    const f3d_block_match_grid* grid, const int* centre, f3d_block_match_record* records, f3d_block_match_info* info)
{
  F3D_REQUIRE_READY("f3d_block_match");
  if (!a || !b || !grid || !records) return f3d::fail("f3d_block_match: null argument");
  MatchArgs m;
  if (bins < 2 || bins > F3D_BLOCK_MATCH_MAX_BINS) return f3d::fail("f3d_block_match: bins must be 2 .. 256");
  if (const char* why = f3d_hist::make_rule(lo, hi, static_cast<long long>(bins), &m.rule)) return f3d::fail("f3d_block_match: %s", why);
  const f3d_block_match_grid& q = *grid;
  if (q.step < 1) return f3d::fail("f3d_block_match: the step must be at least 1");
  if (q.nx < 1 || q.ny < 1 || q.nz < 1) return f3d::fail("f3d_block_match: the grid is empty");
  const unsigned long long count = static_cast<unsigned long long>(q.nx) * q.ny * q.nz;
  if (count > F3D_BLOCK_MATCH_MAX_NODES) return f3d::fail("f3d_block_match: more than 2^22 nodes");
  if (q.window < 1 || q.window > F3D_BLOCK_MATCH_MAX_WINDOW) return f3d::fail("f3d_block_match: the half-window must be 1 .. 8");
  if (q.rx < 0 || q.ry < 0 || q.rz < 0) return f3d::fail("f3d_block_match: a search radius is negative");
  const int r_max = q.rx > q.ry ? (q.rx > q.rz ? q.rx : q.rz) : (q.ry > q.rz ? q.ry : q.rz);
  if (r_max > F3D_BLOCK_MATCH_MAX_REACH || q.window + r_max > F3D_BLOCK_MATCH_MAX_REACH)
    return f3d::fail("f3d_block_match: window + search radius must not exceed 16");
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_block_match")) return 1;
  const long long first[3] = {q.ox, q.oy, q.oz}, counts[3] = {q.nx, q.ny, q.nz}, dims[3] = {g.W, g.H, g.D};
  for (int axis = 0; axis < 3; ++axis)
    if (first[axis] - q.window < 0 || first[axis] + (counts[axis] - 1) * q.step + q.window > dims[axis] - 1)
      return f3d::fail("f3d_block_match: the window of a node leaves the box along %c", "xyz"[axis]);
  if (centre)
    for (unsigned long long i = 0; i < 3 * count; ++i)
      if (centre[i] < -kCentreLimit || centre[i] > kCentreLimit) return f3d::fail("f3d_block_match: a centre component is beyond +-2^20");

  m.grid = q;
  m.side = 2 * q.window + 1;
  m.ex = 2 * (q.window + q.rx) + 1;
  m.ey = 2 * (q.window + q.ry) + 1;
  m.ez = 2 * (q.window + q.rz) + 1;
  m.b_pitch = (m.ex + 4 + 3) & ~3;
  const int aw = (m.side + 3) / 4;
  m.a_bytes = m.side * m.side * 4 * aw;
  m.b_bytes = m.ey * m.ez * m.b_pitch + 8;
  const size_t lds_bytes = static_cast<size_t>(m.a_bytes) + m.b_bytes;

  const size_t record_bytes = count * sizeof(f3d_block_match_record), centre_bytes = centre ? count * 3 * sizeof(int) : 0;
  void* d_buf = nullptr;
  if (f3d::scratch_buffer(record_bytes + centre_bytes, &d_buf)) return 1;
  int* d_records = static_cast<int*>(d_buf);
  int* d_centre = centre ? d_records + count * kRecordWords : nullptr;
  if (centre) F3D_HIP(hipMemcpyAsync(d_centre, centre, centre_bytes, hipMemcpyHostToDevice, f3d::stream()));
  const float* pa = f3d_ptr<const float>(a);
  const float* pb = f3d_ptr<const float>(b);
  const int nodes = static_cast<int>(count);
  switch (aw) {
    case 1: launch_match<1>(nodes, lds_bytes, pa, pb, g, m, d_centre, d_records); break;
    case 2: launch_match<2>(nodes, lds_bytes, pa, pb, g, m, d_centre, d_records); break;
    case 3: launch_match<3>(nodes, lds_bytes, pa, pb, g, m, d_centre, d_records); break;
    case 4: launch_match<4>(nodes, lds_bytes, pa, pb, g, m, d_centre, d_records); break;
    default: launch_match<5>(nodes, lds_bytes, pa, pb, g, m, d_centre, d_records); break;
  }
  F3D_HIP(hipGetLastError());
  // into memory of the library's first: a call that fails on the way leaves the caller's records as they were
  f3d_block_match_record* held = static_cast<f3d_block_match_record*>(std::malloc(record_bytes));
  if (!held) return f3d::fail("f3d_block_match: no host memory for %llu records", count);
  hipError_t e = hipMemcpyAsync(held, d_records, record_bytes, hipMemcpyDeviceToHost, f3d::stream());
  if (e == hipSuccess) e = hipStreamSynchronize(f3d::stream());
  if (e != hipSuccess) {
    std::free(held);
    return f3d::hip_fail(e, "f3d_block_match: reading the records", __FILE__, __LINE__);
  }
  __builtin_memcpy(records, held, record_bytes);
  std::free(held);
  if (info) {
    f3d_block_match_info t = {};
    t.nodes = count;
    for (unsigned long long i = 0; i < count; ++i) {
      const f3d_block_match_record& r = records[i];
      t.ok += r.status == F3D_BLOCK_MATCH_OK;
      t.flat_nodes += r.status == F3D_BLOCK_MATCH_FLAT;
      t.none_nodes += r.status == F3D_BLOCK_MATCH_NONE;
      t.evaluated += static_cast<unsigned long long>(r.evaluated);
      t.outside += static_cast<unsigned long long>(r.outside);
      t.flat += static_cast<unsigned long long>(r.flat);
      t.nan += static_cast<unsigned long long>(r.nan);
    }
    *info = t;
  }
  return 0;
}

int f3d_expand_nodes(const float* u, const float* v, const float* w, int ox, int oy, int oz, int step, int nx, int ny, int nz,
                     f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w, size_t width, size_t height, size_t depth)
{
  F3D_REQUIRE_READY("f3d_expand_nodes");
  if (!u || !v || !w || !out_u || !out_v || !out_w) return f3d::fail("f3d_expand_nodes: null argument");
  if (out_u == out_v || out_u == out_w || out_v == out_w) return f3d::fail("f3d_expand_nodes: two outputs share a container");
  if (step < 1) return f3d::fail("f3d_expand_nodes: the step must be at least 1");
  if (nx < 1 || ny < 1 || nz < 1) return f3d::fail("f3d_expand_nodes: the grid is empty");
  const unsigned long long count = static_cast<unsigned long long>(nx) * ny * nz;
  if (count > F3D_BLOCK_MATCH_MAX_NODES) return f3d::fail("f3d_expand_nodes: more than 2^22 nodes");
  if (ox < -kCentreLimit || ox > kCentreLimit || oy < -kCentreLimit || oy > kCentreLimit || oz < -kCentreLimit || oz > kCentreLimit)
    return f3d::fail("f3d_expand_nodes: the origin is beyond +-2^20");
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_expand_nodes")) return 1;
  void* d_buf = nullptr;
  if (f3d::scratch_buffer(3 * count * sizeof(float), &d_buf)) return 1;
  float* d_nodes = static_cast<float*>(d_buf);
  const float* host[3] = {u, v, w};
  for (int c = 0; c < 3; ++c)
    F3D_HIP(hipMemcpyAsync(d_nodes + c * count, host[c], count * sizeof(float), hipMemcpyHostToDevice, f3d::stream()));
  const ExpandArgs e = {ox, oy, oz, step, nx, ny, nz};
  const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, g.z_hi - g.z_lo);
  hipLaunchKernelGGL(k_expand_nodes, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), d_nodes, e, f3d_ptr<float>(out_u), f3d_ptr<float>(out_v),
                     f3d_ptr<float>(out_w), g);
  F3D_HIP(hipGetLastError());
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  return 0;
}

}  // extern "C"
