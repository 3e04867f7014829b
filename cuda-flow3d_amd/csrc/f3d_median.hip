// 3-D median filter of the flow components for gfx950 (window diameter 3, 5 or 7, mirror boundary).
//
// Replaces src/kernels/median_3d.cu:49-299 of the reference: the output is the
// element of rank r^3/2 of the r^3 window gathered at mirrored indices.  The reference sorts a 343-float
// per-thread local array by insertion; any exact selection gives the same value, so here
//   r = 3, 5 : the window lives in VGPRs and goes through a Batcher odd-even merge network of
//              compare-exchanges (v_min_f32 / v_max_f32); everything that does not feed rank r^3/2 is
//              pruned at compile time by dead-code elimination (1184 of 1441 exchanges remain for r = 5),
//   r = 7    : 343 values do not fit the register file; exact rank selection by bisection on the
//              order-preserving integer image of the floats (32 counting passes over the window).
// The only observable difference to a stable sort is the sign of a zero result when the window holds both
// -0 and +0 (they compare equal); values are otherwise identical.  Between the kernels of this file the same holds:
// v_min_f32 / v_max_f32 of gfx950 order -0 below +0 (the ISA's pseudo-code handles the pair explicitly), so any two
// correct networks of them alone return the same bits, but the file is built with NaN-free min/max and the compiler
// then turns some max(min(a, b), min(max(a, b), c)) into v_med3_f32, which picks by comparing for equality.
// k_median_share can therefore differ from k_median_keep in the sign of a zero result of such a window, and nowhere
// else (tests/test_gpu_median_share.py counts it: none of 14 479 zero results on its mixed-zero volume).
#include "f3d_internal.h"

#include <cstdlib>

namespace {

constexpr int kBX = 64;
constexpr int kBY = 4;

__device__ __forceinline__ void cmp_exchange(float& a, float& b)
{
  const float lo = fminf(a, b);
  const float hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// Batcher's odd-even merge sort for arbitrary N, fully unrolled over a register array.  Exchanges whose results nobody
// reads afterwards disappear at compile time, so a caller that looks at a few ranks only pays for what feeds them.
template <int N>
__device__ __forceinline__ void sort_network(float (&v)[N])
{
#pragma unroll
  for (int p = 1; p < N; p <<= 1) {
#pragma unroll
    for (int k = p; k >= 1; k >>= 1) {
#pragma unroll
      for (int j = k % p; j <= N - 1 - k; j += 2 * k) {
#pragma unroll
        for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i) {
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) cmp_exchange(v[i + j], v[i + j + k]);
        }
      }
    }
  }
}

template <int N>
__device__ __forceinline__ float rank_middle(float (&v)[N])
{
  sort_network(v);
  return v[N / 2];
}

// The element of rank NB (0-based) of the union of two SORTED lists a[0 .. NB] (NB + 1 values) and b[0 .. NB-1]: with
// i values taken from a and NB + 1 - i from b it is min over i of max(a[i-1], b[NB-i]) -- NB max, NB min.
template <int NB>
__device__ __forceinline__ float rank_nb_of_two_sorted(const float* a, const float* b)
{
  float r = a[NB];
#pragma unroll
  for (int i = 1; i <= NB; ++i) r = fminf(r, fmaxf(a[i - 1], b[NB - i]));
  return r;
}

// Up to three volumes of one box per launch (f3d_median_n: u, v, w of a level): grid.z = z-chunks x volumes, a workgroup finds its
// volume by subtraction (scalar work; the kernels below are register-bound and must not pay a vector division for it).
constexpr int kMaxBatch = 3;
struct MedVols {
  const float* in[kMaxBatch];
  float* out[kMaxBatch];
  int zblocks;  // z-chunks (bisection kernel: planes) per volume
};
__device__ __forceinline__ int med_volume(const MedVols& v, int& zb)
{
  int vol = 0;
  zb = static_cast<int>(blockIdx.z);
  while (zb >= v.zblocks) {
    zb -= v.zblocks;
    ++vol;
  }
  return vol;
}

// LDS-staged variant: a workgroup of 64 x 4 lanes marches along z over a chunk of planes.  The (64 + 2h) x (4 + 2h)
// mirrored footprint of every plane is fetched once into a ring of R planes in LDS (a few loads per lane and step);
// the R^3 window of a voxel is then R^3 LDS reads instead of R^3 cached global loads with 64-bit address arithmetic.
template <int R>
__global__ __launch_bounds__(kBX* kBY) void k_median_net(MedVols mv, F3dGeo g, int zchunk)
{
  int zb;
  const int vol = med_volume(mv, zb);
  const float* __restrict__ in = mv.in[vol];
  float* __restrict__ out = mv.out[vol];
  constexpr int HALF = R / 2;
  constexpr int TW = kBX + 2 * HALF, TH = kBY + 2 * HALF;
  __shared__ float ring[R][TH][TW];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  const int x0 = blockIdx.x * kBX, y0 = blockIdx.y * kBY;
  const int x = x0 + threadIdx.x;
  const int y = y0 + threadIdx.y;
  const int z0 = g.z_lo + zb * zchunk;
  const int z1 = min(z0 + zchunk, g.z_hi);
  const bool owner = x < g.W && y < g.H;

  // plane zz (any integer: mirrored) -> ring slot (zz mod R), cooperatively
  auto fetch = [&](int zz) {
    const int zm = f3d_clampi(f3d_mir(zz, g.D), 0, g.D - 1);
    float(*dst)[TW] = ring[((zz % R) + R) % R];
    for (int i = tid; i < TW * TH; i += kBX * kBY) {
      const int ty = i / TW, tx = i - ty * TW;
      const int xs = f3d_clampi(f3d_mir(x0 + tx - HALF, g.W), 0, g.W - 1);
      const int ys = f3d_clampi(f3d_mir(y0 + ty - HALF, g.H), 0, g.H - 1);
      dst[ty][tx] = in[f3d_row(g, ys, zm) + xs];
    }
  };
  for (int zz = z0 - HALF; zz < z0 + HALF; ++zz) fetch(zz);
  for (int z = z0; z < z1; ++z) {
    fetch(z + HALF);
    __syncthreads();
    float v[R * R * R];
#pragma unroll
    for (int iz = 0; iz < R; ++iz) {
      const float(*pl)[TW] = ring[(((z + iz - HALF) % R) + R) % R];
#pragma unroll
      for (int iy = 0; iy < R; ++iy)
#pragma unroll
        for (int ix = 0; ix < R; ++ix) v[(iz * R + iy) * R + ix] = pl[threadIdx.y + iy][threadIdx.x + ix];
    }
    const float med = rank_middle<R * R * R>(v);
    if (owner) out[f3d_row(g, y, z) + x] = med;
    __syncthreads();  // the slot of plane z - HALF is overwritten by the next fetch
  }
}

// Two outputs per lane and step.  The windows of voxels (x, y, z) and (x, y, z+1) share R-1 of their R planes: S, (R-1) R^2
// values.  With m = (R^3 - 1) / 2 the rank looked for, an element of S can be the median of S u P (P = the R^2 values of the
// one plane a window has for itself) only if its rank inside S lies in [m - R^2, m], and the median is then the element of
// rank R^2 among those R^2 + 1 candidates and the sorted P.  So a pair costs ONE pruned sorting network over S (ranks
// m - R^2 .. m), two small full sorts and two min/max chains -- 2 524 min/max for two outputs at R = 5 against 2 x 2 244 of
// the single-output network -- and holds ~110 values at a time instead of 125 + temporaries.
template <int R>
__global__ __launch_bounds__(kBX* kBY) void k_median_pair(MedVols mv, F3dGeo g, int zchunk)
{
  int zb;
  const int vol = med_volume(mv, zb);
  const float* __restrict__ in = mv.in[vol];
  float* __restrict__ out = mv.out[vol];
  constexpr int HALF = R / 2;
  constexpr int TW = kBX + 2 * HALF, TH = kBY + 2 * HALF;
  constexpr int NS = R + 1;  // ring slots: planes z-HALF .. z+HALF+1
  constexpr int RR = R * R, NSH = (R - 1) * RR, M = (R * R * R - 1) / 2;
  __shared__ float ring[NS][TH][TW];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  const int x0 = blockIdx.x * kBX, y0 = blockIdx.y * kBY;
  const int x = x0 + threadIdx.x;
  const int y = y0 + threadIdx.y;
  const int z0 = g.z_lo + zb * zchunk;
  const int z1 = min(z0 + zchunk, g.z_hi);
  const bool owner = x < g.W && y < g.H;
  const int zz_max = z1 - 1 + HALF;  // the last plane this chunk may touch (a slab window holds nothing beyond it)

  auto slot_of = [&](int zz) { return ((zz % NS) + NS) % NS; };
  auto fetch = [&](int zz) {
    const int zm = f3d_clampi(f3d_mir(min(zz, zz_max), g.D), 0, g.D - 1);
    float(*dst)[TW] = ring[slot_of(zz)];
    for (int i = tid; i < TW * TH; i += kBX * kBY) {
      const int ty = i / TW, tx = i - ty * TW;
      const int xs = f3d_clampi(f3d_mir(x0 + tx - HALF, g.W), 0, g.W - 1);
      const int ys = f3d_clampi(f3d_mir(y0 + ty - HALF, g.H), 0, g.H - 1);
      dst[ty][tx] = in[f3d_row(g, ys, zm) + xs];
    }
  };
  auto gather = [&](int zz, float* v) __attribute__((always_inline)) {
    const float(*pl)[TW] = ring[slot_of(zz)];
#pragma unroll
    for (int iy = 0; iy < R; ++iy)
#pragma unroll
      for (int ix = 0; ix < R; ++ix) v[iy * R + ix] = pl[threadIdx.y + iy][threadIdx.x + ix];
  };
  for (int zz = z0 - HALF; zz < z0 + HALF; ++zz) fetch(zz);
  for (int z = z0; z < z1; z += 2) {
    fetch(z + HALF);
    fetch(z + HALF + 1);
    __syncthreads();
    float s[NSH];
#pragma unroll
    for (int iz = 0; iz < R - 1; ++iz) gather(z - HALF + 1 + iz, s + iz * RR);
    sort_network(s);
    float p[RR];
    gather(z - HALF, p);
    sort_network(p);
    const float med_a = rank_nb_of_two_sorted<RR>(s + (M - RR), p);
    gather(z + HALF + 1, p);
    sort_network(p);
    const float med_b = rank_nb_of_two_sorted<RR>(s + (M - RR), p);
    if (owner) {
      out[f3d_row(g, y, z) + x] = med_a;
      if (z + 1 < z1) out[f3d_row(g, y, z + 1) + x] = med_b;
    }
    __syncthreads();  // the slots of planes z - HALF and z - HALF + 1 are overwritten by the next fetches
  }
}

#include "f3d_median_nets.h"

// 5^3 with the SORTED planes kept: a lane holds the sorted 25-lists of the four newest planes in registers, so a pair of
// outputs costs two fresh plane sorts (2 x 280 min/max), two merges of neighbouring plane lists (2 x 238), the pruned merge
// that yields the 26 candidates (244) and the two selection chains (2 x 50): 1 380 for two outputs against 2 524 with the
// sort of the raw 100 in k_median_pair.  Planes are named Q0 .. Q5 = z-2 .. z+3; a step consumes the lists of Q0 and Q1 and
// produces those of Q4 and Q5, so six register arrays rotate by two per step and the march is unrolled three steps deep to
// make the rotation a renaming.  ~200 live values at the peak: two waves per SIMD, like the single-output network.
__global__ __launch_bounds__(kBX* kBY) void k_median_keep(MedVols mv, F3dGeo g, int zchunk)
{
  int zb;
  const int vol = med_volume(mv, zb);
  const float* __restrict__ in = mv.in[vol];
  float* __restrict__ out = mv.out[vol];
  constexpr int R = 5, HALF = 2;
  constexpr int TW = kBX + 2 * HALF, TH = kBY + 2 * HALF;
  constexpr int NS = R + 1;
  __shared__ float ring[NS][TH][TW];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  const int x0 = blockIdx.x * kBX, y0 = blockIdx.y * kBY;
  const int x = x0 + threadIdx.x;
  const int y = y0 + threadIdx.y;
  const int z0 = g.z_lo + zb * zchunk;
  const int z1 = min(z0 + zchunk, g.z_hi);
  const bool owner = x < g.W && y < g.H;
  const int zz_max = z1 - 1 + HALF;

  auto slot_of = [&](int zz) { return ((zz % NS) + NS) % NS; };
  auto fetch = [&](int zz) {
    const int zm = f3d_clampi(f3d_mir(min(zz, zz_max), g.D), 0, g.D - 1);
    float(*dst)[TW] = ring[slot_of(zz)];
    for (int i = tid; i < TW * TH; i += kBX * kBY) {
      const int ty = i / TW, tx = i - ty * TW;
      const int xs = f3d_clampi(f3d_mir(x0 + tx - HALF, g.W), 0, g.W - 1);
      const int ys = f3d_clampi(f3d_mir(y0 + ty - HALF, g.H), 0, g.H - 1);
      dst[ty][tx] = in[f3d_row(g, ys, zm) + xs];
    }
  };
  auto sorted_plane = [&](int zz, float (&v)[25]) __attribute__((always_inline)) {
    const float(*pl)[TW] = ring[slot_of(zz)];
#pragma unroll
    for (int iy = 0; iy < R; ++iy)
#pragma unroll
      for (int ix = 0; ix < R; ++ix) v[iy * R + ix] = pl[threadIdx.y + iy][threadIdx.x + ix];
    sort_network(v);
  };
  // one pair of outputs: q0 .. q3 come in sorted, q4 and q5 are made here
  auto step = [&](const float (&q0)[25], const float (&q1)[25], const float (&q2)[25], const float (&q3)[25], float (&q4)[25],
                  float (&q5)[25], int z) __attribute__((always_inline)) {
    fetch(z + HALF);
    fetch(z + HALF + 1);
    __syncthreads();
    sorted_plane(z + HALF, q4);
    float c[26];
    {
      float ab[50], cd[50];
      merge25(q1, q2, ab);
      merge25(q3, q4, cd);
      candidates(ab, cd, c);
    }
    const float med_a = rank_nb_of_two_sorted<25>(c, q0);
    sorted_plane(z + HALF + 1, q5);
    const float med_b = rank_nb_of_two_sorted<25>(c, q5);
    if (owner) {
      out[f3d_row(g, y, z) + x] = med_a;
      if (z + 1 < z1) out[f3d_row(g, y, z + 1) + x] = med_b;
    }
    __syncthreads();
  };
  float L0[25], L1[25], L2[25], L3[25], L4[25], L5[25];
  for (int zz = z0 - HALF; zz < z0 + HALF; ++zz) fetch(zz);
  __syncthreads();
  sorted_plane(z0 - 2, L0);
  sorted_plane(z0 - 1, L1);
  sorted_plane(z0, L2);
  sorted_plane(z0 + 1, L3);
  for (int z = z0; z < z1; z += 6) {
    step(L0, L1, L2, L3, L4, L5, z);
    if (z + 2 >= z1) break;
    step(L2, L3, L4, L5, L0, L1, z + 2);
    if (z + 4 >= z1) break;
    step(L4, L5, L0, L1, L2, L3, z + 4);
  }
}

#include "f3d_median_nets_share.h"

typedef __attribute__((address_space(3))) float LdsFloat;
// one dword per lane from memory into LDS without a register in between: lane L's value lands at lds_dst + L (the s_nop is the
// wait state the M0 write in front of the instruction needs)
__device__ __forceinline__ void dma4_lane(const float* lane_addr, float* lds_dst)
{
  const unsigned m0v = static_cast<unsigned>(reinterpret_cast<unsigned long>((LdsFloat*)lds_dst));
  asm volatile("s_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(lane_addr), "{m0}"(m0v) : "memory");
}

// 5^3 with the sorted planes kept AND shared.  Against k_median_keep:
//   * merge25 of two neighbouring plane lists is formed once.  The pair (z+1, z+2) that a step merges is the pair the next
//     step needs first, so its sorted 50 go through LDS (keep[50][256], lane-major: a lane only ever reads what it wrote, and
//     the lanes of a wave hit consecutive banks) and only THREE plane lists are carried in registers: with (la, lb, lc) =
//     planes (z-2, z, z+1), a step makes q4 = z+2 and q5 = z+3 and hands (lb, q4, q5) on.  lc dies in the merge and q5 takes
//     la's registers behind med_a, so four register arrays rotate with period four and the march is unrolled four deep.
//   * a plane list is not sorted from the raw 25: every lane sorts ONE y-column (x, y-2 .. y+2) of a freshly fetched plane
//     (18 min/max; the 68 x 4 tile has 272 columns, so the first 16 lanes sort a second one), publishes it, and every lane
//     merges the five columns x-2 .. x+2 (202) -- 220 per list instead of 280.
// A step: 2 x 18 + 2 x 202 + 238 (merge25) + 244 (candidates) + 2 x 50 (selection) = 1 022 min/max for two outputs, two
// barriers, 66 432 B of LDS (two workgroups per CU).  Lanes and rows outside the volume take part in the exchange: their
// columns are read at mirrored, clamped indices like everything else.
// The file is compiled with NaN-free min/max semantics (Makefile): the window holds in-box voxels only, and without the
// promise the compiler puts a canonicalising v_max_f32 v, v, v in front of every fminf / fmaxf of a value it read from LDS.
__global__ __launch_bounds__(kBX* kBY) void k_median_share(MedVols mv, F3dGeo g, int zchunk)
{
  int zb;
  const int vol = med_volume(mv, zb);
  const float* __restrict__ in = mv.in[vol];
  float* __restrict__ out = mv.out[vol];
  constexpr int HALF = 2;
  constexpr int TW = kBX + 2 * HALF, TH = kBY + 2 * HALF;
  constexpr int NT = kBX * kBY, NCOL = TW * kBY;
  __shared__ float keep[50][NT];
  __shared__ float ring[2][TH][TW];
  __shared__ float cols[2][5][NCOL];
  const int tid = threadIdx.y * kBX + threadIdx.x;
  const int x0 = blockIdx.x * kBX, y0 = blockIdx.y * kBY;
  const int x = x0 + threadIdx.x;
  const int y = y0 + threadIdx.y;
  const int z0 = g.z_lo + zb * zchunk;
  const int z1 = min(z0 + zchunk, g.z_hi);
  const bool owner = x < g.W && y < g.H;
  const int zz_max = z1 - 1 + HALF;
  const int own = threadIdx.y * TW + threadIdx.x;  // the column x-2 of this lane's window

  // A plane goes from memory straight into the ring (global_load_lds_dword: lane L's value lands at M0 + 4 L, and a 64-lane
  // row of the workgroup is a wave, so element tid + 256 k of the flat footprint is lane L of the piece at 64 wave + 256 k).
  // No register holds a value in flight, so the planes of the NEXT step are requested as soon as the ring is free and arrive
  // behind this step's networks.  The in-plane offsets of the (at most three) elements a lane fetches do not change along
  // the march: the mirror and clamp arithmetic is done once, a request is a scalar plane base plus these.
  static_assert(kBX == 64, "one row of the workgroup must be one wave");
  constexpr int NF = (TW * TH + NT - 1) / NT;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.y));
  int off[NF];
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const int i = min(tid + k * NT, TW * TH - 1);
    const int ty = i / TW, tx = i - ty * TW;
    const int xs = f3d_clampi(f3d_mir(x0 + tx - HALF, g.W), 0, g.W - 1);
    const int ys = f3d_clampi(f3d_mir(y0 + ty - HALF, g.H), 0, g.H - 1);
    off[k] = ys * g.pitch + xs;
  }
  auto request = [&](int zz, int slot) __attribute__((always_inline)) {
    const int zm = f3d_clampi(f3d_mir(min(zz, zz_max), g.D), 0, g.D - 1);
    const float* plane = in + f3d_row(g, 0, zm);
    float* dst = &ring[slot][0][0] + wave * 64;
#pragma unroll
    for (int k = 0; k < NF; ++k)
      if (tid + k * NT < TW * TH) dma4_lane(plane + off[k], dst + k * NT);
  };
  auto sort_column = [&](int slot, int c) __attribute__((always_inline)) {
    // column c = (row c / TW, tile column c % TW): ring rows have the pitch of the column tile, so it starts at element c
    const float* top = &ring[slot][0][0] + c;
    float raw[5], s[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) raw[k] = top[k * TW];
    sort5(raw, s);
#pragma unroll
    for (int k = 0; k < 5; ++k) cols[slot][k][c] = s[k];
  };
  // the two requested planes -> sorted columns in cols[0] and cols[1]; leaves behind a barrier, after which the ring is free
  // for the next request and cols is read until the next call's first barrier
  auto columns = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces have landed ...
    __syncthreads();                                  // ... and so have everybody's
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
      sort_column(slot, tid);
      if (tid < NCOL - NT) sort_column(slot, NT + tid);
    }
    __syncthreads();
  };
  auto plane_list = [&](int slot, float (&q)[25]) __attribute__((always_inline)) {
    float v[25];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int k = 0; k < 5; ++k) v[j * 5 + k] = cols[slot][k][own + j];
    merge5x5(v, q);
  };
  // one pair of outputs: la = z-2, lb = z, lc = z+1 come in sorted, keep holds merge25(z-1, z); q4 = z+2 is made here, and
  // z+3 lands in la
  auto step = [&](float (&la)[25], const float (&lb)[25], const float (&lc)[25], float (&q4)[25], int z) __attribute__((always_inline)) {
    columns();
    if (z + 2 < z1) {  // the planes of the next step
      request(z + HALF + 2, 0);
      request(z + HALF + 3, 1);
    }
    plane_list(0, q4);
    float c[26];
    {
      float ab[50], cd[50];
      merge25(lc, q4, cd);
#pragma unroll
      for (int i = 0; i < 50; ++i) ab[i] = keep[i][tid];
      candidates(ab, cd, c);
#pragma unroll
      for (int i = 0; i < 50; ++i) keep[i][tid] = cd[i];
    }
    const float med_a = rank_nb_of_two_sorted<25>(c, la);
    plane_list(1, la);
    const float med_b = rank_nb_of_two_sorted<25>(c, la);
    if (owner) {
      out[f3d_row(g, y, z) + x] = med_a;
      if (z + 1 < z1) out[f3d_row(g, y, z + 1) + x] = med_b;
    }
    (void)lb;
  };
  float A[25], B[25], C[25], E[25];
  request(z0 - 2, 0);
  request(z0 - 1, 1);
  columns();
  request(z0, 0);
  request(z0 + 1, 1);
  plane_list(0, A);
  plane_list(1, E);
  columns();
  request(z0 + 2, 0);
  request(z0 + 3, 1);
  plane_list(0, B);
  plane_list(1, C);
  {
    float ab[50];
    merge25(E, B, ab);
#pragma unroll
    for (int i = 0; i < 50; ++i) keep[i][tid] = ab[i];
  }
  for (int z = z0; z < z1; z += 8) {
    step(A, B, C, E, z);
    if (z + 2 >= z1) break;
    step(B, E, A, C, z + 2);
    if (z + 4 >= z1) break;
    step(E, C, B, A, z + 4);
    if (z + 6 >= z1) break;
    step(C, A, E, B, z + 6);
  }
}

__device__ __forceinline__ unsigned order_key(float f)
{
  const unsigned b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// Exact rank selection without holding the window: the answer is the largest T with #(key < T) <= rank.
template <int R>
__global__ __launch_bounds__(kBX* kBY) void k_median_bisect(MedVols mv, F3dGeo g)
{
  int zb;
  const int vol = med_volume(mv, zb);
  const float* __restrict__ in = mv.in[vol];
  float* __restrict__ out = mv.out[vol];
  constexpr int HALF = R / 2;
  constexpr int RANK = (R * R * R) / 2;
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z = g.z_lo + zb;
  if (x >= g.W || y >= g.H) return;
  int xs[R];
#pragma unroll
  for (int i = 0; i < R; ++i) xs[i] = f3d_mir(x + i - HALF, g.W);
  unsigned prefix = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned cand = prefix | (1u << bit);
    int below = 0;
    for (int iz = 0; iz < R; ++iz) {
      const int zz = f3d_mir(z + iz - HALF, g.D);
      for (int iy = 0; iy < R; ++iy) {
        const size_t row = f3d_row(g, f3d_mir(y + iy - HALF, g.H), zz);
#pragma unroll
        for (int ix = 0; ix < R; ++ix) below += order_key(in[row + xs[ix]]) < cand ? 1 : 0;
      }
    }
    if (below <= RANK) prefix = cand;
  }
  const unsigned b = (prefix >> 31) ? (prefix ^ 0x80000000u) : ~prefix;
  out[f3d_row(g, y, z) + x] = __uint_as_float(b);
}

}  // namespace

static int median_launch(const f3d_devptr* inputs, size_t count, size_t width, size_t height, size_t depth, size_t radius,
                         const f3d_devptr* outputs, const f3d_slab* slab, const char* who)
{
  F3D_REQUIRE_READY(who);
  if (!inputs || !outputs) return f3d::fail("%s: null argument", who);
  if (count == 0 || count > static_cast<size_t>(kMaxBatch)) return f3d::fail("%s: %zu volumes (one launch takes 1 .. %d)", who, count, kMaxBatch);
  for (size_t i = 0; i < count; ++i)
    for (size_t j = 0; j < count; ++j)
      if (inputs[i] == outputs[j]) return f3d::fail("%s: input buffer cannot serve as output buffer", who);
  if (radius != 3 && radius != 5 && radius != 7)
    return f3d::fail("%s: wrong median radius (%zu). Supported values: 3, 5, 7", who, radius);
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, slab, who)) return 1;
  const int half = static_cast<int>(radius) / 2;
  if (g.W <= half || g.H <= half || g.D <= half)
    return f3d::fail("%s: every dimension must exceed radius/2 = %d for the mirror boundary", who, half);
  if (g.z_lo == g.z_hi) return 0;
  {
    const int dc = static_cast<int>(f3d::container().depth);
    int lo = g.z_lo - half < 0 ? 0 : g.z_lo - half;
    int hi = g.z_hi + half > g.D ? g.D : g.z_hi + half;
    if (g.z_lo - half < 0 && half + 1 > hi) hi = half + 1;
    if (g.z_hi + half > g.D && g.D - 1 - half < lo) lo = g.D - 1 - half;
    if (lo < g.z_base || hi - g.z_base > dc)
      return f3d::fail("%s: planes [%d,%d) needed but the container holds [%d,%d)", who, lo, hi, g.z_base, g.z_base + dc);
  }
  const dim3 block(kBX, kBY, 1);
  MedVols mv = {};
  for (size_t i = 0; i < count; ++i) {
    mv.in[i] = f3d_ptr<const float>(inputs[i]);
    mv.out[i] = f3d_ptr<float>(outputs[i]);
  }
  const unsigned nvol = static_cast<unsigned>(count);
  if (count > 1 && static_cast<long>(g.z_hi - g.z_lo) * static_cast<long>(count) > 65535L) {  // grid.z: volume by volume
    for (size_t i = 0; i < count; ++i)
      if (int e = median_launch(inputs + i, 1, width, height, depth, radius, outputs + i, slab, who)) return e;
    return 0;
  }
  if (radius == 7) {
    mv.zblocks = g.z_hi - g.z_lo;
    const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, mv.zblocks * nvol);
    hipLaunchKernelGGL(k_median_bisect<7>, grid, block, 0, f3d::stream(), mv, g);
  } else {
    const int planes = g.z_hi - g.z_lo;
    // workgroups of ONE z-chunk layer of the launch: the volumes of a batch fill the rounds together
    const long tiles = static_cast<long>((g.W + kBX - 1) / kBX) * ((g.H + kBY - 1) / kBY) * static_cast<long>(count);
    // F3D_MEDIAN_PAIR: 0 = the one-output-per-step network, 1 = k_median_pair, 2 = k_median_keep, 3 = k_median_share (timing
    // comparisons); unset = k_median_pair or k_median_share, whichever the model below prefers.  Read per call (a launch costs
    // far more) so that tests can switch it.
    const char* forced_env = std::getenv("F3D_MEDIAN_PAIR");
    const int forced = forced_env ? std::atoi(forced_env) : -1;
    if (forced == 0) {
      // z-chunks: enough workgroups to fill the chip, long enough to amortise the ring prologue
      long nz = (8192 + tiles - 1) / tiles;
      if (nz > planes) nz = planes;
      if (nz < 1) nz = 1;
      const int zchunk = static_cast<int>((planes + nz - 1) / nz);
      mv.zblocks = (planes + zchunk - 1) / zchunk;
      const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, mv.zblocks * nvol);
      if (radius == 3) hipLaunchKernelGGL(k_median_net<3>, grid, block, 0, f3d::stream(), mv, g, zchunk);
      if (radius == 5) hipLaunchKernelGGL(k_median_net<5>, grid, block, 0, f3d::stream(), mv, g, zchunk);
    } else {
      // Both kernels are bound by the vector unit: a chunk of zc planes costs its min/max count (per pair of planes 2 600
      // resp. 1 430, plus the four plane sorts k_median_keep starts with and a few hundred for the ring prologue), a
      // workgroup puts one wave on each SIMD of its CU, so 256 workgroups make a round whatever the occupancy, and below
      // two waves per SIMD nothing hides the LDS latency (x 1.3, measured).  Even chunks, so that only the last chunk of
      // an odd range computes a plane for nothing.  (512^3: keep 3.6 ms, pair 5.1-5.5 ms, single-output network 9.0 ms.)
      // k_median_share takes k_median_keep's place in the same model with its own counts.
      const bool share = radius == 5 && forced != 1 && forced != 2;  // unset or 3: k_median_share instead of k_median_keep
      const bool can_keep = radius == 5 && forced != 1;
      const bool can_pair = !(radius == 5 && (forced == 2 || forced == 3));
      const long pair_ops = radius == 5 ? 2600 : 330;
      // k_median_share, counted in its assembly: 1 010 min/max per pair of planes, and a chunk starts with four plane lists
      // from shared columns and one merge25 (1 190)
      const long keep_ops = share ? 1010 : 1430, keep_start = share ? 1190 : 1200;
      int zchunk = 2;
      bool keep = false;
      long best = -1;
      for (int zc = 2; zc <= planes + 1; zc += 2) {
        const long wgs = tiles * ((planes + zc - 1) / zc);
        const long rounds = (wgs + 255) / 256, thin = wgs < 512 ? 13 : 10;
        const long cost_pair = rounds * thin * (300 + (zc / 2) * pair_ops);
        const long cost_keep = rounds * thin * (300 + keep_start + (zc / 2) * keep_ops);
        if (can_pair && (best < 0 || cost_pair < best)) {
          best = cost_pair;
          zchunk = zc;
          keep = false;
        }
        if (can_keep && (best < 0 || cost_keep < best)) {
          best = cost_keep;
          zchunk = zc;
          keep = true;
        }
      }
      mv.zblocks = (planes + zchunk - 1) / zchunk;
      const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, mv.zblocks * nvol);
      if (radius == 3) hipLaunchKernelGGL(k_median_pair<3>, grid, block, 0, f3d::stream(), mv, g, zchunk);
      if (radius == 5 && keep && share) hipLaunchKernelGGL(k_median_share, grid, block, 0, f3d::stream(), mv, g, zchunk);
      if (radius == 5 && keep && !share) hipLaunchKernelGGL(k_median_keep, grid, block, 0, f3d::stream(), mv, g, zchunk);
      if (radius == 5 && !keep) hipLaunchKernelGGL(k_median_pair<5>, grid, block, 0, f3d::stream(), mv, g, zchunk);
    }
  }
  F3D_HIP(hipGetLastError());
  return 0;
}

extern "C" int f3d_median(f3d_devptr input, size_t width, size_t height, size_t depth, size_t radius, f3d_devptr output,
                          const f3d_slab* slab)
{
  return median_launch(&input, 1, width, height, depth, radius, &output, slab, "f3d_median");
}

extern "C" int f3d_median_n(const f3d_devptr* inputs, size_t count, size_t width, size_t height, size_t depth, size_t radius,
                            const f3d_devptr* outputs, const f3d_slab* slab)
{
  return median_launch(inputs, count, width, height, depth, radius, outputs, slab, "f3d_median_n");
}
