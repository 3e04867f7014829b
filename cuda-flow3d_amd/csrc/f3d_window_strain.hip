// Strain fields of a displacement from a least-squares gradient for gfx950: per voxel the displacement gradient G is the slope of the
// unweighted least-squares plane through the present samples of its (2r+1)^3 window, from exact integer moments of the presence
// mask and nine window sums per component formed separably (x, then y, then z) in binary64; from G the eight strain fields of
// f3d_flow_strain by its own float32 expressions (f3d_strain_grad.h).  The definition, the order of every addition and product and
// the tail are those of include/f3d.h (f3d_window_strain); tests/window_strain_ref.py restates them in numpy and matches the kernel
// bit for bit.
//
// Shape: k_local_correlation's (f3d_correlation.hip).  A workgroup of 256 threads owns a tile of kTX x kTY voxels of a plane and
// marches in z over a run of kZ planes, primed with 2r planes.  Per plane:
//   1. the samples of the tile plus an r-wide halo, (kTX + 2r) x (kTY + 2r) triples (u, v, w), go through registers into LDS -- they
//      were loaded a step ahead; a point outside the volume is stored as NaN, which makes it absent, and an absent point adds +0;
//   2. x sums: a thread takes two neighbouring x of one of the kTY + 2r rows and adds, per component, a0 = sum t and a1 = sum i t
//      in ascending x; the sums go back to LDS, the row's mask moments (n, sum i, sum i^2 and the centre's presence) in one word;
//   3. y sums: every thread adds the 2r + 1 rows of its own column in ascending y (b00 = sum a0, b10 = sum a1, b01 = sum j a0) and
//      keeps the plane's nine sums and six mask moments in a register ring of 2r + 1 planes (static indices, see ring_steps);
//   4. z sums: once the ring is full the thread adds its planes in ascending z, solves the 3 x 3 normal equations of the voxel r
//      planes back (integer adjugate and determinant, one binary64 division per entry of G) and stores the selected outputs.
// Nothing is carried from voxel to voxel (no running add / subtract), so a result does not depend on where a march started.
//
// The ring: nine binary64 sums and six small integers per plane.  The integers are kept exact end to end and travel packed two to a
// register (|moment of a plane| <= 196 < 2^15), which makes the ring 21 registers per plane, 147 at r = 3.  That is more than the LDS
// holds for a 32 x 8 tile and fits the 512-entry register file of a lane at two waves per SIMD, so the whole ring lives in registers
// and LDS carries only the samples and the x sums of one plane (DESIGN.md section 19 has the resource table).
//
// Statistics (optional): each workgroup reduces its voxels into one partial in a buffer of its own; a one-workgroup kernel then folds
// the partials in a fixed order (f3d_partials.h), so the result does not depend on scheduling (no float atomics).
#include <utility>

#include "f3d_strain_grad.h"

namespace {

using namespace f3d_partials;

constexpr int kTX = 32;  // tile of a plane
constexpr int kTY = 8;
constexpr int kZ = 32;   // planes of a run
constexpr int kWaves = kTX * kTY / 64;
constexpr int kOutputs = 17;

struct WindowStrainPartial {
  unsigned long long defined, folded, lost, thin;
  float vol_min, vol_max, eq_max, pad;
  double vol_sum;

  static __device__ __forceinline__ WindowStrainPartial identity()
  {
    return {0ull, 0ull, 0ull, 0ull, INFINITY, -INFINITY, -INFINITY, 0.f, 0.0};
  }
  __device__ __forceinline__ void merge(const WindowStrainPartial& q)
  {
    defined += q.defined;
    folded += q.folded;
    lost += q.lost;
    thin += q.thin;
    vol_min = fminf(vol_min, q.vol_min);
    vol_max = fmaxf(vol_max, q.vol_max);
    eq_max = fmaxf(eq_max, q.eq_max);
    vol_sum += q.vol_sum;
  }
};

struct WindowStrainOut {
  float* f[kOutputs];  // vol, exx, eyy, ezz, exy, exz, eyz, eq, G00 .. G22 (null = not stored)
};

// two integers of |value| < 2^15 in one register
__device__ __forceinline__ int pack2(int lo, int hi)
{
  return static_cast<int>((static_cast<unsigned>(lo) & 0xffffu) | (static_cast<unsigned>(hi) << 16));
}
__device__ __forceinline__ int low_of(int p) { return static_cast<short>(static_cast<unsigned>(p) & 0xffffu); }
__device__ __forceinline__ int high_of(int p) { return p >> 16; }

// step(integral_constant<P>) for P = 0, 1, ... until one returns false: the march unrolled over the ring, so that every ring index
// is a constant in each copy of the step (f3d_correlation.hip has the reason)
template <typename Step, int... P>
__device__ __forceinline__ bool ring_steps(Step& step, std::integer_sequence<int, P...>)
{
  return (step(std::integral_constant<int, P>{}) && ...);
}

// include/f3d.h, f3d_window_strain.  R: the radius; partials only with STATS.
template <int R, bool STATS>
__global__ __launch_bounds__(kTX* kTY) void k_window_strain(const float* __restrict__ du, const float* __restrict__ dv,
                                                            const float* __restrict__ dw, WindowStrainOut out, F3dGeo g,
                                                            int min_count, WindowStrainPartial* __restrict__ partials)
{
  constexpr int kRing = 2 * R + 1;
  constexpr int kLX = kTX + 2 * R, kLY = kTY + 2 * R;  // the tile with its halo
  constexpr int kThreads = kTX * kTY;
  constexpr int kLoads = (kLX * kLY + kThreads - 1) / kThreads;  // points of the haloed tile per thread
  static_assert(kLY * kTX / 2 <= kThreads, "the x sums take two points of a row per thread");
  // x_mask: bits 0-3 n, 4-7 (sum i) + 8, 8-15 sum i^2, 16 the row's own point is present
  constexpr int kCentre = 1 << 16;

  __shared__ float sample[3][kLY * kLX];
  __shared__ double x_sum[6][kLY][kTX];  // a0 of u, v, w, then a1 of u, v, w
  __shared__ int x_mask[kLY][kTX];

  const int tid = threadIdx.y * 64 + threadIdx.x;
  const int tx = tid % kTX, ty = tid / kTX;
  const int x = blockIdx.x * kTX + tx, y = blockIdx.y * kTY + ty;
  const bool owner = x < g.W && y < g.H;
  const int z_begin = blockIdx.z * kZ;
  const int z_end = min(g.D, z_begin + kZ);
  const int steps = z_end - z_begin + 2 * R;  // step s handles plane z_begin - R + s

  // this thread's points of the haloed tile: the offset inside a plane, or -1 outside the volume
  long long load_at[kLoads];
#pragma unroll
  for (int l = 0; l < kLoads; ++l) {
    const int i = tid + l * kThreads;
    const int px = blockIdx.x * kTX - R + i % kLX, py = blockIdx.y * kTY - R + i / kLX;
    const bool in = i < kLX * kLY && px >= 0 && px < g.W && py >= 0 && py < g.H;
    load_at[l] = in ? static_cast<long long>(py) * g.pitch + px : -1;
  }
  float next[kLoads][3];
  auto load_plane = [&](int z) {
    const bool plane = z >= 0 && z < g.D;
    const size_t base = plane ? f3d_row(g, 0, z) : 0;
#pragma unroll
    for (int l = 0; l < kLoads; ++l) {
      next[l][0] = next[l][1] = next[l][2] = __builtin_nanf("");
      if (plane && load_at[l] >= 0) {
        next[l][0] = du[base + load_at[l]];
        next[l][1] = dv[base + load_at[l]];
        next[l][2] = dw[base + load_at[l]];
      }
    }
  };

  // the y sums of the newest 2r + 1 planes, plane of step s in slot s % kRing: b00, b10, b01 of u, then of v, then of w, and the
  // plane's mask moments (n, Sx), (Sy, Sxx), (Sxy, Syy)
  double ring[kRing][9];
  int ring_mask[kRing][3];
  unsigned centres = 0;  // bit k: this thread's own point k planes back is present
  WindowStrainPartial sum = WindowStrainPartial::identity();

  load_plane(z_begin - R);
  for (int first = 0; first < steps; first += kRing) {
    auto step = [&](auto slot_of_step) __attribute__((always_inline)) {
      constexpr int p = decltype(slot_of_step)::value;
      const int s = first + p;
      if (s >= steps) return false;  // the same for the whole workgroup
      const int z = z_begin - R + s;

      // 1. the plane's samples into LDS; the next plane's on their way
#pragma unroll
      for (int l = 0; l < kLoads; ++l)
        if (tid + l * kThreads < kLX * kLY) {
          sample[0][tid + l * kThreads] = next[l][0];
          sample[1][tid + l * kThreads] = next[l][1];
          sample[2][tid + l * kThreads] = next[l][2];
        }
      if (s + 1 < steps) load_plane(z + 1);
      __syncthreads();

      // 2. x sums of two neighbouring points of one row: point 0 spans i = 0 .. 2r of the 2r + 2 samples, point 1 spans 1 .. 2r + 1
      if (tid < kLY * kTX / 2) {
        const int row = tid / (kTX / 2), xp = (tid % (kTX / 2)) * 2;
        double a0[2][3], a1[2][3];
        int n[2] = {0, 0}, sx[2] = {0, 0}, sxx[2] = {0, 0}, centre[2] = {0, 0};
#pragma unroll
        for (int i = 0; i < kRing + 1; ++i) {
          const float v[3] = {sample[0][row * kLX + xp + i], sample[1][row * kLX + xp + i], sample[2][row * kLX + xp + i]};
          const bool present = !(isnan(v[0]) || isnan(v[1]) || isnan(v[2]));
          const int m = present ? 1 : 0;
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int o = i - q - R;  // the sample's offset from point q
            if (o < -R || o > R) continue;
            n[q] += m;
            sx[q] += o * m;
            sxx[q] += o * o * m;
            if (o == 0) centre[q] = present ? kCentre : 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const double t = present ? static_cast<double>(v[c]) : 0.0;
              const double it = static_cast<double>(o) * t;
              if (o == -R) {
                a0[q][c] = t;
                a1[q][c] = it;
              } else {
                a0[q][c] += t;
                a1[q][c] += it;
              }
            }
          }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            x_sum[c][row][xp + q] = a0[q][c];
            x_sum[3 + c][row][xp + q] = a1[q][c];
          }
          x_mask[row][xp + q] = n[q] | ((sx[q] + 8) << 4) | (sxx[q] << 8) | centre[q];
        }
      }
      __syncthreads();

      // 3. y sums of this thread's column into the ring (the next step writes x_sum only behind its first barrier)
      {
        int n = 0, Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0;
#pragma unroll
        for (int dy = 0; dy < kRing; ++dy) {
          const int j = dy - R;
          const int word = x_mask[ty + dy][tx];
          const int nx = word & 15, sx = ((word >> 4) & 15) - 8, sxx = (word >> 8) & 255;
          n += nx;
          Sx += sx;
          Sy += j * nx;
          Sxx += sxx;
          Sxy += j * sx;
          Syy += j * j * nx;
          if (dy == R) centres = (centres << 1) | (word >= kCentre ? 1u : 0u);
        }
        ring_mask[p][0] = pack2(n, Sx);
        ring_mask[p][1] = pack2(Sy, Sxx);
        ring_mask[p][2] = pack2(Sxy, Syy);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double b00, b10, b01;
#pragma unroll
          for (int dy = 0; dy < kRing; ++dy) {
            const double a0 = x_sum[c][ty + dy][tx], a1 = x_sum[3 + c][ty + dy][tx];
            const double ja0 = static_cast<double>(dy - R) * a0;
            if (dy == 0) {
              b00 = a0;
              b10 = a1;
              b01 = ja0;
            } else {
              b00 += a0;
              b10 += a1;
              b01 += ja0;
            }
          }
          ring[p][3 * c + 0] = b00;
          ring[p][3 * c + 1] = b10;
          ring[p][3 * c + 2] = b01;
        }
      }

      // 4. the voxel r planes back: z sums oldest plane first, the normal equations, then the float32 tail
      if (s >= 2 * R) {
        int n = 0, Sx = 0, Sy = 0, Sz = 0, Sxx = 0, Sxy = 0, Sxz = 0, Syy = 0, Syz = 0, Szz = 0;
        double D[3][4];  // per component D0, Dx, Dy, Dz
#pragma unroll
        for (int k = 0; k < kRing; ++k) {
          const int slot = (p + 1 + k) % kRing;
          const int kz = k - R;
          const int nk = low_of(ring_mask[slot][0]), sxk = high_of(ring_mask[slot][0]), syk = low_of(ring_mask[slot][1]);
          n += nk;
          Sx += sxk;
          Sy += syk;
          Sz += kz * nk;
          Sxx += high_of(ring_mask[slot][1]);
          Sxy += low_of(ring_mask[slot][2]);
          Sxz += kz * sxk;
          Syy += high_of(ring_mask[slot][2]);
          Syz += kz * syk;
          Szz += kz * kz * nk;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double b00 = ring[slot][3 * c], kb00 = static_cast<double>(kz) * b00;
            if (k == 0) {
              D[c][0] = b00;
              D[c][1] = ring[slot][3 * c + 1];
              D[c][2] = ring[slot][3 * c + 2];
              D[c][3] = kb00;
            } else {
              D[c][0] += b00;
              D[c][1] += ring[slot][3 * c + 1];
              D[c][2] += ring[slot][3 * c + 2];
              D[c][3] += kb00;
            }
          }
        }
        const bool present = (centres >> R) & 1u;
        const float nan = __builtin_nanf("");
        float G[3][3] = {{nan, nan, nan}, {nan, nan, nan}, {nan, nan, nan}};
        bool fitted = false;
        if (present && n >= min_count) {
          // the normal matrix n S_ab - S_a S_b and its adjugate in exact integers (|C| < 2^19, |adj| < 2^39, det < 2^57 at r <= 3)
          const long long c00 = g.W == 1 ? 1 : n * Sxx - Sx * Sx, c11 = g.H == 1 ? 1 : n * Syy - Sy * Sy,
                          c22 = g.D == 1 ? 1 : n * Szz - Sz * Sz;
          const long long c01 = n * Sxy - Sx * Sy, c02 = n * Sxz - Sx * Sz, c12 = n * Syz - Sy * Sz;
          const long long adj00 = c11 * c22 - c12 * c12, adj01 = c02 * c12 - c01 * c22, adj02 = c01 * c12 - c02 * c11;
          const long long adj11 = c00 * c22 - c02 * c02, adj12 = c01 * c02 - c00 * c12, adj22 = c00 * c11 - c01 * c01;
          const long long det = c00 * adj00 + c01 * adj01 + c02 * adj02;
          if (det != 0) {
            fitted = true;
            const double dn = static_cast<double>(n), dSx = static_cast<double>(Sx), dSy = static_cast<double>(Sy),
                         dSz = static_cast<double>(Sz), ddet = static_cast<double>(det);
            const double a00 = static_cast<double>(adj00), a01 = static_cast<double>(adj01), a02 = static_cast<double>(adj02),
                         a11 = static_cast<double>(adj11), a12 = static_cast<double>(adj12), a22 = static_cast<double>(adj22);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const double r0 = dn * D[c][1] - dSx * D[c][0], r1 = dn * D[c][2] - dSy * D[c][0], r2 = dn * D[c][3] - dSz * D[c][0];
              G[c][0] = static_cast<float>(((a00 * r0 + a01 * r1) + a02 * r2) / ddet);
              G[c][1] = static_cast<float>(((a01 * r0 + a11 * r1) + a12 * r2) / ddet);
              G[c][2] = static_cast<float>(((a02 * r0 + a12 * r1) + a22 * r2) / ddet);
            }
          }
        }
        float vol, exx, eyy, ezz, exy, exz, eyz, eq;
        f3d_strain::strain_fields(G[0][0], G[0][1], G[0][2], G[1][0], G[1][1], G[1][2], G[2][0], G[2][1], G[2][2], vol, exx, eyy, ezz,
                                  exy, exz, eyz, eq);
        if (owner) {
          const size_t i = f3d_row(g, y, z - R) + x;
          const float vals[kOutputs] = {vol,     exx,     eyy,     ezz,     exy,     exz,     eyz,     eq,     G[0][0],
                                        G[0][1], G[0][2], G[1][0], G[1][1], G[1][2], G[2][0], G[2][1], G[2][2]};
#pragma unroll
          for (int f = 0; f < kOutputs; ++f)
            if (out.f[f]) out.f[f][i] = vals[f];
          if (STATS) {
            if (!present) ++sum.lost;
            else if (!fitted) ++sum.thin;
            if (!isnan(vol)) {
              ++sum.defined;
              sum.folded += vol <= -1.f ? 1 : 0;
              sum.vol_min = fminf(sum.vol_min, vol);
              sum.vol_max = fmaxf(sum.vol_max, vol);
              sum.eq_max = fmaxf(sum.eq_max, eq);
              sum.vol_sum += static_cast<double>(vol);
            }
          }
        }
      }
      return true;
    };
    ring_steps(step, std::make_integer_sequence<int, kRing>{});
  }

  if (STATS) {
    sum.defined = wave_sum(sum.defined);
    sum.folded = wave_sum(sum.folded);
    sum.lost = wave_sum(sum.lost);
    sum.thin = wave_sum(sum.thin);
    sum.vol_min = wave_min(sum.vol_min);
    sum.vol_max = wave_max(sum.vol_max);
    sum.eq_max = wave_max(sum.eq_max);
    sum.vol_sum = wave_sum(sum.vol_sum);
    block_partial<WindowStrainPartial, kWaves>(sum, partials);
  }
}

template <int R>
int launch(const float* u, const float* v, const float* w, const WindowStrainOut& o, const F3dGeo& g, int min_count,
           f3d_window_strain_stats* stats)
{
  const dim3 grid((g.W + kTX - 1) / kTX, (g.H + kTY - 1) / kTY, (g.D + kZ - 1) / kZ), block(64, kWaves, 1);
  if (!stats) {
    hipLaunchKernelGGL((k_window_strain<R, false>), grid, block, 0, f3d::stream(), u, v, w, o, g, min_count, nullptr);
    F3D_HIP(hipGetLastError());
    return 0;
  }
  WindowStrainPartial r;
  if (reduce_partials(static_cast<size_t>(grid.x) * grid.y * grid.z, &r, [&](WindowStrainPartial* d_part) {
        hipLaunchKernelGGL((k_window_strain<R, true>), grid, block, 0, f3d::stream(), u, v, w, o, g, min_count, d_part);
      }))
    return 1;
  stats->defined = r.defined;
  stats->folded = r.folded;
  stats->lost = r.lost;
  stats->thin = r.thin;
  stats->vol_min = r.defined ? r.vol_min : __builtin_nanf("");
  stats->vol_max = r.defined ? r.vol_max : __builtin_nanf("");
  stats->eq_max = r.defined ? r.eq_max : __builtin_nanf("");
  stats->vol_sum = r.vol_sum;
  return 0;
}

}  // namespace

extern "C" {

int f3d_window_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[17], unsigned fields, unsigned radius,
                      unsigned min_count, size_t width, size_t height, size_t depth, f3d_window_strain_stats* stats)
{
  F3D_REQUIRE_READY("f3d_window_strain");
  if (!u || !v || !w) return f3d::fail("f3d_window_strain: null input");
  if (fields == 0 || (fields & ~(F3D_STRAIN_VOL | F3D_STRAIN_E | F3D_STRAIN_EQ | F3D_WSTRAIN_G)))
    return f3d::fail("f3d_window_strain: fields must be a non-empty combination of F3D_STRAIN_VOL, F3D_STRAIN_E, F3D_STRAIN_EQ, "
                     "F3D_WSTRAIN_G (got %u)", fields);
  if (!out) return f3d::fail("f3d_window_strain: null output array");
  if (radius < 1 || radius > 3) return f3d::fail("f3d_window_strain: radius must be 1 .. 3 (got %u)", radius);
  const unsigned window = (2 * radius + 1) * (2 * radius + 1) * (2 * radius + 1);
  if (min_count < 1 || min_count > window)
    return f3d::fail("f3d_window_strain: min_count must be 1 .. %u at radius %u (got %u)", window, radius, min_count);
  static const char* const names[kOutputs] = {"vol", "exx", "eyy", "ezz", "exy", "exz", "eyz", "eq", "G00",
                                              "G01", "G02", "G10", "G11", "G12", "G20", "G21", "G22"};
  static const unsigned groups[kOutputs] = {F3D_STRAIN_VOL, F3D_STRAIN_E,  F3D_STRAIN_E,  F3D_STRAIN_E,  F3D_STRAIN_E,  F3D_STRAIN_E,
                                            F3D_STRAIN_E,   F3D_STRAIN_EQ, F3D_WSTRAIN_G, F3D_WSTRAIN_G, F3D_WSTRAIN_G, F3D_WSTRAIN_G,
                                            F3D_WSTRAIN_G,  F3D_WSTRAIN_G, F3D_WSTRAIN_G, F3D_WSTRAIN_G, F3D_WSTRAIN_G};
  WindowStrainOut o;
  if (!f3d::select_outputs("f3d_window_strain", "the window reads neighbours", o.f, out, kOutputs, names, groups, fields, u, v, w))
    return 1;
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_window_strain")) return 1;
  const float *pu = f3d_ptr<const float>(u), *pv = f3d_ptr<const float>(v), *pw = f3d_ptr<const float>(w);
  const int k = static_cast<int>(min_count);
  switch (radius) {
    case 1: return launch<1>(pu, pv, pw, o, g, k, stats);
    case 2: return launch<2>(pu, pv, pw, o, g, k, stats);
    default: return launch<3>(pu, pv, pw, o, g, k, stats);
  }
}

}  // extern "C"
