// The trilinear gather of the derived-field kernels, k_compose_flow (f3d_trajectory.hip), k_invert_displacement and k_carry_field
// (f3d_inverse.hip), and the count of the voxels a launch lost.  The gather is k_warp's (f3d_stream_ops.hip, registration_3d.cu:66-79:
// the same products and sums in the same order, contraction off), so a float32 restatement matches each kernel bit for bit.  k_warp
// itself is on the benchmarked solver path and deliberately keeps its own copy; so do that file's reductions.
// Shape of every kernel here: one voxel per lane, a wave64 on kBX consecutive x of one row, a workgroup kBY rows, one plane per
// blockIdx.z.  Everything device-side is inlined into its kernel.
#ifndef F3D_GATHER_H_
#define F3D_GATHER_H_
#include "f3d_internal.h"

namespace f3d_gather {

constexpr int kBX = 64;
constexpr int kBY = 4;

// p inside [0, W-1] x [0, H-1] x [0, D-1] and not NaN
__device__ __forceinline__ bool inside(const F3dGeo& g, float x_f, float y_f, float z_f)
{
  return !(isnan(x_f) || isnan(y_f) || isnan(z_f) || (x_f < 0.f) || (x_f > static_cast<float>(g.W - 1)) || (y_f < 0.f) ||
           (y_f > static_cast<float>(g.H - 1)) || (z_f < 0.f) || (z_f > static_cast<float>(g.D - 1)));
}

// the corners and fractions of an inside position (floor, fractions, min(n - 1, i + 1))
struct Cell {
  size_t r00, r10, r01, r11;
  int xi, x1;
  float dx, dy, dz;
};

__device__ __forceinline__ Cell cell_of(const F3dGeo& g, float x_f, float y_f, float z_f)
{
  Cell c;
  c.xi = static_cast<int>(floorf(x_f));
  const int yi = static_cast<int>(floorf(y_f));
  const int zi = static_cast<int>(floorf(z_f));
  c.dx = x_f - static_cast<float>(c.xi);
  c.dy = y_f - static_cast<float>(yi);
  c.dz = z_f - static_cast<float>(zi);
  c.x1 = min(g.W - 1, c.xi + 1);
  const int y1 = min(g.H - 1, yi + 1);
  const int z1 = min(g.D - 1, zi + 1);
  c.r00 = f3d_row(g, yi, zi);
  c.r10 = f3d_row(g, y1, zi);
  c.r01 = f3d_row(g, yi, z1);
  c.r11 = f3d_row(g, y1, z1);
  return c;
}

// the products and sums in this order are part of the results (contraction is off in this build)
__device__ __forceinline__ float trilinear(const float* __restrict__ f, const Cell& c)
{
  const float dx = c.dx, dy = c.dy, dz = c.dz;
  const float v0 = (1.f - dx) * (1.f - dy) * f[c.r00 + c.xi] + (dx) * (1.f - dy) * f[c.r00 + c.x1] +
                   (1.f - dx) * (dy)*f[c.r10 + c.xi] + (dx) * (dy)*f[c.r10 + c.x1];
  const float v1 = (1.f - dx) * (1.f - dy) * f[c.r01 + c.xi] + (dx) * (1.f - dy) * f[c.r01 + c.x1] +
                   (1.f - dx) * (dy)*f[c.r11 + c.xi] + (dx) * (dy)*f[c.r11 + c.x1];
  return (1.f - dz) * v0 + dz * v1;
}

// `lost` (nullable) gains the number of lanes with is_lost.  Every lane of the wave takes part (no early return before it): a
// ballot, and one atomic per wave that has anything to add.
__device__ __forceinline__ void count_lost(unsigned long long* lost, bool is_lost)
{
  if (lost) {
    const unsigned long long n = __popcll(__ballot(is_lost));
    if (threadIdx.x == 0 && n) atomicAdd(lost, n);
  }
}

// Host side of the count: *d_lost is the calling thread's zeroed device counter (per thread: two lanes may ask at once), or null
// when the caller of the entry point did not ask (lost null); lost_read() after the launch waits for it and stores it.
// The one counter per thread is shared by every entry point that counts (f3d_compose_flow, f3d_carry_field), on purpose: a call
// that uses it ends in lost_read()'s wait on the thread's stream, so no two uses are ever in flight.
inline int lost_zero(const unsigned long long* lost, unsigned long long** d_lost)
{
  static thread_local unsigned long long* counter = nullptr;
  *d_lost = nullptr;
  if (!lost) return 0;
  if (!counter) F3D_HIP(hipMalloc(reinterpret_cast<void**>(&counter), sizeof(unsigned long long)));
  F3D_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), f3d::stream()));
  *d_lost = counter;
  return 0;
}

inline int lost_read(unsigned long long* lost, const unsigned long long* d_lost)
{
  if (!lost) return 0;
  unsigned long long n = 0;
  F3D_HIP(hipMemcpyAsync(&n, d_lost, sizeof(n), hipMemcpyDeviceToHost, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  *lost = n;
  return 0;
}

}  // namespace f3d_gather
#endif  // F3D_GATHER_H_
