// Trajectory accumulation for gfx950: the flows of a frame sequence composed into the displacement of every material point of
// frame 0 (Lagrangian, frame 0's grid, voxel units).
//
// Pair k's flow f_k lives on frame k's grid (frame_{k+1}(x + f_k(x)) ~ frame_k(x), registration_3d.cu's convention), so a point
// that frame 0 had at x and that has moved to x + a(x) moves on by f_k sampled THERE:  a(x) += f_k(x + a(x)).  The sample is
// k_warp's trilinear gather (csrc/f3d_stream_ops.hip, registration_3d.cu:66-79: the same products and sums in the same order,
// contraction off), so a float32 restatement of the kernel matches it bit for bit (tests/trajectory_ref.py).  A point whose
// position leaves the volume, or is already NaN, becomes NaN in all three components and stays NaN ("lost").
//
// Shape as k_warp: one voxel per lane, a wave64 on 64 consecutive x of one row, a workgroup 4 rows.  Own-voxel acc loads and stores
// are coalesced (256 B per wave); the 24 gathers of inc (8 corners x 3 components) fall on the same and the neighbouring rows while
// displacements are small and are served by L1/L2.  Compulsory traffic: 3 reads of acc, 3 of inc, 3 writes of acc = 36 B/voxel.
#include "f3d_internal.h"

namespace {

constexpr int kBX = 64;
constexpr int kBY = 4;

__device__ __forceinline__ float trilinear(const float* __restrict__ f, size_t r00, size_t r10, size_t r01, size_t r11, int xi,
                                           int x1, float dx, float dy, float dz)
{
  const float v0 = (1.f - dx) * (1.f - dy) * f[r00 + xi] + (dx) * (1.f - dy) * f[r00 + x1] +
                   (1.f - dx) * (dy)*f[r10 + xi] + (dx) * (dy)*f[r10 + x1];
  const float v1 = (1.f - dx) * (1.f - dy) * f[r01 + xi] + (dx) * (1.f - dy) * f[r01 + x1] +
                   (1.f - dx) * (dy)*f[r11 + xi] + (dx) * (dy)*f[r11 + x1];
  return (1.f - dz) * v0 + dz * v1;
}

// acc (in place) += inc sampled at x + acc; `lost` (nullable) gains the number of voxels whose acc is NaN afterwards
__global__ __launch_bounds__(kBX* kBY) void k_compose_flow(float* __restrict__ acc_u, float* __restrict__ acc_v,
                                                           float* __restrict__ acc_w, const float* __restrict__ inc_u,
                                                           const float* __restrict__ inc_v, const float* __restrict__ inc_w,
                                                           F3dGeo g, unsigned long long* lost)
{
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z = g.z_lo + blockIdx.z;
  bool is_lost = false;
  if (x < g.W && y < g.H) {
    const size_t c = f3d_row(g, y, z) + x;
    float au = acc_u[c], av = acc_v[c], aw = acc_w[c];
    const float x_f = static_cast<float>(x) + au;
    const float y_f = static_cast<float>(y) + av;
    const float z_f = static_cast<float>(z) + aw;
    if (isnan(x_f) || isnan(y_f) || isnan(z_f) || (x_f < 0.f) || (x_f > static_cast<float>(g.W - 1)) || (y_f < 0.f) ||
        (y_f > static_cast<float>(g.H - 1)) || (z_f < 0.f) || (z_f > static_cast<float>(g.D - 1))) {
      au = av = aw = __builtin_nanf("");
      is_lost = true;
    } else {
      const int xi = static_cast<int>(floorf(x_f));
      const int yi = static_cast<int>(floorf(y_f));
      const int zi = static_cast<int>(floorf(z_f));
      const float dx = x_f - static_cast<float>(xi);
      const float dy = y_f - static_cast<float>(yi);
      const float dz = z_f - static_cast<float>(zi);
      const int x1 = min(g.W - 1, xi + 1);
      const int y1 = min(g.H - 1, yi + 1);
      const int z1 = min(g.D - 1, zi + 1);
      const size_t r00 = f3d_row(g, yi, zi), r10 = f3d_row(g, y1, zi);
      const size_t r01 = f3d_row(g, yi, z1), r11 = f3d_row(g, y1, z1);
      au = au + trilinear(inc_u, r00, r10, r01, r11, xi, x1, dx, dy, dz);
      av = av + trilinear(inc_v, r00, r10, r01, r11, xi, x1, dx, dy, dz);
      aw = aw + trilinear(inc_w, r00, r10, r01, r11, xi, x1, dx, dy, dz);
      // a finite position with a NaN sample (inc holds NaN there) loses the point too: the count is of NaN acc_u
      is_lost = isnan(au);
    }
    acc_u[c] = au;
    acc_v[c] = av;
    acc_w[c] = aw;
  }
  if (lost) {
    // every lane of the wave takes part (no early return above): a ballot, and one atomic per wave that has anything to add
    const unsigned long long n = __popcll(__ballot(is_lost));
    if (threadIdx.x == 0 && n) atomicAdd(lost, n);
  }
}

}  // namespace

extern "C" {

int f3d_compose_flow(f3d_devptr acc_u, f3d_devptr acc_v, f3d_devptr acc_w, f3d_devptr inc_u, f3d_devptr inc_v, f3d_devptr inc_w,
                     size_t width, size_t height, size_t depth, unsigned long long* lost)
{
  F3D_REQUIRE_READY("f3d_compose_flow");
  if (!acc_u || !acc_v || !acc_w || !inc_u || !inc_v || !inc_w) return f3d::fail("f3d_compose_flow: null argument");
  const f3d_devptr accs[3] = {acc_u, acc_v, acc_w}, incs[3] = {inc_u, inc_v, inc_w};
  for (f3d_devptr a : accs)
    for (f3d_devptr i : incs)
      if (a == i) return f3d::fail("f3d_compose_flow: an accumulated component cannot also be an increment (the update is in place)");
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_compose_flow")) return 1;
  static thread_local unsigned long long* d_lost = nullptr;   // per thread: two lanes may ask at once
  if (lost) {
    if (!d_lost) F3D_HIP(hipMalloc(reinterpret_cast<void**>(&d_lost), sizeof(unsigned long long)));
    F3D_HIP(hipMemsetAsync(d_lost, 0, sizeof(unsigned long long), f3d::stream()));
  }
  if (g.z_hi > g.z_lo) {
    const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, g.z_hi - g.z_lo);
    hipLaunchKernelGGL(k_compose_flow, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), f3d_ptr<float>(acc_u), f3d_ptr<float>(acc_v),
                       f3d_ptr<float>(acc_w), f3d_ptr<const float>(inc_u), f3d_ptr<const float>(inc_v),
                       f3d_ptr<const float>(inc_w), g, lost ? d_lost : nullptr);
    F3D_HIP(hipGetLastError());
  }
  if (lost) {
    unsigned long long n = 0;
    F3D_HIP(hipMemcpyAsync(&n, d_lost, sizeof(n), hipMemcpyDeviceToHost, f3d::stream()));
    F3D_HIP(hipStreamSynchronize(f3d::stream()));
    *lost = n;
  }
  return 0;
}

}  // extern "C"
