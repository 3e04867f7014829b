// Trajectory accumulation for gfx950: the flows of a frame sequence composed into the displacement of every material point of
// frame 0 (Lagrangian, frame 0's grid, voxel units).
//
// Pair k's flow f_k lives on frame k's grid (frame_{k+1}(x + f_k(x)) ~ frame_k(x), registration_3d.cu's convention), so a point
// that frame 0 had at x and that has moved to x + a(x) moves on by f_k sampled THERE:  a(x) += f_k(x + a(x)).  The sample is
// the trilinear gather of f3d_gather.h (k_warp's products and sums in the same order, contraction off), so a float32 restatement
// of the kernel matches it bit for bit (tests/trajectory_ref.py).  A point whose
// position leaves the volume, or is already NaN, becomes NaN in all three components and stays NaN ("lost").
//
// Shape as k_warp: one voxel per lane, a wave64 on 64 consecutive x of one row, a workgroup 4 rows.  Own-voxel acc loads and stores
// are coalesced (256 B per wave); the 24 gathers of inc (8 corners x 3 components) fall on the same and the neighbouring rows while
// displacements are small and are served by L1/L2.  Compulsory traffic: 3 reads of acc, 3 of inc, 3 writes of acc = 36 B/voxel.
#include "f3d_gather.h"

namespace {

using namespace f3d_gather;

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
    if (!inside(g, x_f, y_f, z_f)) {
      au = av = aw = __builtin_nanf("");
      is_lost = true;
    } else {
      const Cell cell = cell_of(g, x_f, y_f, z_f);
      au = au + trilinear(inc_u, cell);
      av = av + trilinear(inc_v, cell);
      aw = aw + trilinear(inc_w, cell);
      // a finite position with a NaN sample (inc holds NaN there) loses the point too: the count is of NaN acc_u
      is_lost = isnan(au);
    }
    acc_u[c] = au;
    acc_v[c] = av;
    acc_w[c] = aw;
  }
  count_lost(lost, is_lost);
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
  unsigned long long* d_lost;
  if (lost_zero(lost, &d_lost)) return 1;
  if (g.z_hi > g.z_lo) {
    const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, g.z_hi - g.z_lo);
    hipLaunchKernelGGL(k_compose_flow, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), f3d_ptr<float>(acc_u), f3d_ptr<float>(acc_v),
                       f3d_ptr<float>(acc_w), f3d_ptr<const float>(inc_u), f3d_ptr<const float>(inc_v),
                       f3d_ptr<const float>(inc_w), g, d_lost);
    F3D_HIP(hipGetLastError());
  }
  return lost_read(lost, d_lost);
}

}  // extern "C"
