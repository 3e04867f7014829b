// The start of a pyramid that does not begin at zero, for gfx950: a caller's displacement (a coarse DVC, an FE prediction, a rigid
// pre-registration, the flow of the pair before) made fit to start a solve from, and what was found in it.
//
// Per voxel of the box: three finite components are copied bit for bit (a -0 stays -0); otherwise all three become +0 and the voxel
// counts in `replaced`.  `leaving` counts the finite voxels whose end point (x + u, y + v, z + w), one float add per axis as in
// k_compose_flow, lies outside [0, W-1] x [0, H-1] x [0, D-1]; `max_abs` is the largest |component| over the finite voxels.  The
// counts are integers and the maximum is an integer atomicMax on the bits of a non-negative float (their order is the order of the
// values), so the four results are the same bytes whatever the schedule (tests/warm_start_ref.py restates them).
//
// Shape as k_compose_flow: one voxel per lane, a wave64 on 64 consecutive x of one row, a workgroup 4 rows; a ballot and a popcount
// per wave and one 64-bit atomic per counter per wave that has anything to add.  Compulsory traffic: 3 reads and 3 writes =
// 24 B/voxel.  This is not a hot path: it runs once per solve that starts from a displacement.
#include "f3d_gather.h"

namespace {

using namespace f3d_gather;

struct InitialCounters {
  unsigned long long replaced, leaving;
  unsigned int max_abs_bits;
  unsigned int pad;
};

// every store of the kernel is a vector store: the components per lane, the counters through atomics issued by lane 0 of a wave
__global__ __launch_bounds__(kBX* kBY) void k_initial_flow(const float* u, const float* v, const float* w, float* out_u, float* out_v,
                                                           float* out_w, F3dGeo g, InitialCounters* counters)
{
  // (no __restrict__: out_* may be the inputs themselves; each lane reads its own voxel before it writes it)
  const int x = blockIdx.x * kBX + threadIdx.x;
  const int y = blockIdx.y * kBY + threadIdx.y;
  const int z = g.z_lo + blockIdx.z;
  bool is_replaced = false, is_leaving = false;
  unsigned int bits = 0;  // of the largest |component|: the order of the bits of non-negative floats is the order of their values
  if (x < g.W && y < g.H) {
    const size_t c = f3d_row(g, y, z) + x;
    float a = u[c], b = v[c], d = w[c];
    if (isfinite(a) && isfinite(b) && isfinite(d)) {
      is_leaving = !inside(g, static_cast<float>(x) + a, static_cast<float>(y) + b, static_cast<float>(z) + d);
      const unsigned int sign_off = 0x7fffffffu;
      bits = max(max(__float_as_uint(a) & sign_off, __float_as_uint(b) & sign_off), __float_as_uint(d) & sign_off);
    } else {
      a = b = d = 0.f;
      is_replaced = true;
    }
    out_u[c] = a;
    out_v[c] = b;
    out_w[c] = d;
  }
  if (counters) {
    // every lane of the wave takes part (no early return before this point)
    const unsigned long long n_replaced = __popcll(__ballot(is_replaced));
    const unsigned long long n_leaving = __popcll(__ballot(is_leaving));
    for (int offset = 32; offset > 0; offset >>= 1) bits = max(bits, static_cast<unsigned int>(__shfl_xor(static_cast<int>(bits), offset)));
    if (threadIdx.x == 0) {
      if (n_replaced) atomicAdd(&counters->replaced, n_replaced);
      if (n_leaving) atomicAdd(&counters->leaving, n_leaving);
      if (bits) atomicMax(&counters->max_abs_bits, bits);
    }
  }
}

// the calling thread's device counters (per thread: two lanes may ask at once); a call that uses them ends in a wait on the
// thread's stream, so no two uses are ever in flight
int counters_zero(InitialCounters** d_counters)
{
  static thread_local InitialCounters* counters = nullptr;
  if (!counters) F3D_HIP(hipMalloc(reinterpret_cast<void**>(&counters), sizeof(InitialCounters)));
  F3D_HIP(hipMemsetAsync(counters, 0, sizeof(InitialCounters), f3d::stream()));
  *d_counters = counters;
  return 0;
}

}  // namespace

extern "C" {

int f3d_initial_flow(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w, size_t width,
                     size_t height, size_t depth, f3d_initial_info* info)
{
  F3D_REQUIRE_READY("f3d_initial_flow");
  if (!u || !v || !w || !out_u || !out_v || !out_w) return f3d::fail("f3d_initial_flow: null argument");
  // in place means component for component; any other sharing would let one lane's store reach another component's load
  const f3d_devptr in[3] = {u, v, w}, out[3] = {out_u, out_v, out_w};
  for (int i = 0; i < 3; ++i)
    for (int o = 0; o < 3; ++o)
      if (i != o && (in[i] == out[o] || out[i] == out[o]))
        return f3d::fail("f3d_initial_flow: an output may be its own input, not another component's container");
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_initial_flow")) return 1;
  InitialCounters* d_counters = nullptr;
  if (info && counters_zero(&d_counters)) return 1;
  if (g.z_hi > g.z_lo) {
    const dim3 grid((g.W + kBX - 1) / kBX, (g.H + kBY - 1) / kBY, g.z_hi - g.z_lo);
    hipLaunchKernelGGL(k_initial_flow, grid, dim3(kBX, kBY, 1), 0, f3d::stream(), f3d_ptr<const float>(u), f3d_ptr<const float>(v),
                       f3d_ptr<const float>(w), f3d_ptr<float>(out_u), f3d_ptr<float>(out_v), f3d_ptr<float>(out_w), g, d_counters);
    F3D_HIP(hipGetLastError());
  }
  if (!info) return 0;
  InitialCounters host;
  F3D_HIP(hipMemcpyAsync(&host, d_counters, sizeof(host), hipMemcpyDeviceToHost, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  info->voxels = static_cast<unsigned long long>(width) * height * depth;
  info->replaced = host.replaced;
  info->leaving = host.leaving;
  static_assert(sizeof(float) == sizeof(unsigned int), "the maximum travels as the bits of a float");
  __builtin_memcpy(&info->max_abs, &host.max_abs_bits, sizeof(float));
  return 0;
}

}  // extern "C"
