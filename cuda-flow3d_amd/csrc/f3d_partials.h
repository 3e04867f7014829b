// The statistics skeleton of f3d_flow_strain, f3d_principal_strain and f3d_invert_displacement: every workgroup of the main kernel
// reduces its voxels into one partial P in a buffer of the call's own, and a one-workgroup kernel folds the n partials into
// partials[n].  P supplies identity() and merge(const P&); everything else is here.  The order of combination is fixed, so a result
// does not depend on scheduling (no float atomics), and it is part of the results: a double sum's bits depend on it.
//   within a wave:  the xor butterfly 32, 16, ..., 1 (wave_min / wave_max / wave_sum)
//   across waves:   wave_part[0], then 1 .. WAVES-1 in sequence (block_partial)
//   in the fold:    thread t takes t, t + 256, ... in that order from the identity, then the halving tree 128 ... 1 (fold_partials)
// The reductions of f3d_stream_ops.hip are on the benchmarked solver path and are deliberately not built on this header.
#ifndef F3D_PARTIALS_H_
#define F3D_PARTIALS_H_
#include "f3d_internal.h"

namespace f3d_partials {

constexpr int kReduceThreads = 256;

__device__ __forceinline__ float wave_min(float x)
{
  for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float wave_max(float x)
{
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ double wave_sum(double x)
{
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x)
{
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// the wave's value (lane 0's copy) of each of the WAVES waves of a (64, WAVES) workgroup through LDS into the workgroup's slot;
// every thread of the workgroup calls it (no early return before it)
template <typename P, int WAVES>
__device__ __forceinline__ void block_partial(const P& wave_value, P* __restrict__ partials)
{
  __shared__ P wave_part[WAVES];
  if (threadIdx.x == 0) wave_part[threadIdx.y] = wave_value;
  __syncthreads();
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    P p = wave_part[0];
    for (int i = 1; i < WAVES; ++i) p.merge(wave_part[i]);
    partials[(static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = p;
  }
}

template <typename P>
__global__ __launch_bounds__(kReduceThreads) void fold_partials(P* __restrict__ partials, size_t n)
{
  __shared__ P part[kReduceThreads];
  P p = P::identity();
  for (size_t i = threadIdx.x; i < n; i += kReduceThreads) p.merge(partials[i]);
  part[threadIdx.x] = p;
  __syncthreads();
  for (int s = kReduceThreads / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) part[threadIdx.x].merge(part[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[n] = part[0];
}

// the calling thread's buffer of at least `count` partials (grow-only; per thread: two lanes may ask at once)
template <typename P>
int partial_buffer(size_t count, P** buffer)
{
  static thread_local P* d_part = nullptr;
  static thread_local size_t d_part_count = 0;
  if (d_part_count < count) {
    if (d_part) F3D_HIP(hipFree(d_part));
    d_part = nullptr;
    d_part_count = 0;
    F3D_HIP(hipMalloc(reinterpret_cast<void**>(&d_part), count * sizeof(P)));
    d_part_count = count;
  }
  *buffer = d_part;
  return 0;
}

// main(partials) enqueues the kernel whose n workgroups write one partial each (not called when n is 0); then the fold, the copy of
// its result and the wait for it
template <typename P, typename Main>
int reduce_partials(size_t n, P* result, Main&& main)
{
  P* d_part;
  if (partial_buffer(n + 1, &d_part)) return 1;
  if (n) {
    main(d_part);
    F3D_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(fold_partials<P>, dim3(1), dim3(kReduceThreads), 0, f3d::stream(), d_part, n);
  F3D_HIP(hipGetLastError());
  F3D_HIP(hipMemcpyAsync(result, d_part + n, sizeof(P), hipMemcpyDeviceToHost, f3d::stream()));
  F3D_HIP(hipStreamSynchronize(f3d::stream()));
  return 0;
}

}  // namespace f3d_partials
#endif  // F3D_PARTIALS_H_
