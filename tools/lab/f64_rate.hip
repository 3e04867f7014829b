// Lab: at what rate does gfx950 issue binary64 vector adds and multiplies?  k_local_correlation (f3d_correlation.hip) is some 170
// binary64 operations per voxel, so where it sits depends on that rate.  Every wave runs a loop of 8 independent chains of one
// instruction (v_add_f32 as the yardstick, v_add_f64, v_mul_f64, v_fma_f64), 1, 2 or 4 waves per SIMD on every CU; the time between
// HIP events gives wave-instructions per second, and the ratio to the v_add_f32 line is the answer that does not need the clock.
#include <hip/hip_runtime.h>
#include <cstdio>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr int kChains = 8, kUnroll = 16;

template <int OP>
__global__ __launch_bounds__(1024) void k(double* out, int loops, double seed)
{
  double d[kChains];
  float f[kChains];
#pragma unroll
  for (int i = 0; i < kChains; ++i) {
    d[i] = seed + i + threadIdx.x;
    f[i] = static_cast<float>(d[i]);
  }
  const double dk = seed * 0.5;
  const float fk = static_cast<float>(dk);
  for (int l = 0; l < loops; ++l)
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
#pragma unroll
      for (int i = 0; i < kChains; ++i) {
        if (OP == 0) asm volatile("v_add_f32 %0, %0, %1" : "+v"(f[i]) : "v"(fk));
        if (OP == 1) asm volatile("v_add_f64 %0, %0, %1" : "+v"(d[i]) : "v"(dk));
        if (OP == 2) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(d[i]) : "v"(dk));
        if (OP == 3) asm volatile("v_fma_f64 %0, %0, %1, %1" : "+v"(d[i]) : "v"(dk));
      }
  double s = 0;
#pragma unroll
  for (int i = 0; i < kChains; ++i) s += d[i] + f[i];
  out[(blockIdx.x * blockDim.y + threadIdx.y) * 64 + threadIdx.x] = s;
}

int main()
{
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const double mhz = prop.clockRate / 1000.0;
  double* out;
  CK(hipMalloc(&out, sizeof(double) * cus * 16 * 64));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const char* names[4] = {"v_add_f32", "v_add_f64", "v_mul_f64", "v_fma_f64"};
  const int loops = 20000;
  double base[3] = {0, 0, 0};
  for (int op = 0; op < 4; ++op)
    for (int wi = 0; wi < 3; ++wi) {
      const int waves = 4 << wi;  // per CU: 1, 2, 4 per SIMD
      auto launch = [&](int n) {
        const dim3 grid(cus), block(64, waves);
        if (op == 0) k<0><<<grid, block>>>(out, n, 1.0);
        if (op == 1) k<1><<<grid, block>>>(out, n, 1.0);
        if (op == 2) k<2><<<grid, block>>>(out, n, 1.0);
        if (op == 3) k<3><<<grid, block>>>(out, n, 1.0);
      };
      launch(100);
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0));
      launch(loops);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      const double per_simd = double(loops) * kUnroll * kChains * waves / 4;  // wave-instructions each SIMD issued
      const double ns = ms * 1e6 / per_simd;
      if (op == 0) base[wi] = ns;
      printf("%s, %d waves per SIMD: %.3f ns per wave-instruction and SIMD = %.2f cycles at %.0f MHz, %.2f x v_add_f32\n", names[op],
             waves / 4, ns, ns * mhz * 1e-3, mhz, ns / base[wi]);
    }
  return 0;
}
