// Subset correlation for gfx950 (include/f3d_subset_match.h): per node of a grid, the displacement and its gradient that
// carry a (2W+1)^3 subset of frame 0 onto frame 1, by inverse-compositional Gauss-Newton on the zero-normalised sum of squared
// differences.  The header states the rule and the order of every sum; this file only says how the work is laid out.
//
// k_subset_match: one workgroup of 256 lanes per node, every iteration inside the one launch.  The (2W+3)^3 region of a round the node
// is staged in LDS as float32 (27 KB at W = 8), so F_i and the central differences are formed from LDS whenever they are needed and
// are not stored.  b is read through the cache, 64 taps per window voxel and iteration; the interpolated g_i are kept in LDS as
// binary64 (39 KB at W = 8) for the two passes that follow (G and its norm, then the right-hand side).  Lanes own the window voxels
// i = lane, lane + 256, ... and add in ascending i; block_sum takes up to four sums at a time through the fixed tree in LDS and hands
// lane 0's result to every lane, so all lanes take the same branch without a further exchange.  Lane 0 factors the Hessian, solves
// and composes the update in LDS, and the new parameters reach the others through LDS.  Everything is binary64 with contraction off
// (the build's flags); no lane depends on which wave ran first, so the bytes do not depend on the schedule.
#include "f3d_internal.h"

#include <cstdlib>

#include "f3d_subset_match.h"

namespace {

constexpr int kLanes = F3D_SUBSET_MATCH_LANES;
constexpr int kChunk = 4;         // sums that go through the tree together
constexpr int kRecordDoubles = 18;
static_assert(sizeof(f3d_subset_match_record) == kRecordDoubles * sizeof(double), "a record is 144 bytes");

struct SubsetArgs {
  f3d_subset_match_grid grid;
  int side;    // 2W + 1
  int region;  // 2W + 3
  int n;       // side^3
  int max_iterations;
  double tolerance, reach;
};

// the sums of v over the 256 lanes, by the tree of the header; every lane gets them
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red, int tid)
{
#pragma unroll
  for (int k0 = 0; k0 < N; k0 += kChunk) {
#pragma unroll
    for (int k = 0; k < kChunk; ++k)
      if (k0 + k < N) red[k * kLanes + tid] = v[k0 + k];
    __syncthreads();
    for (int half = kLanes / 2; half > 0; half >>= 1) {
      if (tid < half) {
#pragma unroll
        for (int k = 0; k < kChunk; ++k)
          if (k0 + k < N) red[k * kLanes + tid] += red[k * kLanes + tid + half];
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kChunk; ++k)
      if (k0 + k < N) v[k0 + k] = red[k * kLanes];
    __syncthreads();
  }
}

struct Voxel {
  int ex, ey, ez;  // xi + W
};

__device__ __forceinline__ Voxel voxel_of(int i, int side)
{
  return {i % side, (i / side) % side, i / (side * side)};
}

// J_i of the header from the staged region (its voxel (0, 0, 0) is c - W - 1)
template <int M>
__device__ __forceinline__ void jacobian(const float* region, int R, int W, const Voxel& q, double (&J)[M])
{
  const float* at = region + ((q.ez + 1) * R + (q.ey + 1)) * R + (q.ex + 1);
  const double fx = (static_cast<double>(at[1]) - static_cast<double>(at[-1])) * 0.5;
  const double fy = (static_cast<double>(at[R]) - static_cast<double>(at[-R])) * 0.5;
  const double fz = (static_cast<double>(at[R * R]) - static_cast<double>(at[-R * R])) * 0.5;
  if constexpr (M == 3) {
    J[0] = fx;
    J[1] = fy;
    J[2] = fz;
  } else {
    const double x = static_cast<double>(q.ex - W), y = static_cast<double>(q.ey - W), z = static_cast<double>(q.ez - W);
    const double d[3] = {fx, fy, fz};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      J[4 * c] = d[c];
      J[4 * c + 1] = d[c] * x;
      J[4 * c + 2] = d[c] * y;
      J[4 * c + 3] = d[c] * z;
    }
  }
}

template <int M>
__device__ __forceinline__ double pick(const double (&J)[M], int r, double x, double y, double z)
{
  // entry r without an index into J, which would put J into scratch memory: the same product again (x * 1.0 is x)
  if constexpr (M == 3) {
    return r == 0 ? J[0] : (r == 1 ? J[1] : J[2]);
  } else {
    const int c = r >> 2, k = r & 3;
    const double d = c == 0 ? J[0] : (c == 1 ? J[4] : J[8]);
    const double xi = k == 0 ? 1.0 : (k == 1 ? x : (k == 2 ? y : z));
    return d * xi;
  }
}

__device__ __forceinline__ double window_value(const float* region, int R, const Voxel& q)
{
  return static_cast<double>(region[((q.ez + 1) * R + (q.ey + 1)) * R + (q.ex + 1)]);
}

__device__ __forceinline__ void cubic_weights(double t, double (&w)[4])
{
  w[0] = (((2.0 - t) * t - 1.0) * t) * 0.5;
  w[1] = (((3.0 * t - 5.0) * t) * t + 2.0) * 0.5;
  w[2] = (((4.0 - 3.0 * t) * t + 1.0) * t) * 0.5;
  w[3] = (((t - 1.0) * t) * t) * 0.5;
}

__device__ __forceinline__ double line(const double (&w)[4], double q0, double q1, double q2, double q3)
{
  return ((w[0] * q0 + w[1] * q1) + w[2] * q2) + w[3] * q3;
}

// Cholesky of the m x m matrix in H (rows of 12), in place in the lower triangle; false when a pivot is not positive
__device__ bool factor(double* H, int m)
{
  for (int j = 0; j < m; ++j) {
    for (int k = 0; k < j; ++k) {
      double v = H[j * 12 + k];
      for (int q = 0; q < k; ++q) v -= H[j * 12 + q] * H[k * 12 + q];
      H[j * 12 + k] = v / H[k * 12 + k];
    }
    double d = H[j * 12 + j];
    for (int q = 0; q < j; ++q) d -= H[j * 12 + q] * H[j * 12 + q];
    if (!(d > 0.0)) return false;
    H[j * 12 + j] = sqrt(d);
  }
  return true;
}

// dp = -H^-1 rhs into x (12 parameters in the order of p; the gradient increments of the translation model are +0)
__device__ void solve(const double* L, int m, const double* rhs, double* y, double* dp)
{
  for (int j = 0; j < m; ++j) {
    double v = rhs[j];
    for (int q = 0; q < j; ++q) v -= L[j * 12 + q] * y[q];
    y[j] = v / L[j * 12 + j];
  }
  for (int j = m - 1; j >= 0; --j) {
    double v = y[j];
    for (int q = j + 1; q < m; ++q) v -= L[q * 12 + j] * y[q];
    y[j] = v / L[j * 12 + j];
  }
  for (int k = 0; k < 12; ++k) dp[k] = 0.0;
  if (m == 3) {
    for (int c = 0; c < 3; ++c) dp[4 * c] = -y[c];
  } else {
    for (int k = 0; k < 12; ++k) dp[k] = -y[k];
  }
}

// p <- p o dp^-1 (the header's update); false when the determinant is 0
__device__ bool compose(double* p, const double* dp)
{
  double A[3][3], B[3][3], C[3][3], V[3][3], N[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      A[r][c] = (r == c ? 1.0 : 0.0) + p[4 * r + 1 + c];
      B[r][c] = (r == c ? 1.0 : 0.0) + dp[4 * r + 1 + c];
    }
  C[0][0] = B[1][1] * B[2][2] - B[1][2] * B[2][1];
  C[0][1] = B[0][2] * B[2][1] - B[0][1] * B[2][2];
  C[0][2] = B[0][1] * B[1][2] - B[0][2] * B[1][1];
  C[1][0] = B[1][2] * B[2][0] - B[1][0] * B[2][2];
  C[1][1] = B[0][0] * B[2][2] - B[0][2] * B[2][0];
  C[1][2] = B[0][2] * B[1][0] - B[0][0] * B[1][2];
  C[2][0] = B[1][0] * B[2][1] - B[1][1] * B[2][0];
  C[2][1] = B[0][1] * B[2][0] - B[0][0] * B[2][1];
  C[2][2] = B[0][0] * B[1][1] - B[0][1] * B[1][0];
  const double det = (B[0][0] * C[0][0] + B[0][1] * C[1][0]) + B[0][2] * C[2][0];
  if (det == 0.0) return false;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = C[r][c] / det;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) N[r][c] = (A[r][0] * V[0][c] + A[r][1] * V[1][c]) + A[r][2] * V[2][c];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    p[4 * r] = p[4 * r] - ((N[r][0] * dp[0] + N[r][1] * dp[4]) + N[r][2] * dp[8]);
#pragma unroll
    for (int c = 0; c < 3; ++c) p[4 * r + 1 + c] = N[r][c] - (r == c ? 1.0 : 0.0);
  }
  return true;
}

// every store to `records` is a vector store by the lane that owns the words
template <int M>
__global__ __launch_bounds__(kLanes) void k_subset_match(const float* __restrict__ a, const float* __restrict__ b, F3dGeo g, SubsetArgs s,
                                                         const double* __restrict__ start, double* __restrict__ records)
{
  extern __shared__ double lds[];  // g_i (n binary64), then the region of a (region^3 float32)
  __shared__ double red[kChunk * kLanes];
  __shared__ double Hs[144];
  __shared__ double ps[12], dps[12], rhs[12], ys[12];
  __shared__ double outs[4];  // zncc, step, df, dg
  __shared__ int state[2];    // status (-1: go on), iterations
  double* gs = lds;
  float* region = reinterpret_cast<float*>(lds + s.n);
  const int tid = threadIdx.x;
  const int node = blockIdx.x;
  const f3d_subset_match_grid& q = s.grid;
  const int W = q.window, side = s.side, R = s.region, n = s.n;
  const int cx = q.ox + (node % q.nx) * q.step;
  const int cy = q.oy + ((node / q.nx) % q.ny) * q.step;
  const int cz = q.oz + (node / (q.nx * q.ny)) * q.step;
  double* rec = records + static_cast<size_t>(node) * kRecordDoubles;

  double u0 = 0.0, v0 = 0.0, w0 = 0.0;  // the start translation
  bool no_start = false;
  if (start) {
    const double* mine = start + static_cast<size_t>(node) * 12;
    u0 = mine[0];
    v0 = mine[4];
    w0 = mine[8];
#pragma unroll
    for (int k = 0; k < 12; ++k) no_start |= mine[k] != mine[k];
  }
  if (tid < 12) ps[tid] = start ? start[static_cast<size_t>(node) * 12 + tid] : 0.0;
  if (tid < 4) outs[tid] = 0.0;
  if (tid == 0) {
    state[0] = -1;
    state[1] = 0;
  }
  int nans = 0;
  double fm = 0.0, df = 0.0;
  int status = no_start ? F3D_SUBSET_NO_START : -1;  // the same in every lane from here on

  if (status < 0) {
    // the region of a: inside the box (the entry has checked it)
    for (int i = tid; i < R * R * R; i += kLanes) {
      const int rx = i % R, ry = (i / R) % R, rz = i / (R * R);
      region[i] = a[f3d_row(g, cy - W - 1 + ry, cz - W - 1 + rz) + static_cast<size_t>(cx - W - 1 + rx)];
    }
    __syncthreads();
    double v[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += kLanes) {
      const double f = window_value(region, R, voxel_of(i, side));
      v[0] += f;
      v[1] += f != f ? 1.0 : 0.0;
    }
    block_sum(v, red, tid);
    nans = static_cast<int>(v[1]);
    if (nans > 0) {
      status = F3D_SUBSET_NAN;
    } else {
      fm = v[0] / static_cast<double>(n);
      double w[1] = {0.0};
      for (int i = tid; i < n; i += kLanes) {
        const double F = window_value(region, R, voxel_of(i, side)) - fm;
        w[0] += F * F;
      }
      block_sum(w, red, tid);
      df = sqrt(w[0]);
      if (tid == 0) outs[2] = df;
      if (df == 0.0) status = F3D_SUBSET_FLAT;
    }
  }

  if (status < 0) {
    // the Hessian, a row at a time
    for (int r = 0; r < M; ++r) {
      double acc[M];
#pragma unroll
      for (int c = 0; c < M; ++c) acc[c] = 0.0;
      for (int i = tid; i < n; i += kLanes) {
        double J[M];
        const Voxel e = voxel_of(i, side);
        jacobian<M>(region, R, W, e, J);
        const double Jr = pick<M>(J, r, static_cast<double>(e.ex - W), static_cast<double>(e.ey - W), static_cast<double>(e.ez - W));
#pragma unroll
        for (int c = 0; c < M; ++c) acc[c] += Jr * J[c];
      }
      block_sum(acc, red, tid);
      if (tid == 0) {
#pragma unroll
        for (int c = 0; c < M; ++c) Hs[r * 12 + c] = acc[c];
      }
    }
    __syncthreads();
    if (tid == 0 && !factor(Hs, M)) state[0] = F3D_SUBSET_SINGULAR;
    __syncthreads();
    status = state[0];
  }

  while (status < 0) {
    double p[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) p[k] = ps[k];
    if (tid == 0) state[1] += 1;
    // g_i at the mapped points
    double v[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += kLanes) {
      const Voxel e = voxel_of(i, side);
      const double xx = static_cast<double>(e.ex - W), xy = static_cast<double>(e.ey - W), xz = static_cast<double>(e.ez - W);
      const double x = static_cast<double>(cx + e.ex - W) + (((p[0] + p[1] * xx) + p[2] * xy) + p[3] * xz);
      const double y = static_cast<double>(cy + e.ey - W) + (((p[4] + p[5] * xx) + p[6] * xy) + p[7] * xz);
      const double z = static_cast<double>(cz + e.ez - W) + (((p[8] + p[9] * xx) + p[10] * xy) + p[11] * xz);
      const double bx = floor(x), by = floor(y), bz = floor(z);
      const bool in = bx >= 1.0 && bx <= static_cast<double>(g.W - 3) && by >= 1.0 && by <= static_cast<double>(g.H - 3) && bz >= 1.0 &&
                      bz <= static_cast<double>(g.D - 3);
      if (!in) {
        v[1] += 1.0;
        continue;
      }
      double wx[4], wy[4], wz[4];
      cubic_weights(x - bx, wx);
      cubic_weights(y - by, wy);
      cubic_weights(z - bz, wz);
      const int ix = static_cast<int>(bx) - 1, iy = static_cast<int>(by) - 1, iz = static_cast<int>(bz) - 1;
      double planes[4];
#pragma unroll
      for (int kz = 0; kz < 4; ++kz) {
        double rows[4];
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
          const float* row = b + f3d_row(g, iy + ky, iz + kz) + static_cast<size_t>(ix);
          rows[ky] = line(wx, static_cast<double>(row[0]), static_cast<double>(row[1]), static_cast<double>(row[2]),
                          static_cast<double>(row[3]));
        }
        planes[kz] = line(wy, rows[0], rows[1], rows[2], rows[3]);
      }
      const double value = line(wz, planes[0], planes[1], planes[2], planes[3]);
      gs[i] = value;
      v[0] += value;
    }
    block_sum(v, red, tid);
    if (v[1] > 0.0) {
      status = F3D_SUBSET_OUTSIDE;
      break;
    }
    if (v[0] != v[0]) {
      status = F3D_SUBSET_NAN;
      break;
    }
    const double gm = v[0] / static_cast<double>(n);
    double w[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += kLanes) {
      const double F = window_value(region, R, voxel_of(i, side)) - fm;
      const double G = gs[i] - gm;
      w[0] += G * G;
      w[1] += F * G;
    }
    block_sum(w, red, tid);
    const double dg = sqrt(w[0]);
    if (tid == 0) outs[3] = dg;
    if (dg == 0.0) {
      status = F3D_SUBSET_FLAT_TARGET;
      break;
    }
    if (tid == 0) outs[0] = w[1] / (df * dg);
    const double ratio = df / dg;
    double acc[M];
#pragma unroll
    for (int c = 0; c < M; ++c) acc[c] = 0.0;
    for (int i = tid; i < n; i += kLanes) {
      const Voxel e = voxel_of(i, side);
      double J[M];
      jacobian<M>(region, R, W, e, J);
      const double F = window_value(region, R, e) - fm;
      const double G = gs[i] - gm;
      const double res = F - ratio * G;
#pragma unroll
      for (int c = 0; c < M; ++c) acc[c] += J[c] * res;
    }
    block_sum(acc, red, tid);
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < M; ++c) rhs[c] = acc[c];
      solve(Hs, M, rhs, ys, dps);
      if (!compose(ps, dps)) {
        state[0] = F3D_SUBSET_SINGULAR;
      } else {
        double grads = 0.0;
        for (int k = 0; k < 12; ++k)
          if (k % 4) grads += dps[k] * dps[k];
        const double ww = static_cast<double>(W) * static_cast<double>(W);
        const double step = sqrt(((dps[0] * dps[0] + dps[4] * dps[4]) + dps[8] * dps[8]) + ww * grads);
        outs[1] = step;
        const double du = ps[0] - u0, dv = ps[4] - v0, dw = ps[8] - w0;
        if (step < s.tolerance)
          state[0] = F3D_SUBSET_OK;
        else if (sqrt((du * du + dv * dv) + dw * dw) > s.reach)
          state[0] = F3D_SUBSET_LOST;
        else if (state[1] == s.max_iterations)
          state[0] = F3D_SUBSET_NOT_CONVERGED;
      }
    }
    __syncthreads();
    status = state[0];
  }

  __syncthreads();
  if (tid < 12) rec[tid] = ps[tid];
  else if (tid < 16) rec[tid] = outs[tid - 12];
  if (tid == 0) {
    int* tail = reinterpret_cast<int*>(rec + 16);
    tail[0] = status;
    tail[1] = state[1];
    tail[2] = nans;
    tail[3] = 0;
  }
}

}  // namespace

extern "C" {

int f3d_subset_match(f3d_devptr a, f3d_devptr b, size_t width, size_t height, size_t depth, const f3d_subset_match_grid* grid, int model,
                     const double* start, int max_iterations, double tolerance, double reach, f3d_subset_match_record* records,
                     f3d_subset_match_info* info)
{
  F3D_REQUIRE_READY("f3d_subset_match");
  if (!a || !b || !grid || !records) return f3d::fail("f3d_subset_match: null argument");
  if (model != F3D_SUBSET_TRANSLATION && model != F3D_SUBSET_AFFINE) return f3d::fail("f3d_subset_match: unknown model %d", model);
  const f3d_subset_match_grid& q = *grid;
  if (q.step < 1) return f3d::fail("f3d_subset_match: the step must be at least 1");
  if (q.nx < 1 || q.ny < 1 || q.nz < 1) return f3d::fail("f3d_subset_match: the grid is empty");
  const unsigned long long count = static_cast<unsigned long long>(q.nx) * q.ny * q.nz;
  if (count > F3D_SUBSET_MATCH_MAX_NODES) return f3d::fail("f3d_subset_match: more than 2^22 nodes");
  if (q.window < 1 || q.window > F3D_SUBSET_MATCH_MAX_WINDOW) return f3d::fail("f3d_subset_match: the half-window must be 1 .. 8");
  if (max_iterations < 1 || max_iterations > F3D_SUBSET_MATCH_MAX_ITERATIONS)
    return f3d::fail("f3d_subset_match: max_iterations must be 1 .. 64");
  if (!(tolerance > 0.0)) return f3d::fail("f3d_subset_match: the tolerance must be above 0");
  if (!(reach > 0.0)) return f3d::fail("f3d_subset_match: the reach must be above 0");
  F3dGeo g;
  if (!f3d::make_geo(&g, width, height, depth, nullptr, "f3d_subset_match")) return 1;
  const long long first[3] = {q.ox, q.oy, q.oz}, counts[3] = {q.nx, q.ny, q.nz}, dims[3] = {g.W, g.H, g.D};
  for (int axis = 0; axis < 3; ++axis)
    if (first[axis] - q.window - 1 < 0 || first[axis] + (counts[axis] - 1) * q.step + q.window + 1 > dims[axis] - 1)
      return f3d::fail("f3d_subset_match: the window of a node and a voxel round it leave the box along %c", "xyz"[axis]);

  SubsetArgs s;
  s.grid = q;
  s.side = 2 * q.window + 1;
  s.region = 2 * q.window + 3;
  s.n = s.side * s.side * s.side;
  s.max_iterations = max_iterations;
  s.tolerance = tolerance;
  s.reach = reach;
  const size_t lds_bytes = static_cast<size_t>(s.n) * sizeof(double) + static_cast<size_t>(s.region) * s.region * s.region * sizeof(float);

  const size_t record_bytes = count * sizeof(f3d_subset_match_record), start_bytes = start ? count * 12 * sizeof(double) : 0;
  void* d_buf = nullptr;
  if (f3d::scratch_buffer(record_bytes + start_bytes, &d_buf)) return 1;
  double* d_records = static_cast<double*>(d_buf);
  double* d_start = start ? d_records + count * kRecordDoubles : nullptr;
  if (start) F3D_HIP(hipMemcpyAsync(d_start, start, start_bytes, hipMemcpyHostToDevice, f3d::stream()));
  const float* pa = f3d_ptr<const float>(a);
  const float* pb = f3d_ptr<const float>(b);
  const int nodes = static_cast<int>(count);
  if (model == F3D_SUBSET_AFFINE) {
    F3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_subset_match<12>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(lds_bytes)));
    hipLaunchKernelGGL(k_subset_match<12>, dim3(nodes), dim3(kLanes), lds_bytes, f3d::stream(), pa, pb, g, s, d_start, d_records);
  } else {
    F3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_subset_match<3>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(lds_bytes)));
    hipLaunchKernelGGL(k_subset_match<3>, dim3(nodes), dim3(kLanes), lds_bytes, f3d::stream(), pa, pb, g, s, d_start, d_records);
  }
  F3D_HIP(hipGetLastError());
  // into memory of the library's first: a call that fails on the way leaves the caller's records as they were
  f3d_subset_match_record* held = static_cast<f3d_subset_match_record*>(std::malloc(record_bytes));
  if (!held) return f3d::fail("f3d_subset_match: no host memory for %llu records", count);
  hipError_t e = hipMemcpyAsync(held, d_records, record_bytes, hipMemcpyDeviceToHost, f3d::stream());
  if (e == hipSuccess) e = hipStreamSynchronize(f3d::stream());
  if (e != hipSuccess) {
    std::free(held);
    return f3d::hip_fail(e, "f3d_subset_match: reading the records", __FILE__, __LINE__);
  }
  __builtin_memcpy(records, held, record_bytes);
  std::free(held);
  if (info) {
    f3d_subset_match_info t = {};
    t.nodes = count;
    for (unsigned long long i = 0; i < count; ++i) {
      const f3d_subset_match_record& r = records[i];
      if (r.status >= 0 && r.status < F3D_SUBSET_STATUS_COUNT) t.status[r.status] += 1;
      t.iterations += static_cast<unsigned long long>(r.iterations);
      t.nan += static_cast<unsigned long long>(r.nan);
    }
    *info = t;
  }
  return 0;
}

}  // extern "C"
