// The cyclic Jacobi diagonalisation of a symmetric 3 x 3 tensor that f3d_principal_strain (f3d_principal.hip) and
// f3d_polar_decomposition (f3d_polar.hip) both run on the Green-Lagrange tensor: the rotation of one pair and the five sweeps of
// include/f3d.h, f3d_principal_strain, rule 2.  Per-lane vector arithmetic on the six entries of A and, when DIRS, the nine of V;
// everything here is inlined into its kernel, so both compile the same text.
#ifndef F3D_JACOBI3_H_
#define F3D_JACOBI3_H_
#include "f3d_internal.h"

namespace f3d_jacobi3 {

constexpr int kSweeps = 5;

// include/f3d.h, f3d_principal_strain, rule 2: the rotation of the pair (p, q) with r the third index; vp / vq: columns p and q of V
template <bool DIRS>
__device__ __forceinline__ void rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float (&vp)[3], float (&vq)[3])
{
  if (apq == 0.f) return;
  const float theta = (aqq - app) / (2.f * apq);
  float t = 1.f / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  if (theta < 0.f) t = -t;
  const float c = 1.f / sqrtf(t * t + 1.f);
  const float s = t * c;
  const float h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.f;
  const float rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  if (DIRS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float kp = vp[k], kq = vq[k];
      vp[k] = c * kp - s * kq;
      vq[k] = s * kp + c * kq;
    }
  }
}

// the five sweeps over the pairs (0, 1), (0, 2), (1, 2); v0, v1, v2: the columns of V (untouched without DIRS).  Every lane of the
// wave calls it: a wave leaves the loop as soon as no lane has an off-diagonal left.
template <bool DIRS>
__device__ __forceinline__ void sweeps(float& a00, float& a11, float& a22, float& a01, float& a02, float& a12, float (&v0)[3],
                                       float (&v1)[3], float (&v2)[3])
{
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    // rule 2: a sweep over three zero off-diagonals is the identity, so once that holds in every lane the rest can go
    if (__ballot(a01 != 0.f || a02 != 0.f || a12 != 0.f) == 0) break;
    rotate<DIRS>(a00, a11, a01, a02, a12, v0, v1);  // (0, 1), r = 2
    rotate<DIRS>(a00, a22, a02, a01, a12, v0, v2);  // (0, 2), r = 1
    rotate<DIRS>(a11, a22, a12, a01, a02, v1, v2);  // (1, 2), r = 0
  }
}

}  // namespace f3d_jacobi3
#endif  // F3D_JACOBI3_H_
