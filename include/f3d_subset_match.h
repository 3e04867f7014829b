/*
 * f3d_subset_match.h -- the device entry of subset correlation (local DVC): on a grid of nodes, the displacement and
 * the displacement gradient that carry a (2W+1)^3 subset of frame 0 onto frame 1, found by inverse-compositional Gauss-Newton on
 * the zero-normalised sum of squared differences, with the correlation coefficient it ends at.  Part of the C ABI of libf3d_hip.so;
 * the conventions are those of f3d.h, which this header includes (f3d.h does not include it, as it does not include
 * f3d_block_match.h: the tests that pin the declarations of both stay as they are).
 */
#ifndef F3D_SUBSET_MATCH_H_
#define F3D_SUBSET_MATCH_H_

#include "f3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define F3D_SUBSET_MATCH_MAX_WINDOW 8      /* the largest half-window */
#define F3D_SUBSET_MATCH_MAX_ITERATIONS 64
#define F3D_SUBSET_MATCH_MAX_NODES (1u << 22)
#define F3D_SUBSET_MATCH_LANES 256         /* of the partition of a window's voxels, see "Sums" below */

/* the shape function */
#define F3D_SUBSET_TRANSLATION 0 /* 3 parameters: u, v, w */
#define F3D_SUBSET_AFFINE 1      /* 12 parameters */

/* status of a node's record, tried in the order of the rule below */
#define F3D_SUBSET_OK 0
#define F3D_SUBSET_NAN 1           /* a NaN in the window of a, or in a value of b that was read */
#define F3D_SUBSET_FLAT 2          /* the window of a is constant */
#define F3D_SUBSET_FLAT_TARGET 3   /* the mapped window of b is constant */
#define F3D_SUBSET_SINGULAR 4      /* a pivot of the Hessian is not positive, or the determinant of an update is 0 */
#define F3D_SUBSET_OUTSIDE 5       /* a tap of a mapped point lies outside the box */
#define F3D_SUBSET_LOST 6          /* the translation is farther than `reach` from its start */
#define F3D_SUBSET_NOT_CONVERGED 7 /* max_iterations updates, the last step not below the tolerance */
#define F3D_SUBSET_NO_START 8      /* a NaN in the node's start */
#define F3D_SUBSET_STATUS_COUNT 9

/* Node (i, j, k), i fastest, has its centre c at (ox + i step, oy + j step, oz + k step). */
typedef struct f3d_subset_match_grid {
  int ox, oy, oz;
  int step;       /* >= 1 */
  int nx, ny, nz; /* >= 1, nx ny nz <= F3D_SUBSET_MATCH_MAX_NODES */
  int window;     /* half-window W, 1 .. 8; every node needs W + 1 voxels to each face of the box */
} f3d_subset_match_grid;

/* The record of one node, 144 bytes.  p = (u, ux, uy, uz, v, vx, vy, vz, w, wx, wy, wz): the window voxel at offset xi in [-W, W]^3
 * from c maps to c + xi + (u + ux xi_x + uy xi_y + uz xi_z, ...).
 *
 * The rule.  Everything after the float32 loads is binary64, every operation rounded on its own, no contraction; the sums are taken
 * as "Sums" says.  n = (2W+1)^3, window voxel i = ((xi_z + W)(2W+1) + (xi_y + W))(2W+1) + (xi_x + W).
 *   start:   p = the node's 12 start values (all zero without `start`); a NaN among them: NO_START, p is the start, all else 0.
 *   window:  f_i = a(c + xi_i); nan = the NaN among them; nan > 0: NAN.  fm = (sum f_i) / n, F_i = f_i - fm, df = sqrt(sum F_i F_i);
 *            df == 0: FLAT.
 *   Hessian: fx_i = (a(c + xi_i + ex) - a(c + xi_i - ex)) * 0.5, fy_i and fz_i alike;  J_i = (fx, fx xi_x, fx xi_y, fx xi_z, fy,
 *            fy xi_x, ..., fz xi_z) for AFFINE (m = 12), (fx, fy, fz) for TRANSLATION (m = 3);  H[r][c] = sum J_i[r] J_i[c].
 *            Cholesky, row by row: L[j][k] = (H[j][k] - L[j][0] L[k][0] - ... - L[j][k-1] L[k][k-1]) / L[k][k] for k < j, the
 *            products subtracted one at a time in this order; d = H[j][j] - L[j][0]^2 - ... - L[j][j-1]^2; not d > 0: SINGULAR;
 *            L[j][j] = sqrt(d).
 *   then, for iteration = 1, 2, ...:
 *     point: x_i = (double)(c_x + xi_x) + (((u + ux xi_x) + uy xi_y) + uz xi_z), y_i and z_i alike;  bx = floor(x_i), t = x_i - bx.
 *            Unless 1 <= bx <= width - 3 (the taps bx - 1 .. bx + 2 inside the box; a NaN fails) and alike in y and z for every
 *            i: OUTSIDE.
 *     g_i:   weights w0 = (((2 - t) t - 1) t) * 0.5, w1 = (((3 t - 5) t) t + 2) * 0.5, w2 = (((4 - 3 t) t + 1) t) * 0.5,
 *            w3 = (((t - 1) t) t) * 0.5;  a line of four values q is ((w0 q0 + w1 q1) + w2 q2) + w3 q3: the 16 lines of b along x
 *            with the weights of x, then 4 lines along y of those, then one along z.
 *            sum g_i is NaN: NAN.  gm = (sum g_i) / n, G_i = g_i - gm, dg = sqrt(sum G_i G_i); dg == 0: FLAT_TARGET.
 *            zncc = (sum F_i G_i) / (df * dg).
 *     step:  q = df / dg, r_i = F_i - q G_i, rhs[k] = sum J_i[k] r_i;  L y = rhs forward (y[j] = (rhs[j] - L[j][0] y[0] - ... ) /
 *            L[j][j]), L^T x = y backward (x[j] = (y[j] - L[j+1][j] x[j+1] - ... - L[m-1][j] x[m-1]) / L[j][j]), dp = -x (the nine
 *            gradient increments of TRANSLATION are +0).
 *     update (inverse compositional): A = I + the gradient of p, t = (u, v, w); B = I + the gradient of dp, s = its translation.
 *            C = the cofactors of B (C[0][0] = B11 B22 - B12 B21, C[0][1] = B02 B21 - B01 B22, C[0][2] = B01 B12 - B02 B11,
 *            C[1][0] = B12 B20 - B10 B22, C[1][1] = B00 B22 - B02 B20, C[1][2] = B02 B10 - B00 B12, C[2][0] = B10 B21 - B11 B20,
 *            C[2][1] = B01 B20 - B00 B21, C[2][2] = B00 B11 - B01 B10), det = (B00 C00 + B01 C10) + B02 C20; det == 0: SINGULAR;
 *            V = C / det (each entry divided); A' = A V with A'[r][c] = (A[r][0] V[0][c] + A[r][1] V[1][c]) + A[r][2] V[2][c];
 *            t'[r] = t[r] - ((A'[r][0] s0 + A'[r][1] s1) + A'[r][2] s2);  p = (t', A' - I).
 *     stop:  step = sqrt(((du^2 + dv^2) + dw^2) + (W W) * (the squares of the nine gradient increments added in the order of p));
 *            step < tolerance: OK.  Else sqrt(((u - u0)^2 + (v - v0)^2) + (w - w0)^2) > reach, with 0 the start: LOST.  Else
 *            iteration == max_iterations: NOT_CONVERGED.
 * A record holds what was last computed: p; zncc, step, df, dg (0 until they are); iterations = the iterations begun.
 *
 * Sums.  Every sum over the window is taken like this, and that is part of the contract: lane l of 256 adds the terms of the
 * voxels i = l, l + 256, l + 512, ... in ascending i to +0; then for half = 128, 64, ..., 1 lane l < half adds the sum of lane
 * l + half to its own; the sum is lane 0's. */
typedef struct f3d_subset_match_record {
  double p[12];
  double zncc;
  double step;   /* the last step */
  double df, dg;
  int status;
  int iterations;
  int nan;       /* the NaN voxels of a in this node's window */
  int reserved;  /* 0 */
} f3d_subset_match_record;

typedef struct f3d_subset_match_info {
  unsigned long long nodes;
  unsigned long long status[F3D_SUBSET_STATUS_COUNT]; /* nodes per status: they add up to nodes */
  unsigned long long iterations;                      /* over all nodes */
  unsigned long long nan;                             /* NaN voxels of a, every window counted separately */
} f3d_subset_match_info;

/* a, b: float32 containers of the current geometry holding frame 0 and frame 1 over the box width x height x depth.  start
 * (nullable: all zero): 12 binary64 per node in host memory, in the order of p.  records: nx ny nz records in host memory.  info:
 * nullable.  Whole volume, library stream; the call waits for the stream.  Padding outside the box is never read.  The same
 * arguments give the same bytes whatever the schedule.  Refused, with nothing written: a null a, b, grid or records; a model that is
 * neither; step, counts or window out of range; more than 2^22 nodes; max_iterations outside 1 .. 64; a tolerance or a reach that is
 * not > 0 (a NaN is not); a node whose window + 1 leaves the box; a zero dimension or a box beyond the container. */
int f3d_subset_match(f3d_devptr a, f3d_devptr b, size_t width, size_t height, size_t depth, const f3d_subset_match_grid* grid,
                     int model, const double* start, int max_iterations, double tolerance, double reach,
                     f3d_subset_match_record* records, f3d_subset_match_info* info);

#ifdef __cplusplus
}
#endif
#endif /* F3D_SUBSET_MATCH_H_ */
