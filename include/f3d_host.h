/*
 * f3d_host.h -- C ABI of libf3d_host.so: the C++ host side (driver + operator classes that mirror the
 * reference's src/optical_flow and src/cuda_operations/entire_data) exposed to other languages.
 * The Python package binds exactly these entry points with ctypes; nothing here carries torch or numpy types.
 *
 *   f3d_flow_*  : OpticalFlowE  (src/optical_flow/optical_flow_e.h:38-66; ComputeFlow optical_flow_e.cpp:132-601)
 *   f3d_op_*    : the six CudaOperation* classes through their string-keyed parameter bag
 *                 (src/cuda_operations/cuda_operation_base.h:40-46, keys in SURVEY.md 8b)
 *   host helpers: level schedule (optical_flow_base.cpp:31-56), Gaussian taps
 *                 (cuda_operation_convolution.cpp:85-108), RAW volume I/O (data3d.cpp:95-237),
 *                 the synthetic translated-Gaussian benchmark pair.
 * All functions return 0 on success unless stated otherwise.
 */
#ifndef F3D_HOST_H_
#define F3D_HOST_H_

#include "f3d.h"
#include "f3d_block_match.h"
#include "f3d_subset_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the 9-key driver bag of src/main.cpp:156-165 as a plain struct */
typedef struct f3d_flow_params {
  size_t warp_levels_count;
  float  warp_scale_factor;
  size_t outer_iterations_count;
  size_t inner_iterations_count;
  float  equation_alpha;
  float  equation_smoothness;
  float  equation_data;
  size_t median_radius;
  float  gaussian_sigma;
} f3d_flow_params;

typedef struct f3d_flow_s* f3d_flow;
typedef struct f3d_op_s* f3d_op;

/* defaults of src/main.cpp:77-85 */
void f3d_flow_default_params(f3d_flow_params* p);

/* Orderly end of device use (the reference's cuCtxDestroy at src/main.cpp:236 with what this library adds around it):
 * releases the out-of-core path's device arena, copy queues and events, destroys the RCCL communicator if one exists,
 * then f3d_shutdown().  Idempotent; every step is a no-op when there is nothing to release.  Drivers and operators that
 * are still alive must be destroyed BEFORE this call -- their containers are theirs to free.  Bindings call it from their
 * own exit hook (the Python package registers it with atexit at import) so that nothing depends on the order in which
 * the process tears libraries down. */
int f3d_host_shutdown(void);

int f3d_flow_create(f3d_flow* flow);
/* OpticalFlowE::Initialize: allocates the 15 containers and initialises the six operators */
int f3d_flow_initialize(f3d_flow flow, size_t width, size_t height, size_t depth);
/* OpticalFlowE::ComputeFlow on dense host volumes (x fastest); u, v, w receive width*height*depth floats */
int f3d_flow_compute(f3d_flow flow, const float* frame_0, const float* frame_1, const f3d_flow_params* params,
                     int silent, float* u, float* v, float* w);
/* device-resident variant: upload once, solve any number of times, download on demand */
int f3d_flow_upload(f3d_flow flow, const float* frame_0, const float* frame_1);
int f3d_flow_compute_resident(f3d_flow flow, const f3d_flow_params* params, int silent, float* device_seconds);
int f3d_flow_download(f3d_flow flow, float* u, float* v, float* w);
int f3d_flow_container(f3d_flow flow, f3d_size4* container);
/* Diagnostics (the reference's counterpart is the disabled block optical_flow_e.cpp:536-571 that registers
 * frame_1 with the final flow and dumps the volume).  With level statistics enabled every later compute records, per pyramid
 * level, the residual of frame_1 warped by the flow handed down from the coarser level against frame_0 (before the solve) and the
 * min / max / average flow magnitude after the level's median. */
typedef struct f3d_level_stat {
  int level;
  size_t width, height, depth;
  double residual_rms, residual_mean_abs;
  float residual_max_abs;
  float flow_min, flow_max, flow_avg;
} f3d_level_stat;
int f3d_flow_set_level_stats(f3d_flow flow, int enable);
int f3d_flow_level_stat_count(f3d_flow flow, size_t* count);
int f3d_flow_level_stat(f3d_flow flow, size_t index, f3d_level_stat* out);  /* index 0 = coarsest level of the last compute */
/* residual of the ORIGINAL frame_1 registered with the flow on the device (h = 1) against the original frame_0, and of the pair
 * as it stands; values: rms, mean |.|, max |.| each.  Needs f3d_flow_upload + f3d_flow_compute_resident. */
int f3d_flow_final_residual(f3d_flow flow, double registered[3], double unregistered[3]);
/* Trajectory of a frame sequence (the displacement of every voxel of frame 0 to the frame the sequence has reached: frame 0's grid,
 * voxel units; f3d_compose_flow of include/f3d.h is the step).  Per pair: f3d_flow_upload + f3d_flow_compute_resident, then
 * f3d_flow_trajectory_append composes the flow the driver holds into the trajectory on the device.  f3d_flow_compute releases its
 * result, so it is no source.
 *   begin     allocates three containers on first use (fails when they do not fit), then sets the trajectory to zero
 *   append    an error before begin or when no flow is held; enqueues and returns
 *   download  u, v, w receive width*height*depth floats; lost (nullable) the number of voxels whose u is NaN (left the volume)
 *   end       frees the three containers (f3d_flow_destroy does too)
 * A device library without f3d_compose_flow still loads; then every call fails.  Failures of these calls are described by
 * f3d_host_last_error(). */
int f3d_flow_trajectory_begin(f3d_flow flow);
int f3d_flow_trajectory_append(f3d_flow flow);
int f3d_flow_trajectory_download(f3d_flow flow, float* u, float* v, float* w, unsigned long long* lost);
int f3d_flow_trajectory_end(f3d_flow flow);
/* Strain fields (f3d_flow_strain of include/f3d.h has the definition): of the flow the driver holds (source F3D_STRAIN_OF_FLOW, after
 * f3d_flow_compute_resident) or of the trajectory (F3D_STRAIN_OF_TRAJECTORY, after f3d_flow_trajectory_begin).  fields selects groups
 * of the eight outputs vol, exx, eyy, ezz, exy, exz, eyz, eq (F3D_STRAIN_VOL / _E / _EQ); out[i] of a selected output receives
 * width*height*depth floats, the others are ignored; stats (nullable) the statistics.  Blocks until the fields are on the host.
 * The driver keeps a container per selected field until f3d_flow_strain_end (or f3d_flow_destroy).  A device library without
 * f3d_flow_strain still loads; then the call fails.  Failures are described by f3d_host_last_error(). */
#define F3D_STRAIN_OF_FLOW 0
#define F3D_STRAIN_OF_TRAJECTORY 1
int f3d_flow_strain_compute(f3d_flow flow, int source, unsigned fields, float* const out[8], f3d_strain_stats* stats);
int f3d_flow_strain_end(f3d_flow flow);

/* A solve started from a given displacement instead of zero (f3d_initial_flow of include/f3d.h prepares it: a voxel with a component
 * that is not finite becomes zero; info, nullable, says what was found).  The initial flow is data in three containers of the driver's
 * own, like the trajectory: it stays as it is until it is set again, f3d_flow_initial_end or f3d_flow_destroy, and only the two
 * *_from_initial calls read it -- f3d_flow_compute and f3d_flow_compute_resident never do.
 *   upload    from three host volumes of width * height * depth floats (a guess from outside: a coarse DVC, an FE prediction, a
 *             rigid pre-registration)
 *   take      a copy of the flow the driver holds (source F3D_STRAIN_OF_FLOW, after f3d_flow_compute_resident: the pair before
 *             under steady motion, or frame 0 -> frame k-1 for a direct solve frame 0 -> frame k) or of the trajectory
 *             (F3D_STRAIN_OF_TRAJECTORY, after f3d_flow_trajectory_begin)
 *   download  the prepared flow (for tests)
 *   end       frees the three containers
 *   f3d_flow_compute_resident_from_initial / f3d_flow_compute_from_initial: their namesakes with the pyramid's first level started
 *             from the initial flow resampled to that level's size (copied when that level is the original size; values are not
 *             rescaled, a flow is in original voxels at every level); with no level at all the result is the prepared initial flow.
 *             The depth (warp_levels_count) has to cover the error of the guess, not the displacement.
 * A device library without f3d_initial_flow still loads; then upload and take fail with a message naming it, and the compute calls
 * fail because no initial flow is held.  Failures are described by f3d_host_last_error(). */
int f3d_flow_initial_upload(f3d_flow flow, const float* u, const float* v, const float* w, f3d_initial_info* info);
int f3d_flow_initial_take(f3d_flow flow, int source, f3d_initial_info* info);
int f3d_flow_initial_download(f3d_flow flow, float* u, float* v, float* w);
int f3d_flow_initial_end(f3d_flow flow);
int f3d_flow_compute_resident_from_initial(f3d_flow flow, const f3d_flow_params* params, int silent, float* device_seconds);
int f3d_flow_compute_from_initial(f3d_flow flow, const float* frame_0, const float* frame_1, const f3d_flow_params* params, int silent,
                                  float* u, float* v, float* w);

/* Strain fields over a strain window (f3d_window_strain of include/f3d.h has the definition) of the same two sources,
 * F3D_STRAIN_OF_FLOW or F3D_STRAIN_OF_TRAJECTORY.  fields selects groups of the seventeen outputs vol, exx, eyy, ezz, exy, exz, eyz, eq,
 * G00 .. G22 (F3D_STRAIN_VOL / _E / _EQ, F3D_WSTRAIN_G); radius 1 .. 3; min_count 1 .. (2 radius + 1)^3.  Everything else as for
 * f3d_flow_strain_compute; the containers live until f3d_flow_window_strain_end (or f3d_flow_destroy). */
int f3d_flow_window_strain_compute(f3d_flow flow, int source, unsigned fields, unsigned radius, unsigned min_count,
                                   float* const out[17], f3d_window_strain_stats* stats);
int f3d_flow_window_strain_end(f3d_flow flow);

/* Principal strains (f3d_principal_strain of include/f3d.h has the definition) of the same two sources, F3D_STRAIN_OF_FLOW or
 * F3D_STRAIN_OF_TRAJECTORY.  fields selects groups of the ten outputs e1, e2, e3, gmax, d1x, d1y, d1z, d3x, d3y, d3z
 * (F3D_PRINCIPAL_VALUES / _SHEAR / _DIR1 / _DIR3); out[i] of a selected output receives width * height * depth floats, entries of
 * other outputs are ignored; stats is nullable.  The driver keeps a container per selected field until f3d_flow_principal_end (or
 * f3d_flow_destroy).  A device library without f3d_principal_strain still loads; then the call fails with a message naming it. */
int f3d_flow_principal_compute(f3d_flow flow, int source, unsigned fields, float* const out[10], f3d_principal_stats* stats);
int f3d_flow_principal_end(f3d_flow flow);

/* Local rotation and principal stretches (f3d_polar_decomposition of include/f3d.h has the definition) of the same two sources,
 * F3D_STRAIN_OF_FLOW or F3D_STRAIN_OF_TRAJECTORY.  fields selects groups of the seven outputs theta, rx, ry, rz, l1, l2, l3
 * (F3D_POLAR_ANGLE / _VECTOR / _STRETCH); out[i] of a selected output receives width * height * depth floats, entries of other
 * outputs are ignored; stats is nullable.  The driver keeps a container per selected field until f3d_flow_polar_end (or
 * f3d_flow_destroy).  A device library without f3d_polar_decomposition still loads; then the call fails with a message naming it. */
int f3d_flow_polar_compute(f3d_flow flow, int source, unsigned fields, float* const out[7], f3d_polar_stats* stats);
int f3d_flow_polar_end(f3d_flow flow);

/* Principal strains, and local rotation and principal stretches, of the least-squares gradient over a strain window: per call
 * f3d_window_strain's F3D_WSTRAIN_G group into nine containers the driver keeps to itself, then f3d_principal_from_gradient /
 * f3d_polar_from_gradient on them (include/f3d.h has the definitions), of the same two sources.  fields, out and stats as for
 * f3d_flow_principal_compute / f3d_flow_polar_compute, radius and min_count as for f3d_flow_window_strain_compute.  A call depends on
 * its arguments only: it needs no earlier f3d_flow_window_strain_compute and leaves what that holds as it is.  The output containers
 * live until the kind's _end (or f3d_flow_destroy); the gradient's nine are freed when both kinds have ended.  A device library
 * without f3d_principal_from_gradient / f3d_polar_from_gradient still loads; then the call fails with a message naming it. */
int f3d_flow_window_principal_compute(f3d_flow flow, int source, unsigned fields, unsigned radius, unsigned min_count,
                                      float* const out[10], f3d_principal_stats* stats);
int f3d_flow_window_principal_end(f3d_flow flow);
int f3d_flow_window_polar_compute(f3d_flow flow, int source, unsigned fields, unsigned radius, unsigned min_count, float* const out[7],
                                  f3d_polar_stats* stats);
int f3d_flow_window_polar_end(f3d_flow flow);

/* Inverse displacement (f3d_invert_displacement of include/f3d.h has the definition) of the same two sources, F3D_STRAIN_OF_FLOW or
 * F3D_STRAIN_OF_TRAJECTORY: out[0..3] = g_u, g_v, g_w, err receive width * height * depth floats each (all four required); stats is
 * nullable.  Blocks until the fields are on the host.  The driver keeps four containers until f3d_flow_inverse_end (or
 * f3d_flow_destroy).  A device library without f3d_invert_displacement still loads; then the call fails with a message naming it. */
int f3d_flow_inverse_compute(f3d_flow flow, int source, unsigned iterations, float tolerance, float* const out[4],
                             f3d_inverse_stats* stats);
int f3d_flow_inverse_end(f3d_flow flow);

/* Match quality (f3d_local_correlation of include/f3d.h has the definition) of the flow the driver holds and the frames it holds
 * (after f3d_flow_upload + f3d_flow_compute_resident): frame 1 is carried onto frame 0's grid through the flow (f3d_carry_field,
 * linear; NaN where the point leaves the volume) and compared with frame 0 over (2 radius + 1)^3 windows.  fields selects the three
 * outputs warped (the carried frame 1), zncc, rmsd (F3D_MATCH_WARPED / _ZNCC / _RMSD); out[i] of a selected output receives
 * width * height * depth floats, entries of other outputs are ignored; radius 1 .. 4; stats is nullable (below counts zncc <
 * threshold).  source must be F3D_STRAIN_OF_FLOW: frame 0 of a trajectory is not kept, so F3D_STRAIN_OF_TRAJECTORY is refused with a
 * message.  Blocks until the fields are on the host.  The driver keeps the warped container and one per selected field until
 * f3d_flow_match_end (or f3d_flow_destroy).  A device library without f3d_local_correlation still loads; then the call fails with a
 * message naming it. */
#define F3D_MATCH_WARPED 1u
#define F3D_MATCH_ZNCC 2u
#define F3D_MATCH_RMSD 4u
int f3d_flow_match_compute(f3d_flow flow, int source, unsigned fields, unsigned radius, float threshold, float* const out[3],
                           f3d_correlation_stats* stats);
int f3d_flow_match_end(f3d_flow flow);

/* The solve between f3d_motion_sums and f3d_remove_motion (include/f3d.h): the fit d ~ t + M X of a displacement from its moment sums,
 * X the coordinates about the centre the sums were taken about.  Host code, plain binary64, no device needed.  fit->centre is not
 * touched: the caller sets it to ((width-1)/2, (height-1)/2, (depth-1)/2).  t, M, n, rms_before, model, cos_angle and axial are
 * written (f3d_remove_motion of include/f3d.h says what they mean); no transcendental function enters any of them.
 *   F3D_MOTION_TRANSLATION  M = 0, t = Sd / n
 *   F3D_MOTION_AFFINE       the least-squares t, M from the normal equations [[n, Sx^T], [Sx, Sxx]] with the three right-hand sides
 *                           (Sd_j, Sxd_0j, Sxd_1j, Sxd_2j) by Cholesky.  An axis along which all present voxels have one coordinate
 *                           (n Sxx_aa == Sx_a^2, decided in the exact integers of doubled coordinates) is left out and its column of M
 *                           is 0; two such axes are refused (collinear).  A pivot that is not above 2^-40 of its diagonal entry is
 *                           refused: the present voxels are coplanar.
 *   F3D_MOTION_RIGID        Kabsch.  With xbar = Sx / n, dbar = Sd / n, Cxx = Sxx - n xbar xbar^T, Cxd = Sxd - n xbar dbar^T and
 *                           H = Cxx + Cxd, R is the rotation (determinant +1) of the singular value decomposition of H^T: a Jacobi
 *                           eigen-decomposition of H H^T carried out one-sidedly on the columns of H^T (rotations of column pairs
 *                           until they are orthogonal, so no singular value is squared), the third singular vectors by cross
 *                           products.  M = R - I, t = dbar - M xbar.  Refused with fewer than 3 voxels, and when the second singular
 *                           value is not above 2^-40 of the first (collinear; the floor f3d_local_correlation uses for "flat").
 * No present voxel (n == 0) is refused for every model, and so is an unknown model.  Returns non-zero with f3d_host_last_error() set
 * and the fit untouched when refused. */
int f3d_motion_solve(const struct f3d_motion_sums* sums, int model, f3d_motion_fit* fit);

/* The solve between f3d_label_motion_sums and f3d_remove_label_motion (include/f3d.h, which also defines F3D_LABEL_*): one fit per
 * label.  Host code, no device needed.  sums, fits and status have n_labels entries; label L is entry L-1.  status[L-1] is
 *   F3D_LABEL_EMPTY       when n == 0
 *   F3D_LABEL_SMALL       when n < min_voxels
 *   F3D_LABEL_DEGENERATE  when f3d_motion_solve of these sums (about the volume centre) refuses
 *   F3D_LABEL_OK          otherwise
 * An OK fit is then moved from the centre of the volume to the centroid of the label, so that t is the motion of the body itself and
 * not an extrapolation to the middle of the volume.  With xbar_a = Sx_a / n, in binary64, every operation rounded on its own, in
 * exactly this order:
 *   centre_a = volume_centre_a + xbar_a
 *   t_r      = t_r + ((M_r0 * xbar_0 + M_r1 * xbar_1) + M_r2 * xbar_2)
 * M and everything else f3d_motion_solve reports stay.  A label that is not OK gets a zeroed fit with n and model set.  Returns non-zero
 * (f3d_host_last_error() set, nothing written) only for an unknown model or a null pointer. */
int f3d_motion_solve_labels(const struct f3d_motion_sums* sums, size_t n_labels, int model, unsigned long long min_voxels,
                            const double volume_centre[3], f3d_motion_fit* fits, int* status);

/* Motion of the flow the driver holds or of the trajectory (source F3D_STRAIN_OF_FLOW / F3D_STRAIN_OF_TRAJECTORY): f3d_motion_sums on
 * the device, f3d_motion_solve, f3d_remove_motion into three containers the driver keeps until f3d_flow_motion_end (or
 * f3d_flow_destroy).  out[0..2] receive the residual u, v, w (width * height * depth floats each; all three required); fit receives the
 * fit with its centre (required); residual (nullable) the statistics of the residual.  min_zncc NaN: every voxel with a displacement
 * takes part.  Otherwise only voxels with zncc >= min_zncc in the zncc container of the last f3d_flow_match_compute, which must have
 * been computed of the same pair: the call fails with a message when there is none, and when source is the trajectory (that zncc
 * lives on the pair's grid).  A device library without f3d_motion_sums or f3d_remove_motion still loads; then the call fails with a
 * message naming the entry. */
int f3d_flow_motion_compute(f3d_flow flow, int source, int model, float min_zncc, float* const out[3], f3d_motion_fit* fit,
                            f3d_motion_residual* residual);
int f3d_flow_motion_end(f3d_flow flow);

/* Per-label motion of the flow the driver holds or of the trajectory (source F3D_STRAIN_OF_FLOW / F3D_STRAIN_OF_TRAJECTORY):
 * f3d_label_motion_sums on the device, f3d_motion_solve_labels, f3d_remove_label_motion into three containers the driver keeps until
 * f3d_flow_label_motion_end (or f3d_flow_destroy), and f3d_label_motion_sums of the residual.  labels: width * height * depth int32 on
 * the grid of the displacement (frame 0's for the trajectory), 0 background, 1 .. n_labels the bodies; they are uploaded into a
 * container the driver keeps, and a null labels reuses the ones uploaded by an earlier call.  out[0..2] receive the residual u, v, w
 * (all three required; NaN where a voxel's label has no fit); fits and status (n_labels entries each, required) what
 * f3d_motion_solve_labels writes; rms_after (nullable, n_labels entries) the rms of each label's residual, sqrt((Sdd_u + Sdd_v +
 * Sdd_w) / n) of the sums of the residual, NaN where the label has none; info (nullable) the voxel counts of the first sums.  A device
 * library without f3d_label_motion_sums or f3d_remove_label_motion still loads; then the call fails with a message naming the entry. */
int f3d_flow_label_motion_compute(f3d_flow flow, int source, const int* labels, size_t n_labels, int model, unsigned long long min_voxels,
                                  float* const out[3], f3d_motion_fit* fits, int* status, double* rms_after /* nullable */,
                                  f3d_label_info* info /* nullable */);
int f3d_flow_label_motion_end(f3d_flow flow);

/* Kinematics of the contacts f3d_label_contacts found (include/f3d.h): where each contact lies, how large it is, which way it faces,
 * and how far it opened and slid.  Host code, no device needed.  contacts and out have n entries; dims is (width, height, depth) of the
 * volume the contacts were found in; fits and status are what f3d_motion_solve_labels wrote for the same labels (n_labels entries
 * each), or both null.  Everything is binary64, only + - * / and sqrt, every operation rounded on its own, in exactly this order:
 *   T          = faces[0] + faces[1] + faces[2]                         (an integer)
 *   point_a    = 0.5 * (dims_a - 1) + c2_a / (2 * T)                    the mean face centre, in voxel coordinates
 *   area       = sqrt((A_0 * A_0 + A_1 * A_1) + A_2 * A_2)              A = the area vector as doubles (exact)
 *   normal_a   = A_a / area                                             from lo to hi
 *   jump_a     = (J_a * 2^-14) / n_jump                                 the mean displacement of hi minus that of lo across the faces
 *   for a vector d:  along = (d_0 * normal_0 + d_1 * normal_1) + d_2 * normal_2,   t_a = d_a - along * normal_a,
 *                    across = sqrt((t_0 * t_0 + t_1 * t_1) + t_2 * t_2)
 *   jump_normal, jump_slip = along, across of jump                      jump_normal > 0: the contact opened; < 0: it closed
 *   d_L(c)_r   = t_r + ((M_r0 * X + M_r1 * Y) + M_r2 * Z)               the fit of label L at c, X = c_0 - centre_L[0], Y, Z likewise
 *   delta_r    = d_hi(point)_r - d_lo(point)_r
 *   fit_normal, fit_slip = along, across of delta
 * status is a set of bits:
 *   F3D_CONTACT_SMALL     T < min_faces (everything is still computed)
 *   F3D_CONTACT_FLAT      the area vector is zero (a closed or folded patch): area is 0, normal and everything projected on it is NaN
 *   F3D_CONTACT_NOJUMP    n_jump == 0: jump_normal and jump_slip are NaN
 *   F3D_CONTACT_UNFITTED  fits or status is null, a label is outside 1 .. n_labels, or the status of lo or hi is not F3D_LABEL_OK:
 *                         fit_normal and fit_slip are NaN
 * Returns non-zero (f3d_host_last_error() set, nothing written) for a null contacts (with n > 0), dims or out, only one of fits and
 * status given, or a zero dimension. */
#define F3D_CONTACT_SMALL 1u
#define F3D_CONTACT_FLAT 2u
#define F3D_CONTACT_NOJUMP 4u
#define F3D_CONTACT_UNFITTED 8u
typedef struct f3d_contact_kin {
  double point[3], area, normal[3];
  double jump_normal, jump_slip, fit_normal, fit_slip;
  unsigned status;
} f3d_contact_kin;
int f3d_contact_kinematics(const struct f3d_contact* contacts, size_t n, const size_t dims[3], const f3d_motion_fit* fits /* nullable */,
                           const int* status /* nullable */, size_t n_labels, unsigned long long min_faces, f3d_contact_kin* out);

/* Contacts between the labels of a segmentation in the flow the driver holds or in the trajectory (source F3D_STRAIN_OF_FLOW /
 * F3D_STRAIN_OF_TRAJECTORY): f3d_label_contacts on the labels the driver keeps on the device, with a capacity that starts at
 * 8 * n_labels (at most 2^20) and doubles until the table is complete.  labels as in f3d_flow_label_motion_compute: uploaded when given, and a null
 * labels reuses the ones an earlier call (of this entry or of f3d_flow_label_motion_compute) uploaded.  *contacts receives a list of
 * *count entries sorted by (lo, hi) that the driver owns: it stays valid until the next call of this entry, f3d_flow_contacts_end or
 * f3d_flow_destroy.  info is required.  f3d_flow_contacts_end frees the list; the labels stay on the device until
 * f3d_flow_label_motion_end.  A device library without f3d_label_contacts still loads; then the call fails with a message naming it. */
int f3d_flow_contacts_compute(f3d_flow flow, int source, const int* labels /* nullable */, size_t n_labels,
                              const struct f3d_contact** contacts, size_t* count, f3d_contact_info* info);
int f3d_flow_contacts_end(f3d_flow flow);

/* The solve from the shape sums of f3d_label_shape_sums (include/f3d.h) to the shape table of the bodies.  Host code, no device
 * needed.  sums and out have n_labels entries; label L is entry L-1.  Coordinates are voxel indices, a voxel is a unit cube about its
 * index.  Binary64, every operation rounded on its own, in exactly this order (n, s1, s2, pairs, squares, cubes of the sums; N = (double)n):
 *   status        F3D_LABEL_EMPTY when n == 0: voxels 0, box_lo 0, box_hi -1, border, faces and euler 0, every double NaN.
 *                 F3D_LABEL_OK otherwise
 *   voxels, box_lo, box_hi, border   n, lo, hi, border as they are
 *   centroid_i    (double)s1_i / N
 *   diameter      cbrt(6.0 * N / pi): of the ball of the same volume
 *   C_ik          m_ik = n s2_ik - s1_i s1_k exactly in a 128-bit integer (below 2^93), (double)m_ik / (N * N), and + 1.0 / 12.0 on the
 *                 diagonal for the voxel's own extent: the covariance of the body as a union of unit cubes, without cancellation in
 *                 floating point
 *   l_1 >= l_2 >= l_3, axes   the eigenvalues and unit eigenvectors of C by cyclic Jacobi: 12 sweeps over the pairs (0,1) (0,2)
 *                 (1,2); for a pair (p, q) with C_pq != 0, theta = (C_qq - C_pp) / (2.0 * C_pq), t = sign(theta) / (|theta| +
 *                 sqrt(theta * theta + 1.0)) (sign(0) = +1), c = 1.0 / sqrt(t * t + 1.0), s = t * c, columns then rows p and q
 *                 of C become c * p - s * q and s * p + c * q, C_pq = C_qp = 0, and the columns of the accumulated rotation
 *                 likewise.  Sorted descending, equal values in column order.  axes[3 * i + a] is component a of axis i, divided
 *                 by its norm, its sign chosen so that its component of largest magnitude is positive (the first such on ties)
 *   semi_axes_i   sqrt(5.0 * l_i): the solid ellipsoid with the same second moments
 *   faces         sum over k = 0, 1, 2 of 2 (n - pairs[k]), an integer: the staircase area, the box border closing the body
 *   surface       2.0 * sum over k = 0 .. 12, in this order from 0.0, of w_k * (double)(2 (n - pairs[k])) / |d_k|: the Cauchy-Crofton
 *                 estimate over the 13 directions of f3d_label_shape_sums, |d_k| = 1.0, sqrt(2.0), sqrt(3.0), and w_k = 0.0915557824
 *                 (3 axes), 0.0739612557 (6 face diagonals), 0.0703912796 (4 body diagonals): the share of the unit sphere nearest
 *                 to +-d_k among the 26 directions
 *   sphericity    cbrt(pi * ((6.0 * N) * (6.0 * N))) / surface: 1 for a ball
 *   euler         n - (pairs[0] + pairs[1] + pairs[2]) + (squares[0] + squares[1] + squares[2]) - cubes: the Euler number of the body
 *                 under the six-connectivity of f3d_label_components: pieces - tunnels + cavities
 * Returns non-zero (f3d_host_last_error() set, nothing written) only for a null pointer. */
typedef struct f3d_label_shape {
  int status;
  unsigned long long voxels;
  long long box_lo[3], box_hi[3];
  unsigned long long border[3];
  double centroid[3], diameter, semi_axes[3], axes[9];
  unsigned long long faces;
  double surface, sphericity;
  long long euler;
} f3d_label_shape;
int f3d_label_shape_solve(const struct f3d_label_shape_sums* sums, size_t n_labels, f3d_label_shape* out);

/* The shapes of the labels the driver keeps on the device: f3d_label_shape_sums and f3d_label_shape_solve.  labels as in
 * f3d_flow_label_motion_compute: uploaded when given, and a null labels reuses the ones an earlier call uploaded or
 * f3d_flow_labels_compute / f3d_flow_labels_split made.  No displacement is needed, so this also runs before any solve.  shapes has
 * n_labels entries (required); info is nullable.  A device library without f3d_label_shape_sums still loads; then the call fails with
 * a message naming it. */
int f3d_flow_label_shapes_compute(f3d_flow flow, const int* labels /* nullable */, size_t n_labels, f3d_label_shape* shapes,
                                  f3d_label_shape_info* info /* nullable */);

/* The labels made on the device instead of uploaded: f3d_label_components (include/f3d.h has the definition of foreground, component,
 * root, the numbering and every counter) of a frame into the label container of the driver, the one f3d_flow_label_motion_compute and
 * f3d_flow_contacts_compute fill from their `labels` argument and reuse when that is null -- so a null labels and n_labels =
 * info->n_labels afterwards run on these bodies.  frame: a device container of the driver's geometry, or 0 for the resident frame 0 (the
 * raw frame 0 of the last f3d_flow_upload / f3d_flow_compute_resident, not a blurred copy).  *sizes receives a list of *count =
 * info->n_labels sizes (label L at index L - 1) that the driver owns: it stays valid until the next call of this entry,
 * f3d_flow_labels_end or f3d_flow_destroy.  info is required.  f3d_flow_labels_download copies the label container, however it was
 * filled, to width * height * depth int32.  f3d_flow_labels_end frees the list of sizes; the labels stay on the device until
 * f3d_flow_label_motion_end.  A device library without f3d_label_components still loads; then the call fails with a message naming it. */
int f3d_flow_labels_compute(f3d_flow flow, f3d_devptr frame /* 0: the resident frame 0 */, float lo, float hi, unsigned long long min_voxels,
                            const unsigned long long** sizes, size_t* count, f3d_component_info* info);
/* f3d_flow_labels_split: the same through f3d_split_components (include/f3d.h), which takes touching bodies apart at core_d2; same label
 * container, same list of sizes, and the same failure naming the entry when the device library has none. */
int f3d_flow_labels_split(f3d_flow flow, f3d_devptr frame /* 0: the resident frame 0 */, float lo, float hi, unsigned long long core_d2,
                          unsigned long long min_voxels, const unsigned long long** sizes, size_t* count, f3d_split_info* info);
int f3d_flow_labels_end(f3d_flow flow);
int f3d_flow_labels_download(f3d_flow flow, int* labels);

/* The solve from the overlap rows of f3d_label_overlap (include/f3d.h) to the tracks of the bodies: which body of B is which body of
 * A, which broke, which merged, which came and went.  Host code, no device needed.  rows are count rows with distinct keys (the sorted
 * list of f3d_label_overlap; the result does not depend on their order), n_ab is the n of the row (a, b).  a has n_a entries (body a at
 * index a - 1), b and map_b have n_b entries, summary is nullable.  min_fraction is in (0, 1]; "the share of p in q counts" means
 * (double)p >= min_fraction * (double)q in binary64 with that one multiplication.  Integers are exact; every double is formed as
 * written, every operation rounded on its own.  In exactly this order:
 *   1. per body a >= 1 of A, over its rows (a, b), b = -1, 0, 1 .. n_b:
 *        n = sum n_ab;  n_lost = n_(a,-1);  n_background = n_(a,0)
 *        best_b = the b >= 1 of largest n_ab > 0, ties to the smallest b, 0 when there is none;  n_best = that n_ab, else 0
 *        shift_j = (double)(cb2_j - ca2_j) / (2.0 * (double)n_best) of the row (a, best_b): the exact mean displacement of the part of
 *                  a that landed in best_b, rounded once.  NaN without a best_b
 *      per body b >= 1 of B, over its rows (a, b), a = 0 .. n_a:
 *        m = sum n_ab: the voxels of A's GRID that land in b -- not the voxel count of b in its own volume, which the rows do not hold
 *        n_unreached = n_(0,b);  best_a = the a >= 1 of largest n_ab > 0, ties to the smallest a, 0 when there is none;  n_best likewise
 *   2. n_targets of a = the number of b >= 1 whose n_ab's share of n counts;  n_sources of b = the number of a >= 1 whose n_ab's share
 *      of m counts
 *   3. a with n == 0: status F3D_TRACK_EMPTY alone, fraction, shift and iou NaN.  Otherwise
 *        fraction = (double)n_best / (double)n
 *        iou = (double)n_best / (double)(n + m_(best_b) - n_best), 0.0 without a best_b
 *        F3D_TRACK_MATCHED   best_b >= 1 and best_a of best_b is a (mutual best)
 *        F3D_TRACK_SPLIT     n_targets >= 2
 *        F3D_TRACK_VANISHED  n_targets == 0
 *        F3D_TRACK_LEFT      n_lost's share of n counts
 *      b with m == 0: status F3D_TRACK_EMPTY alone.  Otherwise F3D_TRACK_MATCHED (best_a >= 1 and best_b of best_a is b),
 *        F3D_TRACK_MERGED (n_sources >= 2), F3D_TRACK_APPEARED (n_sources == 0)
 *   4. map_b[b - 1]: a MATCHED b gets the number of its a; every other b that is not EMPTY gets n_a + 1, n_a + 2, ... in ascending b;
 *      an EMPTY b gets 0.  So the largest fragment of a broken body keeps the body's number and the others are new.
 * summary counts the bodies of A that are matched, split, vanished, left, those of B that are merged, appeared, and n_ids, the largest
 * number map_b hands out (n_a when none is new).
 * Returns non-zero (f3d_host_last_error() set, nothing written) for a null rows (with count > 0), a, b or map_b (with bodies to
 * write), n_a or n_b of 0, a min_fraction outside (0, 1] or NaN, and a row whose key is outside 0 .. n_a x -1 .. n_b or is (0, 0) or
 * (0, -1). */
#define F3D_TRACK_EMPTY 1u
#define F3D_TRACK_MATCHED 2u
#define F3D_TRACK_SPLIT 4u
#define F3D_TRACK_VANISHED 8u
#define F3D_TRACK_LEFT 16u
#define F3D_TRACK_MERGED 32u
#define F3D_TRACK_APPEARED 64u
typedef struct f3d_track_a {
  unsigned long long n, n_lost, n_background, n_best;
  int best_b, n_targets;
  double fraction, shift[3], iou;
  unsigned status;
} f3d_track_a;
typedef struct f3d_track_b {
  unsigned long long m, n_unreached, n_best;
  int best_a, n_sources;
  unsigned status;
} f3d_track_b;
typedef struct f3d_track_summary {
  unsigned long long matched, split, merged, vanished, appeared, left, n_ids;
} f3d_track_summary;
int f3d_overlap_solve(const struct f3d_overlap* rows, size_t count, size_t n_a, size_t n_b, double min_fraction, f3d_track_a* a,
                      f3d_track_b* b, int* map_b, f3d_track_summary* summary /* nullable */);

/* A second label volume, "B", beside the labels of the driver ("A", on frame 0's grid): the bodies of a later frame, on the grid a
 * displacement leads to.  It lives in a container of its own that goes with f3d_flow_label_motion_end or f3d_flow_destroy.
 *   f3d_flow_labels_b_upload    width * height * depth int32, 0 background, 1 .. n_b the bodies
 *   f3d_flow_labels_b_segment   f3d_label_components (core_d2 == 0) or f3d_split_components (core_d2 >= 1) of `frame` into B; frame 0
 *                               means the resident frame 1, the RAW later frame of the pair the driver holds.  *sizes receives a list of
 *                               *count = info->n_labels sizes that the driver owns until the next call of this entry,
 *                               f3d_flow_labels_end or f3d_flow_destroy.  info (required) is f3d_split_info; without a split only its first
 *                               eight fields, those of f3d_component_info, are written and the rest are 0
 *   f3d_flow_overlap_compute    f3d_label_overlap of A and B through the held flow or the trajectory (source F3D_STRAIN_OF_FLOW /
 *                               F3D_STRAIN_OF_TRAJECTORY), with a capacity that starts at 8 * (n_a + n_b) (at most 2^20) and doubles
 *                               until the table is complete.  *rows receives *count rows sorted by (a, b) that the driver owns until
 *                               the next call of this entry, f3d_flow_overlap_end or f3d_flow_destroy.  info is required
 *   f3d_flow_labels_b_relabel   f3d_relabel_labels of B in place with map (n_b entries), e.g. f3d_overlap_solve's map_b
 *   f3d_flow_labels_b_download  B to width * height * depth int32
 * A device library without the entry a call needs still loads; then the call fails with a message naming the entry. */
int f3d_flow_labels_b_upload(f3d_flow flow, const int* labels);
int f3d_flow_labels_b_segment(f3d_flow flow, f3d_devptr frame /* 0: the resident frame 1 */, float lo, float hi, unsigned long long core_d2,
                              unsigned long long min_voxels, const unsigned long long** sizes, size_t* count, f3d_split_info* info);
int f3d_flow_overlap_compute(f3d_flow flow, int source, size_t n_a, size_t n_b, const struct f3d_overlap** rows, size_t* count,
                             f3d_overlap_info* info);
int f3d_flow_overlap_end(f3d_flow flow);
int f3d_flow_labels_b_relabel(f3d_flow flow, const int* map, size_t n_b);
int f3d_flow_labels_b_download(f3d_flow flow, int* labels);

/* The solve from the rows and counts of f3d_label_field_sums (include/f3d.h) to the statistics of a scalar field per body.  Host code,
 * no device needed; shift, lo, hi and bins are those of the device call, counts is null iff bins == 0.  stats[L-1] of label L:
 *   status        F3D_LABEL_EMPTY when n == 0, else F3D_LABEL_SMALL when n < min_voxels, else F3D_LABEL_OK.  A SMALL label is filled
 *                 like an OK one
 *   n, below, above   copied from the row
 *   min, max      the floats of min_key and max_key as binary64; NaN for an EMPTY label, as is every double below
 *   mean          ldexp((double)iq / (double)n, -shift)
 *   variance      V = n * iqq - iq^2 (iqq = iqq_hi * 2^32 + iqq_lo) formed exactly in unsigned __int128 -- below 2^111, never
 *                 negative -- rounded once to binary64, divided by (double)n and again by (double)n: vq, the population variance of
 *                 q; variance = ldexp(vq, -2 * shift)
 *   std           ldexp(sqrt(vq), -shift)
 *   q05, median, q95   with bins and m = sum(counts row) > 0: the ranks (m - 1) / 20, (m - 1) / 2 and (m - 1) - (m - 1) / 20 in integer
 *                 arithmetic, f3d_histogram_rank of each gives a bin k (q05_bin, median_bin, q95_bin), and the value is the binary64
 *                 midpoint (e_k + e_(k+1)) / 2.0 of that bin's float32 edges e_k = f3d_histogram_edge(lo, hi, bins, k), with hi for
 *                 e_bins: a quantile is known to a bin, no finer.  Without bins, or with m == 0, the values are NaN and the bins -1
 * summary (nullable): the numbers of OK, EMPTY and SMALL labels and mean = sum(n * mean) / sum(n) over the OK labels, both sums in
 * binary64 in label order, every operation rounded on its own; NaN without an OK label.
 * Returns non-zero (f3d_host_last_error() set) for a null sums or stats, counts given with bins == 0 or missing with bins > 0, shift
 * outside -100 .. 100, bins above 256, what f3d_histogram refuses of lo, hi, bins, or a row of counts that adds up to more than
 * 2^33. */
typedef struct f3d_label_field_stat {
  int status;
  int q05_bin, median_bin, q95_bin;
  unsigned long long n, below, above;
  double min, max, mean, variance, std, q05, median, q95;
} f3d_label_field_stat;
typedef struct f3d_label_field_summary {
  unsigned long long ok, empty, small;
  double mean;
} f3d_label_field_summary;
int f3d_label_field_solve(const struct f3d_label_field_sums* sums, const unsigned* counts /* n_labels * bins; null iff bins == 0 */,
                          size_t n_labels, int shift, float lo, float hi, size_t bins, unsigned long long min_voxels,
                          f3d_label_field_stat* stats /* n_labels entries */, f3d_label_field_summary* summary /* nullable */);

/* The shift of f3d_label_field_sums for a field whose finite values lie in [min, max], `finite` of them (f3d_value_range's results): with
 * m = max(|min|, |max|) = f * 2^e, f in [0.5, 1) (frexp), the shift is 24 - e clamped to -100 .. 100, and 0 when m == 0, nothing is
 * finite or a bound is not.  Unless the clamp acts (m at or above 2^124), m * 2^shift < 2^24: no finite voxel is out of range, the
 * quantum is 2^-24 of the largest magnitude, and an integer field below 2^24 in magnitude, a uint16 grey value say, is kept exactly.
 * Returns the shift; nothing can fail. */
int f3d_label_field_shift(float min, float max, unsigned long long finite);

/* Statistics of a field over the labels the driver keeps on the device (f3d_label_field_sums, then f3d_label_field_solve), and a value
 * per label painted into a volume (f3d_paint_labels).  The labels are those an earlier call uploaded or f3d_flow_labels_compute /
 * f3d_flow_labels_split made.
 *   f3d_flow_label_field_compute  field is a device container of the driver's geometry -- a derived field's container, say -- or 0 for
 *                                 the resident frame 0.  range is {lo, hi}, null iff bins == 0.  stats has n_labels entries (required);
 *                                 counts has n_labels * bins entries (null iff bins == 0); info and summary are nullable
 *   f3d_flow_labels_paint         values[l - 1] into the voxels of label l, NaN elsewhere, into a container of the driver's pool, and
 *                                 down into out (width * height * depth floats)
 * A device library without the entry a call needs still loads; then the call fails with a message naming the entry. */
int f3d_flow_label_field_compute(f3d_flow flow, f3d_devptr field /* 0: the resident frame 0 */, size_t n_labels, int shift,
                                 const float* range /* {lo, hi}; null iff bins == 0 */, size_t bins, unsigned long long min_voxels,
                                 f3d_label_field_stat* stats, unsigned* counts, f3d_label_field_info* info,
                                 f3d_label_field_summary* summary);
int f3d_flow_labels_paint(f3d_flow flow, const float* values, size_t n_labels, float* out);
/* f3d_value_range of `field` (0: the resident frame 0) masked by the driver's labels: the finite minimum and maximum over the voxels whose
 * label is not 0, from which a caller takes f3d_label_field_shift and, with bins, the range when it has none of its own. */
int f3d_flow_label_field_range(f3d_flow flow, f3d_devptr field /* 0: the resident frame 0 */, float* min, float* max, f3d_range_info* info);
/* The container of a field the driver holds, for f3d_flow_label_field_compute: "grey" (the resident frame 0), "vol", "eq"
 * (f3d_flow_strain_compute), "gmax" (the maximum shear of f3d_flow_principal_compute), "angle" (f3d_flow_polar_compute), "zncc", "rmsd"
 * (f3d_flow_match_compute), "wvol", "weq" (f3d_flow_window_strain_compute).  Fails for another name and until the field is computed;
 * the container is the driver's and lives as long as that field does. */
int f3d_flow_field_container(f3d_flow flow, const char* name, f3d_devptr* container);

/* Exact selection on a histogram of f3d_histogram (include/f3d.h has the bin rule).  Host code, no device needed.  Each returns
 * non-zero (f3d_host_last_error() set, nothing written) when it refuses its arguments.
 *
 * f3d_histogram_edge: the smallest float32 s in [lo, hi] whose bin is at least k, found by bisection over the ordered bit patterns with
 * the bin function the kernel runs.  k == 0 gives lo; k >= bins is refused, and so is what f3d_histogram refuses of lo, hi and bins.
 * By monotonicity {s in [lo, hi] : s >= edge} is exactly the set of bins k .., so f3d_label_components(lo = edge, hi).foreground equals
 * sum(counts[k:]) by construction, and with hi = the largest float below edge (nextafterf(edge, -inf)) and lo its foreground is
 * sum(counts[:k]).
 *
 * f3d_otsu: the cuts of classes = 2 or 3 that maximise the between-class variance, exactly specified.  With N(a,b) = sum h_i and
 * M(a,b) = sum i h_i over a <= i < b (exact integers; counts that add up to more than 2^33 are refused, so M < 2^45), a candidate is
 * 0 < c_1 (< c_2) < bins, its classes are the bins [0, c_1), [c_1, c_2), [c_2, bins), and its objective is the binary64 sum, left to
 * right in class order, of (double)M * (double)M / (double)N, every operation rounded on its own.  A candidate with an empty class is
 * skipped.  Candidates are walked in lexicographic order and replaced only on strict >, so ties go to the smallest cut.  cuts receives
 * classes - 1 bins: class j starts at bin cuts[j - 1], i.e. at the value f3d_histogram_edge(.., cuts[j - 1]).  info: status
 * F3D_OTSU_OK with the class populations and the objective, or F3D_OTSU_DEGENERATE when fewer bins are occupied than classes; then
 * nothing is written to cuts and populations and objective are 0.
 *
 * f3d_histogram_rank: the bin holding the r-th smallest used voxel (0-based), the first bin whose cumulative count exceeds r; refused
 * at r >= used. */
#define F3D_OTSU_OK 0
#define F3D_OTSU_DEGENERATE 1
typedef struct f3d_otsu_info {
  int status;
  unsigned long long populations[3];
  double objective;
} f3d_otsu_info;
int f3d_histogram_edge(float lo, float hi, size_t bins, size_t k, float* edge);
int f3d_otsu(const unsigned long long* counts, size_t bins, int classes /* 2 or 3 */, unsigned* cuts /* classes - 1 */, f3d_otsu_info* info);
int f3d_histogram_rank(const unsigned long long* counts, size_t bins, unsigned long long r, unsigned* bin);

/* Histogram of a frame on the device: f3d_histogram (include/f3d.h) of `frame`, a device container of the driver's geometry, or 0 for the
 * resident frame 0 that f3d_flow_labels_compute thresholds.  range: {lo, hi}, or null for the finite minimum and maximum of the frame
 * (f3d_value_range); the bounds used come back in *lo_used and *hi_used.  counts has bins entries; info is required.  The call fails
 * with a message that says which when the frame is constant or has no finite voxel (only with a null range).  A device library
 * without f3d_histogram or f3d_value_range still loads; then the call fails with a message naming the entry. */
int f3d_flow_histogram(f3d_flow flow, f3d_devptr frame /* 0: the resident frame 0 */, const float* range /* nullable: {lo, hi} */,
                       size_t bins, unsigned long long* counts, f3d_histogram_info* info, float* lo_used, float* hi_used);

/* Validation of the flow the driver holds or of the trajectory (source F3D_STRAIN_OF_FLOW / F3D_STRAIN_OF_TRAJECTORY):
 * f3d_validate_displacement (include/f3d.h has the definition and what step, eps, threshold, min_neighbours and mode mean) into
 * containers the driver keeps until f3d_flow_validate_end (or f3d_flow_destroy).  out[0] receives r, out[1..3] the validated u, v, w
 * (width * height * depth floats each); a null out[0] leaves r out, null out[1..3] (all three or none) the displacement; at least one
 * of the two is required.  fill_passes (needs out[1..3]): up to that many further passes over the result with threshold +inf, no mask
 * and F3D_VALIDATE_REPLACE, each of which gives the undefined voxels with at least min_neighbours defined neighbours their median;
 * they stop when no voxel is undefined or the count stops falling.  stats (nullable) are those of the first pass with replaced and
 * undefined brought to the final state.  min_zncc is f3d_flow_motion_compute's: NaN for no mask; otherwise voxels whose zncc in the
 * last f3d_flow_match_compute of the same pair is below it (or NaN) are absent -- rejected themselves and no neighbour of anyone; the
 * call fails with a message when that zncc is not there, and when source is the trajectory.  A device library without
 * f3d_validate_displacement still loads; then the call fails with a message naming the entry. */
int f3d_flow_validate_compute(f3d_flow flow, int source, unsigned step, float eps, float threshold, unsigned min_neighbours,
                              unsigned mode, unsigned fill_passes, float min_zncc, float* const out[4], f3d_validate_stats* stats);
int f3d_flow_validate_end(f3d_flow flow);

/* The solve from the records of f3d_block_match (include/f3d_block_match.h) to one row per node.  Host code, no device needed;
 * binary64, every operation rounded on its own, in exactly this order.  With n = (2 window + 1)^3 and da = n saa - sa^2 of a record,
 * the ZNCC of a shift with sums sb, sbb, sab is
 *   z = (double)(n sab - sa sb) / sqrt((double)da * (double)(n sbb - sb^2))
 * zncc is z at the best shift, z0.  Per axis, when both face neighbours of the best shift are valid, with z- and z+ theirs:
 *   curvature = (z- - 2.0 * z0) + z+;  when curvature < 0.0:  offset = (z- - z+) / (2.0 * curvature), clamped to [-0.5, 0.5]
 * and the offset is 0.0 otherwise (the three-point parabola through the peak).  status, the first that applies:
 *   F3D_BLOCK_NODE_FLAT  the record says the window of frame 0 is constant
 *   F3D_BLOCK_NODE_NONE  the record has no candidate
 *   F3D_BLOCK_NODE_LOW   zncc < min_zncc
 *   F3D_BLOCK_NODE_EDGE  along an axis with a search radius above 0 the best shift lies radius from the centre: on the face of the
 *                        search range, the motion is probably beyond reach
 *   F3D_BLOCK_NODE_OK
 * u, v, w = (float)((double)shift + offset) when the status is OK or EDGE, NaN otherwise; shift, zncc (NaN) and offset (0) of a FLAT
 * or NONE node are empty.  position is the node's voxel; evaluated, outside, flat are the record's counts.  centre is the array given
 * to f3d_block_match (nullable: all zero).  Returns non-zero (f3d_host_last_error() set, nothing written) for a null records, grid
 * or nodes, a grid f3d_block_match refuses, or a NaN min_zncc. */
#define F3D_BLOCK_NODE_OK 0
#define F3D_BLOCK_NODE_FLAT 1
#define F3D_BLOCK_NODE_NONE 2
#define F3D_BLOCK_NODE_LOW 3
#define F3D_BLOCK_NODE_EDGE 4
typedef struct f3d_block_match_node {
  int position[3];
  int shift[3];
  int status;
  int evaluated, outside, flat;
  double zncc;
  double offset[3];
  float u, v, w;
  int reserved; /* 0 */
} f3d_block_match_node;
typedef struct f3d_block_match_summary {
  unsigned long long nodes, ok, flat, none, low, edge; /* nodes is the sum of the others */
} f3d_block_match_summary;
/* The grid of nodes block matching lays over a width x height x depth volume: nodes `step` apart whose (2 window + 1)^3 windows lie
 * inside the volume, as many as fit, centred: per axis of n voxels, with room = n - 1 - 2 window, the first node lies at
 * window + (room % step) / 2 and there are (n - 1 - window - first) / step + 1 of them (integer arithmetic).  Host code.  Returns
 * non-zero (f3d_host_last_error() set, nothing written) for a null grid, a step below 1, a window outside 1 .. 8, a negative radius,
 * window + radius above 16, a window that leaves the volume, or more than 2^22 nodes. */
int f3d_block_match_layout(size_t width, size_t height, size_t depth, int step, int window, int rx, int ry, int rz,
                           f3d_block_match_grid* grid);
int f3d_block_match_solve(const f3d_block_match_record* records, const f3d_block_match_grid* grid, const int* centre, double min_zncc,
                          f3d_block_match_node* nodes /* nx ny nz entries */, f3d_block_match_summary* summary /* nullable */);

/* Block matching on the pair the driver holds (f3d_flow_upload), and the guess of the solve from it.
 *   f3d_flow_block_match      f3d_block_match_layout over the driver's volume, f3d_block_match of the resident frames 0 and 1 on the
 *                             library stream (range null: the finite minimum and maximum of frame 0, f3d_value_range), then
 *                             f3d_block_match_solve.  centre (nullable) has one int32 triple per node of that layout.  grid, info,
 *                             summary are nullable.  The records and the rows stay with the driver.
 *   f3d_flow_block_match_rows copies them out: records and / or nodes (each nullable) with room for `capacity` nodes; fails when
 *                             there are more, or none yet
 *   f3d_flow_initial_from_nodes  the node vectors u, v, w of the rows as an nx x ny x nz volume through f3d_validate_displacement
 *                             (F3D_VALIDATE_REPLACE, no weight, step 1, eps 0.1, threshold 2, 9 neighbours; validated nullable),
 *                             the result through f3d_expand_nodes into the driver's initial-flow containers, those through
 *                             f3d_initial_flow (info nullable).  Afterwards f3d_flow_compute_resident_from_initial starts from it.
 * A device library without f3d_block_match, f3d_expand_nodes, f3d_value_range, f3d_validate_displacement or f3d_initial_flow still
 * loads; then the call that needs it fails with a message naming it.  Failures are described by f3d_host_last_error(). */
int f3d_flow_block_match(f3d_flow flow, int step, int window, int rx, int ry, int rz, size_t bins, const float* range /* lo, hi */,
                         const int* centre, double min_zncc, f3d_block_match_grid* grid, f3d_block_match_info* info,
                         f3d_block_match_summary* summary);
int f3d_flow_block_match_rows(f3d_flow flow, size_t capacity, f3d_block_match_record* records, f3d_block_match_node* nodes);
int f3d_flow_initial_from_nodes(f3d_flow flow, f3d_validate_stats* validated, f3d_initial_info* info);

/* The table of the records of f3d_subset_match (include/f3d_subset_match.h): one row per node.  Host code, no device
 * needed.  status is the record's, but a record that is OK with not zncc >= min_zncc is F3D_SUBSET_NODE_LOW.  position, iterations
 * and zncc are the node's and the record's.  u, v, w = (float)p[0], p[4], p[8] and grad = (float) of ux, uy, uz, vx, ..., wz when
 * the status is OK, NaN otherwise.  compare (nullable) points to three float32 arrays of nx ny nz node values, a displacement to hold
 * against: diff[k] = (float)((double)compare[k][node] - (double)(u, v, w)[k]), NaN without compare.
 * Summary: status[] counts the rows per status; median_zncc is over the records that are OK (before the LOW test); compared counts
 * the OK rows whose three differences are not NaN, and over their lengths sqrt((d0 d0 + d1 d1) + d2 d2), binary64, every operation
 * rounded on its own: rms = sqrt((the squares added in node order) / compared), median and p95.  Of m sorted values the median is
 * the one at (m - 1) / 2 and the 95 % quantile the one at (95 m + 99) / 100 - 1 (integer arithmetic); NaN when m = 0.
 * Returns non-zero (f3d_host_last_error() set, nothing written) for a null records, grid or nodes, a grid f3d_subset_match refuses
 * on its own numbers (step, counts, window; a node below 0 or beyond 2^30), or a NaN min_zncc. */
#define F3D_SUBSET_NODE_LOW 9
#define F3D_SUBSET_NODE_STATUS_COUNT 10
typedef struct f3d_subset_match_node {
  int position[3];
  int status;
  int iterations;
  int reserved; /* 0 */
  double zncc;
  float u, v, w;
  float grad[9];
  float diff[3];
  int reserved2; /* 0 */
} f3d_subset_match_node;
typedef struct f3d_subset_match_summary {
  unsigned long long nodes;
  unsigned long long status[F3D_SUBSET_NODE_STATUS_COUNT]; /* they add up to nodes */
  unsigned long long compared;
  double median_zncc;
  double rms, median, p95; /* of |compare - subset| */
} f3d_subset_match_summary;
/* The grid subset correlation lays over a width x height x depth volume, as f3d_block_match_layout does with one voxel more to each
 * face (the central differences): with reach = window + 1 and room = n - 1 - 2 reach per axis of n voxels, the first node lies at
 * reach + (room % step) / 2 and there are (n - 1 - reach - first) / step + 1 of them.  Non-zero (nothing written) for a null grid, a
 * step below 1, a window outside 1 .. 8, a window that leaves the volume, or more than 2^22 nodes. */
int f3d_subset_match_layout(size_t width, size_t height, size_t depth, int step, int window, f3d_subset_match_grid* grid);
int f3d_subset_match_table(const f3d_subset_match_record* records, const f3d_subset_match_grid* grid, double min_zncc,
                           const float* const* compare /* nullable: three arrays */, f3d_subset_match_node* nodes /* nx ny nz entries */,
                           f3d_subset_match_summary* summary /* nullable */);
/* Subset correlation on the pair the driver holds (f3d_flow_upload): f3d_subset_match_layout over the driver's volume,
 * f3d_subset_match of the resident frames 0 and 1 on the library stream, then f3d_subset_match_table.  start says where the start
 * translations come from (the start gradients are zero): F3D_SUBSET_START_ZERO; F3D_SUBSET_START_NODES, the block-match table the
 * driver holds (f3d_flow_block_match first), each subset node taking u, v, w of the block-match node nearest to it per axis (the
 * lower of two equally near), NaN unless that node is ok or edge; F3D_SUBSET_START_FLOW, the held flow read at the node voxels.
 * Whenever the driver holds a flow, its values at the node voxels are the table's comparison.  reach 0 means the window radius.
 * grid, info, summary are nullable.  The records and rows stay with the driver; f3d_flow_subset_match_rows copies them out (each
 * nullable, room for `capacity` nodes).  A device library without f3d_subset_match still loads; then the call fails with a
 * message naming it. */
#define F3D_SUBSET_START_ZERO 0
#define F3D_SUBSET_START_NODES 1
#define F3D_SUBSET_START_FLOW 2
int f3d_flow_subset_match(f3d_flow flow, int step, int window, int model, int start, int max_iterations, double tolerance, double reach,
                          double min_zncc, f3d_subset_match_grid* grid, f3d_subset_match_info* info, f3d_subset_match_summary* summary);
int f3d_flow_subset_match_rows(f3d_flow flow, size_t capacity, f3d_subset_match_record* records, f3d_subset_match_node* nodes);
/* message of this thread's last call that failed in the host library itself; f3d_last_error() when there is none */
const char* f3d_host_last_error(void);
int f3d_flow_destroy(f3d_flow flow);

/* name: "add" | "convolution" | "median" | "registration" | "resample" | "solve" */
int f3d_op_create(f3d_op* op, const char* name);
const char* f3d_op_name(f3d_op op);
int f3d_op_initialize(f3d_op op, const f3d_size4* container_size);
/* Execute(OperationParameters&): keys[i] -> value_ptrs[i] (non-owning, like the reference's bag) */
int f3d_op_execute(f3d_op op, const char* const* keys, void* const* value_ptrs, size_t count);
/* ExecuteBatch of the add, median and resample operators: `bags` bags laid end to end, bag b holding counts[b] entries -- up to
 * three volumes of one box in one launch per kernel where the bags allow it, otherwise one Execute after the other (same results).
 * Non-zero for operators without a batch form. */
int f3d_op_execute_batch(f3d_op op, const char* const* keys, void* const* value_ptrs, const size_t* counts, size_t bags);
int f3d_op_set_slab(f3d_op op, const f3d_slab* slab);
int f3d_op_destroy(f3d_op op);

/* host-only helpers (no device needed) */
/* ---- piecemeal (out-of-core) path: host volumes streamed through the device in z-chunks --------------------
 * Operators "add_p", "resample_p", "registration_p", "solve_p", "stat_p" (f3d_op_create) mirror
 * src/cuda_operations/partial_data/cuda_operation_*_p.cpp: they take no container at initialize (pass NULL) and their
 * Data3D* keys (operand_0, input, output, frame_0, flow_u, temp, ...) take f3d_volume_object() of a wrapped volume. */
typedef struct f3d_volume_s* f3d_volume;
/* non-owning Data3D view of caller memory (src/data_types/data3d.h:22-62) */
int f3d_volume_wrap(f3d_volume* vol, float* data, size_t width, size_t height, size_t depth);
void* f3d_volume_object(f3d_volume vol);
/* the storage the view addresses NOW: registration_p and solve_p swap storage between their volumes like the reference
 * (Data3D::Swap, cuda_operation_register_p.cpp:138, cuda_operation_solve_p.cpp:167-169) */
float* f3d_volume_data(f3d_volume vol);
int f3d_volume_destroy(f3d_volume vol);
/* what the last solve_p Execute did */
int f3d_op_solve_p_last(f3d_op op, int* chunk, int* outer_per_pass, int* halo, size_t* passes, int* overlapped);
/* 1 when the last execute of the "solve_p" operator ran the last sweep of an outer iteration together with the weights of the next
 * one (a second weight pair per chunk set: 15 fields instead of 13, taken when they fit and a residency holds two outer iterations
 * or more) */
int f3d_op_solve_p_fused_weights(f3d_op op, int* fused);
/* chunk plan of solve_p for a level (pure host arithmetic) and the device budget it would use now.  overlap_mode 0 = copies
 * and kernels in order, 1 = two chunk sets with the copies beside the kernels, -1 = whichever the cost model prefers */
int f3d_plan_solve_piecemeal(size_t budget_bytes, size_t width, size_t height, int depth, int inner_iterations, int outer_iterations,
                             int forced_outer_per_pass, int overlap_mode, int* chunk, int* outer_per_pass, int* halo, int* max_planes,
                             int* overlapped);
size_t f3d_piecemeal_budget_bytes(void);
/* how the solver drivers cut the `inner` sweeps of ONE outer iteration into launches (pure host arithmetic, host/solve_schedule.h).
 * fused: the solve takes the fused launches; tri: the three-stage launches too; carry: another outer iteration follows and the
 * driver can take its weights along.  Fills up to `capacity` launches: sweeps[i] = 1 .. 3 sweeps in launch i, next_weights[i] = 1
 * when it also writes the next phi / ksi; returns their number, or -1 if capacity is too small. */
int f3d_plan_sweeps(int inner, int fused, int tri, int carry, int* sweeps, int* next_weights, int capacity);
/* the weights-first cut of the same sweeps (the resident solve operator on levels that take f3d_solve_phi_ksi_sweep_fd): launch 0 is
 * (phi/ksi of this outer iteration, sweep) -- weights_first[0] = 1 --, then two sweeps per launch, then one for an even `inner`; no
 * launch writes the next weights.  first[i] = index of launch i's first sweep within the outer iteration (the operator finds the level's
 * last launch by first + sweeps = inner).  Same return convention. */
int f3d_plan_sweeps_weights_first(int inner, int* first, int* sweeps, int* weights_first, int* next_weights, int capacity);
/* how a fused solver launch (k_pair8) of a level window is cut into workgroups (pure host arithmetic, csrc/f3d_pair8_plan.h; DESIGN.md
 * section 3, "Launch shapes"): the first A tiles in a chunks of zc_a planes each, the other tiles in b chunks of zc_b planes; A = 0 is
 * the uniform plan.  width, rows, planes: extents of the window; ty: rows per tile; zc_limit: planes a chunk may hold at most;
 * per_round: workgroups that run at a time (<= 0: 256, or F3D_PAIR8_ROUND); fold: the last tile column holds two row bands per tile.
 * plan[8] = A, a, b, zc_a, zc_b, workgroups, cost in plane steps, tiles.  F3D_PAIR8_PLAN=0 gives the uniform plan. */
int f3d_pair8_plan(int width, int rows, int planes, int ty, int zc_limit, int per_round, int fold, long long* plan);
/* the `zc_limit` of the solver launches (the launchers' own function, csrc/f3d_pair8_plan.h): the planes a z-chunk may hold at most
 * in a container whose planes are plane_bytes = container height x pitch bytes, for a launch that reads `reach` halo planes on either
 * side of a chunk (1: f3d_phi_ksi[_zones], f3d_solve_sweep[_add]; 2: the two-stage launches; 3: f3d_solve_sweep3,
 * f3d_solve_sweep2_phi_ksi) -- a chunk and its halo span at most 2^32 bytes, which is what the kernels' 32-bit byte offsets cover.
 * 0: not even one plane fits, and every such launch refuses the container (a level that marches along y is not cut in z). */
int f3d_solver_chunk_limit(unsigned long long plane_bytes, int reach);
/* the kernel's decode of workgroup numbers first .. first + count - 1 under plan[0 .. 4] (the same function, compiled for the host):
 * out[6 i ..] = tile, tile column, tile row, folded, z0, z1 (planes [z0, z1) of [z_lo, z_hi)), or six times -1 for a padding number.
 * *grid (if given) = workgroup numbers of the launch.  Returns 0, or 1 for arguments that make no plan. */
int f3d_pair8_decode(int width, int rows, int ty, int fold, const long long* plan, int xcd_remap, int z_lo, int z_hi, int first,
                     int count, int* out, int* grid);
/* the plan the fused z-marching launches take (the launcher's own function): up to three classes of tiles in tile order, class i
 * of tiles_i tiles in chunks_i chunks of zc_i planes, every class but the last filling whole rounds; an empty class has no tiles.
 * F3D_PAIR8_PLAN (read per call) unset or 2: the wide plan, taken where it is strictly cheaper than f3d_pair8_plan's; 1: exactly
 * f3d_pair8_plan's; 0: the uniform plan.  Arguments as for f3d_pair8_plan.
 * plan[12] = tiles_a, chunks_a, zc_a, tiles_b, chunks_b, zc_b, tiles_c, chunks_c, zc_c, workgroups, cost in plane steps, tiles. */
int f3d_pair8_plan_wide(int width, int rows, int planes, int ty, int zc_limit, int per_round, int fold, long long* plan);
/* f3d_pair8_decode under plan[0 .. 8] of f3d_pair8_plan_wide */
int f3d_pair8_decode_wide(int width, int rows, int ty, int fold, const long long* plan, int xcd_remap, int z_lo, int z_hi, int first,
                          int count, int* out, int* grid);

/* OpticalFlowP (src/optical_flow/optical_flow_p.h:35-57; ComputeFlow optical_flow_p.cpp:57-318): no pre-blur, no median */
typedef struct f3d_pflow_s* f3d_pflow;
int f3d_pflow_create(f3d_pflow* flow);
int f3d_pflow_initialize(f3d_pflow flow, size_t width, size_t height, size_t depth);
int f3d_pflow_compute(f3d_pflow flow, const float* frame_0, const float* frame_1, size_t width, size_t height, size_t depth,
                      const f3d_flow_params* params, int silent, float* u, float* v, float* w, float* device_seconds);
/* of the last compute: solver residencies, levels cut into chunks, coarse levels that ran wholly on the device */
int f3d_pflow_stats(f3d_pflow flow, size_t* solve_passes, size_t* streamed_levels, size_t* resident_levels);
/* of the last compute: host levels whose frame 1 was registered inside the solver's first residency instead of by the separate
 * registration operator (cuda_operation_register_p.cpp:54-139); F3D_P_FUSED_WARP=0 keeps the operator everywhere */
int f3d_pflow_levels_registered_inside(f3d_pflow flow, size_t* levels);
/* of the last compute: host levels whose solver held the two frames and u, v, w on the device for the whole level beside the chunk sets
 * (three fields up per residency instead of eight; chosen by the cost model, F3D_P_CONSTANTS=0 / 1 pins it) */
int f3d_pflow_levels_with_constants_on_device(f3d_pflow flow, size_t* levels);
/* whether the resident levels of the last compute resampled their frames from device copies of the two originals */
int f3d_pflow_originals_on_device(f3d_pflow flow, int* yes);
/* also apply the Gaussian pre-blur and the per-level median, i.e. OpticalFlowE's whole pipeline on host volumes (off by
 * default like the reference's piecemeal driver; F3D_P_FULL=1 also turns it on).  The two extra operators are
 * "convolution_p" (keys input, output, data_size, gaussian_sigma) and "median_p" (input, output, data_size, radius). */
int f3d_pflow_set_full_pipeline(f3d_pflow flow, int enabled);
/* coarse levels whose working set fits the budget stay on the device (default on; F3D_P_RESIDENT=0 also turns it off) */
int f3d_pflow_set_resident(f3d_pflow flow, int enabled);
/* wall seconds of the last compute in {frame resample, flow resample, registration, solve, add} of the levels that went
 * through the host, and [5] in the resident coarse levels */
int f3d_pflow_operator_seconds(f3d_pflow flow, double* seconds6);
int f3d_pflow_destroy(f3d_pflow flow);

size_t f3d_max_warp_level(size_t width, size_t height, size_t depth, float scale_factor);
int f3d_level_geometry(size_t width, size_t height, size_t depth, float scale_factor, int level,
                       f3d_size4* size, float* hx, float* hy, float* hz);
int f3d_gaussian_taps(float sigma, float* taps, size_t capacity, size_t* radius);
int f3d_raw_read_u8(const char* path, size_t width, size_t height, size_t depth, float* out);
int f3d_raw_read_f32(const char* path, size_t width, size_t height, size_t depth, float* out);
int f3d_raw_write_u8(const char* path, const float* in, size_t width, size_t height, size_t depth);
int f3d_raw_write_f32(const char* path, const float* in, size_t width, size_t height, size_t depth);
int f3d_vtk_write_flow(const char* path, const float* u, const float* v, const float* w, size_t width, size_t height,
                       size_t depth);
/* translated-Gaussian pair: 64 blobs, splitmix64 seed 20241003, frame_1(p) = frame_0(p - t), t = (2, -1, 0.5) */
int f3d_synth_pair(size_t width, size_t height, size_t depth, float* frame_0, float* frame_1);
/* slab form: planes [z_lo, z_hi) only, unscaled, plus the maximum of frame_0 over them (scale = 255 / global max) */
int f3d_synth_planes(size_t width, size_t height, size_t depth, size_t z_lo, size_t z_hi, float* frame_0, float* frame_1,
                     float* frame_0_max);

/* ---- multi-GPU z-slab driver (OpticalFlowSlab; no reference counterpart) ------------------------ */

typedef struct f3d_slabflow_s* f3d_slabflow;

/* n_ranks slabs in total; this process computes local_ranks[0..n_local): one rank (RCCL between processes, after
 * f3d_comm_init) or all n_ranks (one-GPU rehearsal with plane copies instead of RCCL). */
int f3d_slabflow_create(f3d_slabflow* flow, int n_ranks, const int* local_ranks, int n_local, int halo_capacity);
int f3d_slabflow_initialize(f3d_slabflow flow, size_t width, size_t height, size_t depth);
/* frames and flows are FULL volumes; only the planes of the local ranks are read / written */
int f3d_slabflow_compute(f3d_slabflow flow, const float* frame_0, const float* frame_1, const f3d_flow_params* params,
                         float* u, float* v, float* w);
int f3d_slabflow_upload(f3d_slabflow flow, const float* frame_0, const float* frame_1);
int f3d_slabflow_compute_resident(f3d_slabflow flow, const f3d_flow_params* params, float* device_seconds);
int f3d_slabflow_download(f3d_slabflow flow, float* u, float* v, float* w);
/* outer iterations of the last solve whose halo exchange ran beside the interior of the slab (diagnostics) */
int f3d_slabflow_overlapped_iterations(f3d_slabflow flow, size_t* count);
/* groups of several outer iterations the last compute ran between two exchanges (thin slabs of small levels take
 * n (K + 1) halo planes at once; F3D_SLAB_OUTER_PER_EXCHANGE=n forces n, 1 = one exchange per outer iteration) */
int f3d_slabflow_batched_exchanges(f3d_slabflow flow, size_t* count);
/* pyramid levels of the last compute whose warp reached further along z than the halo room of the local containers: frame 1 was
 * gathered into a container of its own from as many ranks as the reach spans (SURVEY.md 8e fallback) */
int f3d_slabflow_gathered_warps(f3d_slabflow flow, size_t* count);
/* exchanges of the last compute made after a solver stage (F3D_SLAB_EXCHANGE=stage: 2 / 1 / 3 planes after the fused pairs and the
 * last sweep instead of 6 planes once per outer iteration; same bits, fewer redundant planes, three times the messages) */
int f3d_slabflow_stage_exchanges(f3d_slabflow flow, size_t* count);
/* the exchange order of the solves that follow: 0 = once per outer iteration (default), 1 = after every solver stage.  Both give the
 * single-GPU bits; which is faster depends on the machine's exchange latency, so bench.py --gpus N times both in one run. */
int f3d_slabflow_set_exchange_per_stage(f3d_slabflow flow, int per_stage);
int f3d_slabflow_destroy(f3d_slabflow flow);

/* the decomposition plan (pure host arithmetic, usable without a device) */
int f3d_plan_owned(int depth, int rank, int n_ranks, int* lo, int* hi);
/* fills up to `capacity` transfers; returns their number, or -1 if capacity is too small */
int f3d_plan_exchange(int depth, int rank, int n_ranks, int need_lo, int need_hi, int* peer, int* send_lo, int* send_hi,
                      int* recv_lo, int* recv_hi, int capacity);
int f3d_plan_resample_source(int in_depth, int out_depth, int out_lo, int out_hi, int* lo, int* hi);

#ifdef __cplusplus
}
#endif
#endif /* F3D_HOST_H_ */
