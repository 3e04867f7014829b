// C ABI of the host side (include/f3d_host.h): thin, exception-free wrappers over the C++ classes.
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "f3d_host.h"
#include "block_match.h"
#include "subset_match.h"
#include "contact_kinematics.h"
#include "label_field.h"
#include "label_shape.h"
#include "label_track.h"
#include "hip_utils.h"
#include "motion_fit.h"
#include "operations.h"
#include "operations_p.h"
#include "optical_flow.h"
#include "optical_flow_p.h"
#include "optical_flow_slab.h"
#include "synth.h"
#include "threshold_select.h"
#include "../csrc/f3d_pair8_plan.h"

struct f3d_flow_s {
  OpticalFlowE driver;
  bool device_ready = false;
  bool trajectory_started = false;
  bool zncc_of_held_flow = false;  // the match container holds the zncc of the flow the driver holds (f3d_flow_motion_compute's mask)
  std::vector<f3d_contact> contacts;  // what f3d_flow_contacts_compute hands out
  std::vector<unsigned long long> label_sizes;  // what f3d_flow_labels_compute hands out
  std::vector<unsigned long long> label_b_sizes;  // what f3d_flow_labels_b_segment hands out
  std::vector<f3d_overlap> overlaps;  // what f3d_flow_overlap_compute hands out
};

struct f3d_slabflow_s {
  OpticalFlowSlab* driver = nullptr;
  ~f3d_slabflow_s() { delete driver; }
};

struct f3d_pflow_s {
  OpticalFlowP driver;
};

struct f3d_volume_s {
  Data3D view;
  f3d_volume_s(float* data, size_t w, size_t h, size_t d) : view(data, w, h, d) {}
};

struct f3d_op_s {
  CudaOperationBase* op = nullptr;
  ~f3d_op_s() { delete op; }
};

namespace {

// message of the last failed call of this thread that failed in the host library itself (f3d_host_last_error)
thread_local std::string g_host_error;

int HostFail(const char* what)
{
  g_host_error = what ? what : "unknown error";
  return 1;
}

void FillBag(OperationParameters& bag, f3d_flow_params& p)
{
  bag.PushValuePtr("warp_levels_count", &p.warp_levels_count);
  bag.PushValuePtr("warp_scale_factor", &p.warp_scale_factor);
  bag.PushValuePtr("outer_iterations_count", &p.outer_iterations_count);
  bag.PushValuePtr("inner_iterations_count", &p.inner_iterations_count);
  bag.PushValuePtr("equation_alpha", &p.equation_alpha);
  bag.PushValuePtr("equation_smoothness", &p.equation_smoothness);
  bag.PushValuePtr("equation_data", &p.equation_data);
  bag.PushValuePtr("median_radius", &p.median_radius);
  bag.PushValuePtr("gaussian_sigma", &p.gaussian_sigma);
}

}  // namespace

extern "C" {

void f3d_flow_default_params(f3d_flow_params* p)
{
  p->warp_levels_count = 40;
  p->warp_scale_factor = 0.95f;
  p->outer_iterations_count = 40;
  p->inner_iterations_count = 5;
  p->equation_alpha = 7.5f;
  p->equation_smoothness = 0.001f;
  p->equation_data = 0.001f;
  p->median_radius = 5;
  p->gaussian_sigma = 2.0f;
}

int f3d_flow_create(f3d_flow* flow)
{
  if (!flow) return 1;
  *flow = new (std::nothrow) f3d_flow_s;
  return *flow ? 0 : 1;
}

int f3d_flow_initialize(f3d_flow flow, size_t width, size_t height, size_t depth)
{
  if (!flow) return 1;
  if (f3d_init(-1) != 0) {
    std::fprintf(stderr, "f3d_flow_initialize: %s\n", f3d_last_error());
    return 1;
  }
  DataSize4 size = {width, height, depth, 0};
  return flow->driver.Initialize(size) ? 0 : 1;
}

int f3d_flow_compute(f3d_flow flow, const float* frame_0, const float* frame_1, const f3d_flow_params* params,
                     int silent, float* u, float* v, float* w)
{
  if (!flow || !frame_0 || !frame_1 || !params || !u || !v || !w) return 1;
  const DataSize4& c = flow->driver.ContainerSize();
  Data3D f0(const_cast<float*>(frame_0), c.width, c.height, c.depth);
  Data3D f1(const_cast<float*>(frame_1), c.width, c.height, c.depth);
  Data3D fu(u, c.width, c.height, c.depth), fv(v, c.width, c.height, c.depth), fw(w, c.width, c.height, c.depth);
  f3d_flow_params p = *params;
  OperationParameters bag;
  FillBag(bag, p);
  flow->driver.silent = silent != 0;
  flow->driver.ComputeFlow(f0, f1, fu, fv, fw, bag);
  return 0;
}

int f3d_flow_upload(f3d_flow flow, const float* frame_0, const float* frame_1)
{
  if (!flow || !frame_0 || !frame_1) return 1;
  flow->zncc_of_held_flow = false;
  const DataSize4& c = flow->driver.ContainerSize();
  Data3D f0(const_cast<float*>(frame_0), c.width, c.height, c.depth);
  Data3D f1(const_cast<float*>(frame_1), c.width, c.height, c.depth);
  if (!flow->driver.AllocateResidentFrames()) return 1;
  flow->driver.UploadResidentFrames(f0, f1);
  return 0;
}

int f3d_flow_compute_resident(f3d_flow flow, const f3d_flow_params* params, int silent, float* device_seconds)
{
  if (!flow || !params) return 1;
  flow->zncc_of_held_flow = false;
  f3d_flow_params p = *params;
  OperationParameters bag;
  FillBag(bag, p);
  flow->driver.silent = silent != 0;
  flow->driver.ComputeFlowResident(bag);
  if (device_seconds) *device_seconds = flow->driver.LastDeviceSeconds();
  return 0;
}

int f3d_flow_download(f3d_flow flow, float* u, float* v, float* w)
{
  if (!flow || !u || !v || !w) return 1;
  const DataSize4& c = flow->driver.ContainerSize();
  Data3D fu(u, c.width, c.height, c.depth), fv(v, c.width, c.height, c.depth), fw(w, c.width, c.height, c.depth);
  flow->driver.DownloadFlow(fu, fv, fw);
  return 0;
}

int f3d_flow_container(f3d_flow flow, f3d_size4* container)
{
  if (!flow || !container) return 1;
  const DataSize4& c = flow->driver.ContainerSize();
  *container = {c.width, c.height, c.depth, c.pitch};
  return 0;
}

int f3d_flow_set_level_stats(f3d_flow flow, int enable)
{
  if (!flow) return 1;
  flow->driver.collect_level_statistics = enable != 0;
  return 0;
}

int f3d_flow_level_stat_count(f3d_flow flow, size_t* count)
{
  if (!flow || !count) return 1;
  *count = flow->driver.LevelStats().size();
  return 0;
}

int f3d_flow_level_stat(f3d_flow flow, size_t index, f3d_level_stat* out)
{
  if (!flow || !out || index >= flow->driver.LevelStats().size()) return 1;
  const OpticalFlowE::LevelStatistics& st = flow->driver.LevelStats()[index];
  out->level = st.level;
  out->width = st.size.width;
  out->height = st.size.height;
  out->depth = st.size.depth;
  out->residual_rms = st.before.rms;
  out->residual_mean_abs = st.before.mean_abs;
  out->residual_max_abs = st.before.max_abs;
  out->flow_min = st.flow.min;
  out->flow_max = st.flow.max;
  out->flow_avg = st.flow.avg;
  return 0;
}

int f3d_flow_final_residual(f3d_flow flow, double registered[3], double unregistered[3])
{
  if (!flow || !registered || !unregistered) return 1;
  OpticalFlowE::Residual a, b;
  if (!flow->driver.FinalResidual(a, b)) return 1;
  registered[0] = a.rms; registered[1] = a.mean_abs; registered[2] = a.max_abs;
  unregistered[0] = b.rms; unregistered[1] = b.mean_abs; unregistered[2] = b.max_abs;
  return 0;
}

int f3d_flow_trajectory_begin(f3d_flow flow)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_trajectory_begin: null driver");
  if (!flow->driver.ResetTrajectory()) return HostFail(flow->driver.TrajectoryError().c_str());
  flow->trajectory_started = true;
  return 0;
}

int f3d_flow_trajectory_append(f3d_flow flow)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_trajectory_append: null driver");
  if (!flow->trajectory_started) return HostFail("f3d_flow_trajectory_append: f3d_flow_trajectory_begin has not been called");
  if (!flow->driver.ComposeTrajectory()) return HostFail(flow->driver.TrajectoryError().c_str());
  return 0;
}

int f3d_flow_trajectory_download(f3d_flow flow, float* u, float* v, float* w, unsigned long long* lost)
{
  g_host_error.clear();
  if (!flow || !u || !v || !w) return HostFail("f3d_flow_trajectory_download: null argument");
  if (!flow->trajectory_started) return HostFail("f3d_flow_trajectory_download: f3d_flow_trajectory_begin has not been called");
  const DataSize4& c = flow->driver.ContainerSize();
  Data3D fu(u, c.width, c.height, c.depth), fv(v, c.width, c.height, c.depth), fw(w, c.width, c.height, c.depth);
  if (!flow->driver.DownloadTrajectory(fu, fv, fw, lost)) return HostFail(flow->driver.TrajectoryError().c_str());
  return 0;
}

int f3d_flow_trajectory_end(f3d_flow flow)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_trajectory_end: null driver");
  flow->driver.ReleaseTrajectory();
  flow->trajectory_started = false;
  return 0;
}

int f3d_flow_initial_upload(f3d_flow flow, const float* u, const float* v, const float* w, f3d_initial_info* info)
{
  g_host_error.clear();
  if (!flow || !u || !v || !w) return HostFail("f3d_flow_initial_upload: null argument");
  const DataSize4& c = flow->driver.ContainerSize();
  Data3D fu(const_cast<float*>(u), c.width, c.height, c.depth), fv(const_cast<float*>(v), c.width, c.height, c.depth),
      fw(const_cast<float*>(w), c.width, c.height, c.depth);
  if (!flow->driver.SetInitialFlow(fu, fv, fw, info)) return HostFail(flow->driver.InitialFlowError().c_str());
  return 0;
}

int f3d_flow_initial_take(f3d_flow flow, int source, f3d_initial_info* info)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_initial_take: null driver");
  if (source != F3D_STRAIN_OF_FLOW && source != F3D_STRAIN_OF_TRAJECTORY)
    return HostFail("f3d_flow_initial_take: source must be F3D_STRAIN_OF_FLOW or F3D_STRAIN_OF_TRAJECTORY");
  if (source == F3D_STRAIN_OF_TRAJECTORY && !flow->trajectory_started)
    return HostFail("f3d_flow_initial_take: no trajectory is active (f3d_flow_trajectory_begin first)");
  const OpticalFlowE::Displacement of = source == F3D_STRAIN_OF_FLOW ? OpticalFlowE::HeldFlow() : OpticalFlowE::Trajectory();
  if (!flow->driver.SetInitialFlow(of, info)) return HostFail(flow->driver.InitialFlowError().c_str());
  return 0;
}

int f3d_flow_initial_download(f3d_flow flow, float* u, float* v, float* w)
{
  g_host_error.clear();
  if (!flow || !u || !v || !w) return HostFail("f3d_flow_initial_download: null argument");
  const DataSize4& c = flow->driver.ContainerSize();
  Data3D fu(u, c.width, c.height, c.depth), fv(v, c.width, c.height, c.depth), fw(w, c.width, c.height, c.depth);
  if (!flow->driver.DownloadInitialFlow(fu, fv, fw)) return HostFail(flow->driver.InitialFlowError().c_str());
  return 0;
}

int f3d_flow_initial_end(f3d_flow flow)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_initial_end: null driver");
  flow->driver.ReleaseInitialFlow();
  return 0;
}

int f3d_flow_compute_resident_from_initial(f3d_flow flow, const f3d_flow_params* params, int silent, float* device_seconds)
{
  g_host_error.clear();
  if (!flow || !params) return HostFail("f3d_flow_compute_resident_from_initial: null argument");
  flow->zncc_of_held_flow = false;
  f3d_flow_params p = *params;
  OperationParameters bag;
  FillBag(bag, p);
  flow->driver.silent = silent != 0;
  if (!flow->driver.ComputeFlowResident(bag, true)) {
    const std::string& why = flow->driver.InitialFlowError();
    return HostFail(why.empty() ? "f3d_flow_compute_resident_from_initial: the solve could not run (f3d_flow_upload first)" : why.c_str());
  }
  if (device_seconds) *device_seconds = flow->driver.LastDeviceSeconds();
  return 0;
}

int f3d_flow_compute_from_initial(f3d_flow flow, const float* frame_0, const float* frame_1, const f3d_flow_params* params, int silent,
                                  float* u, float* v, float* w)
{
  g_host_error.clear();
  if (!flow || !frame_0 || !frame_1 || !params || !u || !v || !w) return HostFail("f3d_flow_compute_from_initial: null argument");
  const DataSize4& c = flow->driver.ContainerSize();
  Data3D f0(const_cast<float*>(frame_0), c.width, c.height, c.depth);
  Data3D f1(const_cast<float*>(frame_1), c.width, c.height, c.depth);
  Data3D fu(u, c.width, c.height, c.depth), fv(v, c.width, c.height, c.depth), fw(w, c.width, c.height, c.depth);
  f3d_flow_params p = *params;
  OperationParameters bag;
  FillBag(bag, p);
  flow->driver.silent = silent != 0;
  if (!flow->driver.ComputeFlow(f0, f1, fu, fv, fw, bag, true)) {
    const std::string& why = flow->driver.InitialFlowError();
    return HostFail(why.empty() ? "f3d_flow_compute_from_initial: the solve could not run" : why.c_str());
  }
  return 0;
}

namespace {

// the checks every f3d_flow_*_compute makes of its driver, its source and the trajectory; `who` is the entry point's name
bool DerivedSource(f3d_flow flow, int source, bool have_out, const char* who, OpticalFlowE::Displacement* of)
{
  g_host_error.clear();
  const std::string name(who);
  if (!flow || !have_out) return !HostFail((name + ": null argument").c_str());
  if (source != F3D_STRAIN_OF_FLOW && source != F3D_STRAIN_OF_TRAJECTORY)
    return !HostFail((name + ": source must be F3D_STRAIN_OF_FLOW or F3D_STRAIN_OF_TRAJECTORY").c_str());
  if (source == F3D_STRAIN_OF_TRAJECTORY && !flow->trajectory_started)
    return !HostFail((name + ": no trajectory is active (f3d_flow_trajectory_begin first)").c_str());
  *of = source == F3D_STRAIN_OF_FLOW ? OpticalFlowE::HeldFlow() : OpticalFlowE::Trajectory();
  return true;
}

// the result of a Compute, then out[0 .. count) viewed as volumes of the container's size and the selected fields downloaded
int DerivedDownload(f3d_flow flow, OpticalFlowE::Derived which, bool computed, float* const* out, unsigned fields)
{
  OpticalFlowE& d = flow->driver;
  if (!computed) return HostFail(d.DerivedError(which).c_str());
  const DataSize4& c = d.ContainerSize();
  std::unique_ptr<Data3D> views[OpticalFlowE::kMaxDerivedFields];
  Data3D* dst[OpticalFlowE::kMaxDerivedFields] = {};
  for (int i = 0; i < OpticalFlowE::DerivedFieldCount(which); ++i)
    if (out[i]) {
      views[i].reset(new Data3D(out[i], c.width, c.height, c.depth));
      dst[i] = views[i].get();
    }
  return d.DownloadDerived(which, dst, fields) ? 0 : HostFail(d.DerivedError(which).c_str());
}

int DerivedEnd(f3d_flow flow, OpticalFlowE::Derived which, const char* null_driver)
{
  g_host_error.clear();
  if (!flow) return HostFail(null_driver);
  flow->driver.ReleaseDerived(which);
  return 0;
}

}  // namespace

int f3d_flow_strain_compute(f3d_flow flow, int source, unsigned fields, float* const out[8], f3d_strain_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out != nullptr, "f3d_flow_strain_compute", &of)) return 1;
  return DerivedDownload(flow, OpticalFlowE::kStrain, flow->driver.ComputeStrain(of, fields, stats), out, fields);
}

int f3d_flow_strain_end(f3d_flow flow) { return DerivedEnd(flow, OpticalFlowE::kStrain, "f3d_flow_strain_end: null driver"); }

int f3d_flow_window_strain_compute(f3d_flow flow, int source, unsigned fields, unsigned radius, unsigned min_count,
                                   float* const out[17], f3d_window_strain_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out != nullptr, "f3d_flow_window_strain_compute", &of)) return 1;
  return DerivedDownload(flow, OpticalFlowE::kWindowStrain, flow->driver.ComputeWindowStrain(of, fields, radius, min_count, stats), out,
                         fields);
}

int f3d_flow_window_strain_end(f3d_flow flow)
{
  return DerivedEnd(flow, OpticalFlowE::kWindowStrain, "f3d_flow_window_strain_end: null driver");
}

int f3d_flow_principal_compute(f3d_flow flow, int source, unsigned fields, float* const out[10], f3d_principal_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out != nullptr, "f3d_flow_principal_compute", &of)) return 1;
  return DerivedDownload(flow, OpticalFlowE::kPrincipal, flow->driver.ComputePrincipal(of, fields, stats), out, fields);
}

int f3d_flow_principal_end(f3d_flow flow) { return DerivedEnd(flow, OpticalFlowE::kPrincipal, "f3d_flow_principal_end: null driver"); }

int f3d_flow_polar_compute(f3d_flow flow, int source, unsigned fields, float* const out[7], f3d_polar_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out != nullptr, "f3d_flow_polar_compute", &of)) return 1;
  return DerivedDownload(flow, OpticalFlowE::kPolar, flow->driver.ComputePolar(of, fields, stats), out, fields);
}

int f3d_flow_polar_end(f3d_flow flow) { return DerivedEnd(flow, OpticalFlowE::kPolar, "f3d_flow_polar_end: null driver"); }

int f3d_flow_window_principal_compute(f3d_flow flow, int source, unsigned fields, unsigned radius, unsigned min_count,
                                      float* const out[10], f3d_principal_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out != nullptr, "f3d_flow_window_principal_compute", &of)) return 1;
  return DerivedDownload(flow, OpticalFlowE::kWindowPrincipal, flow->driver.ComputeWindowPrincipal(of, fields, radius, min_count, stats),
                         out, fields);
}

int f3d_flow_window_principal_end(f3d_flow flow)
{
  return DerivedEnd(flow, OpticalFlowE::kWindowPrincipal, "f3d_flow_window_principal_end: null driver");
}

int f3d_flow_window_polar_compute(f3d_flow flow, int source, unsigned fields, unsigned radius, unsigned min_count, float* const out[7],
                                  f3d_polar_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out != nullptr, "f3d_flow_window_polar_compute", &of)) return 1;
  return DerivedDownload(flow, OpticalFlowE::kWindowPolar, flow->driver.ComputeWindowPolar(of, fields, radius, min_count, stats), out,
                         fields);
}

int f3d_flow_window_polar_end(f3d_flow flow)
{
  return DerivedEnd(flow, OpticalFlowE::kWindowPolar, "f3d_flow_window_polar_end: null driver");
}

int f3d_flow_inverse_compute(f3d_flow flow, int source, unsigned iterations, float tolerance, float* const out[4],
                             f3d_inverse_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out && out[0] && out[1] && out[2] && out[3], "f3d_flow_inverse_compute", &of)) return 1;
  return DerivedDownload(flow, OpticalFlowE::kInverse, flow->driver.ComputeInverse(of, iterations, tolerance, stats), out, 1);
}

int f3d_flow_inverse_end(f3d_flow flow) { return DerivedEnd(flow, OpticalFlowE::kInverse, "f3d_flow_inverse_end: null driver"); }

static_assert(F3D_MATCH_WARPED == OpticalFlowE::kMatchWarped && F3D_MATCH_ZNCC == OpticalFlowE::kMatchZncc &&
                  F3D_MATCH_RMSD == OpticalFlowE::kMatchRmsd, "f3d_host.h and optical_flow.h name the match fields alike");

int f3d_flow_match_compute(f3d_flow flow, int source, unsigned fields, unsigned radius, float threshold, float* const out[3],
                           f3d_correlation_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out != nullptr, "f3d_flow_match_compute", &of)) return 1;
  const bool computed = flow->driver.ComputeMatch(of, 0, 0, fields, radius, threshold, stats);
  // the kernel stores zncc unless rmsd alone was asked for
  if (computed && ((fields & F3D_MATCH_ZNCC) || !(fields & F3D_MATCH_RMSD))) flow->zncc_of_held_flow = true;
  return DerivedDownload(flow, OpticalFlowE::kMatch, computed, out, fields);
}

int f3d_flow_match_end(f3d_flow flow)
{
  if (flow) flow->zncc_of_held_flow = false;
  return DerivedEnd(flow, OpticalFlowE::kMatch, "f3d_flow_match_end: null driver");
}

int f3d_motion_solve(const struct f3d_motion_sums* sums, int model, f3d_motion_fit* fit)
{
  g_host_error.clear();
  if (!sums || !fit) return HostFail("f3d_motion_solve: null argument");
  std::string why;
  return SolveMotion(*sums, model, fit, &why) ? 0 : HostFail(why.c_str());
}

int f3d_motion_solve_labels(const struct f3d_motion_sums* sums, size_t n_labels, int model, unsigned long long min_voxels,
                            const double volume_centre[3], f3d_motion_fit* fits, int* status)
{
  g_host_error.clear();
  if (!sums || !volume_centre || !fits || !status) return HostFail("f3d_motion_solve_labels: null argument");
  std::string why;
  return SolveLabelMotions(sums, n_labels, model, min_voxels, volume_centre, fits, status, &why) ? 0 : HostFail(why.c_str());
}

int f3d_flow_motion_compute(f3d_flow flow, int source, int model, float min_zncc, float* const out[3], f3d_motion_fit* fit,
                            f3d_motion_residual* residual)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out && out[0] && out[1] && out[2] && fit, "f3d_flow_motion_compute", &of)) return 1;
  DevicePtr weight = 0;
  if (min_zncc == min_zncc) {
    if (source == F3D_STRAIN_OF_TRAJECTORY)
      return HostFail("f3d_flow_motion_compute: min_zncc cannot mask the trajectory: the zncc of a match lives on the pair's grid");
    weight = flow->zncc_of_held_flow ? flow->driver.DerivedContainer(OpticalFlowE::kMatch, 1) : 0;
    if (!weight) return HostFail("f3d_flow_motion_compute: min_zncc needs the zncc of a match of this pair (f3d_flow_match_compute first)");
  }
  return DerivedDownload(flow, OpticalFlowE::kMotion, flow->driver.ComputeMotion(of, model, weight, min_zncc, fit, residual), out, 1);
}

int f3d_flow_motion_end(f3d_flow flow) { return DerivedEnd(flow, OpticalFlowE::kMotion, "f3d_flow_motion_end: null driver"); }

int f3d_flow_label_motion_compute(f3d_flow flow, int source, const int* labels, size_t n_labels, int model, unsigned long long min_voxels,
                                  float* const out[3], f3d_motion_fit* fits, int* status, double* rms_after, f3d_label_info* info)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out && out[0] && out[1] && out[2] && fits && status, "f3d_flow_label_motion_compute", &of)) return 1;
  OpticalFlowE& d = flow->driver;
  if (labels && !d.UploadLabels(labels)) return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  float* const four[4] = {out[0], out[1], out[2], nullptr};
  return DerivedDownload(flow, OpticalFlowE::kLabelMotion, d.ComputeLabelMotion(of, n_labels, model, min_voxels, fits, status, rms_after, info),
                         four, 1);
}

int f3d_flow_label_motion_end(f3d_flow flow)
{
  return DerivedEnd(flow, OpticalFlowE::kLabelMotion, "f3d_flow_label_motion_end: null driver");
}

int f3d_contact_kinematics(const struct f3d_contact* contacts, size_t n, const size_t dims[3], const f3d_motion_fit* fits, const int* status,
                           size_t n_labels, unsigned long long min_faces, f3d_contact_kin* out)
{
  g_host_error.clear();
  if ((n && !contacts) || !dims || !out) return HostFail("f3d_contact_kinematics: null argument");
  if ((fits == nullptr) != (status == nullptr)) return HostFail("f3d_contact_kinematics: fits and status need each other");
  std::string why;
  return ContactKinematics(contacts, n, dims, fits, status, n_labels, min_faces, out, &why) ? 0 : HostFail(why.c_str());
}

int f3d_flow_contacts_compute(f3d_flow flow, int source, const int* labels, size_t n_labels, const struct f3d_contact** contacts,
                              size_t* count, f3d_contact_info* info)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, contacts && count && info, "f3d_flow_contacts_compute", &of)) return 1;
  OpticalFlowE& d = flow->driver;
  if (labels && !d.UploadLabels(labels)) return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  if (!d.ComputeContacts(of, n_labels, &flow->contacts, info)) return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  *contacts = flow->contacts.data();
  *count = flow->contacts.size();
  return 0;
}

int f3d_flow_contacts_end(f3d_flow flow)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_contacts_end: null driver");
  std::vector<f3d_contact>().swap(flow->contacts);
  return 0;
}

int f3d_label_shape_solve(const struct f3d_label_shape_sums* sums, size_t n_labels, f3d_label_shape* out)
{
  g_host_error.clear();
  if (n_labels && (!sums || !out)) return HostFail("f3d_label_shape_solve: null argument");
  SolveLabelShapes(sums, n_labels, out);
  return 0;
}

int f3d_flow_label_shapes_compute(f3d_flow flow, const int* labels, size_t n_labels, f3d_label_shape* shapes, f3d_label_shape_info* info)
{
  g_host_error.clear();
  if (!flow || !shapes) return HostFail("f3d_flow_label_shapes_compute: null argument");
  OpticalFlowE& d = flow->driver;
  if (labels && !d.UploadLabels(labels)) return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  if (!d.ComputeLabelShapes(n_labels, shapes, info)) return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_flow_labels_compute(f3d_flow flow, f3d_devptr frame, float lo, float hi, unsigned long long min_voxels,
                            const unsigned long long** sizes, size_t* count, f3d_component_info* info)
{
  g_host_error.clear();
  if (!flow || !sizes || !count || !info) return HostFail("f3d_flow_labels_compute: null argument");
  OpticalFlowE& d = flow->driver;
  if (!d.ComputeLabels(frame, lo, hi, min_voxels, &flow->label_sizes, info))
    return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  *sizes = flow->label_sizes.data();
  *count = flow->label_sizes.size();
  return 0;
}

int f3d_flow_labels_split(f3d_flow flow, f3d_devptr frame, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels,
                          const unsigned long long** sizes, size_t* count, f3d_split_info* info)
{
  g_host_error.clear();
  if (!flow || !sizes || !count || !info) return HostFail("f3d_flow_labels_split: null argument");
  OpticalFlowE& d = flow->driver;
  if (!d.ComputeSplitLabels(frame, lo, hi, core_d2, min_voxels, &flow->label_sizes, info))
    return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  *sizes = flow->label_sizes.data();
  *count = flow->label_sizes.size();
  return 0;
}

int f3d_flow_labels_end(f3d_flow flow)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_labels_end: null driver");
  std::vector<unsigned long long>().swap(flow->label_sizes);
  std::vector<unsigned long long>().swap(flow->label_b_sizes);
  return 0;
}

int f3d_flow_labels_download(f3d_flow flow, int* labels)
{
  g_host_error.clear();
  if (!flow || !labels) return HostFail("f3d_flow_labels_download: null argument");
  if (!flow->driver.DownloadLabels(labels)) return HostFail(flow->driver.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_overlap_solve(const struct f3d_overlap* rows, size_t count, size_t n_a, size_t n_b, double min_fraction, f3d_track_a* a,
                      f3d_track_b* b, int* map_b, f3d_track_summary* summary)
{
  g_host_error.clear();
  if ((count && !rows) || !a || !b || !map_b) return HostFail("f3d_overlap_solve: null argument");
  if (n_a == 0 || n_b == 0) return HostFail("f3d_overlap_solve: n_a and n_b must be at least 1");
  std::string why;
  return SolveOverlaps(rows, count, n_a, n_b, min_fraction, a, b, map_b, summary, &why) ? 0 : HostFail(why.c_str());
}

int f3d_block_match_solve(const f3d_block_match_record* records, const f3d_block_match_grid* grid, const int* centre, double min_zncc,
                          f3d_block_match_node* nodes, f3d_block_match_summary* summary)
{
  g_host_error.clear();
  if (!records || !grid || !nodes) return HostFail("f3d_block_match_solve: null argument");
  std::string why;
  return SolveBlockMatch(records, grid, centre, min_zncc, nodes, summary, &why) ? 0 : HostFail(why.c_str());
}

int f3d_block_match_layout(size_t width, size_t height, size_t depth, int step, int window, int rx, int ry, int rz,
                           f3d_block_match_grid* grid)
{
  g_host_error.clear();
  if (!grid) return HostFail("f3d_block_match_layout: null argument");
  std::string why;
  return LayoutBlockMatch(width, height, depth, step, window, rx, ry, rz, grid, &why) ? 0 : HostFail(why.c_str());
}

int f3d_subset_match_table(const f3d_subset_match_record* records, const f3d_subset_match_grid* grid, double min_zncc,
                           const float* const* compare, f3d_subset_match_node* nodes, f3d_subset_match_summary* summary)
{
  g_host_error.clear();
  if (!records || !grid || !nodes) return HostFail("f3d_subset_match_table: null argument");
  std::string why;
  return TableSubsetMatch(records, grid, min_zncc, compare, nodes, summary, &why) ? 0 : HostFail(why.c_str());
}

int f3d_subset_match_layout(size_t width, size_t height, size_t depth, int step, int window, f3d_subset_match_grid* grid)
{
  g_host_error.clear();
  if (!grid) return HostFail("f3d_subset_match_layout: null argument");
  std::string why;
  return LayoutSubsetMatch(width, height, depth, step, window, grid, &why) ? 0 : HostFail(why.c_str());
}

int f3d_flow_subset_match(f3d_flow flow, int step, int window, int model, int start, int max_iterations, double tolerance, double reach,
                          double min_zncc, f3d_subset_match_grid* grid, f3d_subset_match_info* info, f3d_subset_match_summary* summary)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_subset_match: null driver");
  OpticalFlowE::SubsetMatchParams p;
  p.step = step;
  p.window = window;
  p.model = model;
  p.start = start;
  p.max_iterations = max_iterations;
  p.tolerance = tolerance;
  p.reach = reach;
  p.min_zncc = min_zncc;
  if (!flow->driver.SubsetMatch(p, info, summary)) return HostFail(flow->driver.InitialFlowError().c_str());
  if (grid) *grid = flow->driver.SubsetMatchGrid();
  return 0;
}

int f3d_flow_subset_match_rows(f3d_flow flow, size_t capacity, f3d_subset_match_record* records, f3d_subset_match_node* nodes)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_subset_match_rows: null driver");
  const std::vector<f3d_subset_match_node>& rows = flow->driver.SubsetMatchNodes();
  if (rows.empty()) return HostFail("f3d_flow_subset_match_rows: no node table is held (f3d_flow_subset_match first)");
  if (rows.size() > capacity) return HostFail("f3d_flow_subset_match_rows: the table has more nodes than there is room for");
  if (records) std::memcpy(static_cast<void*>(records), flow->driver.SubsetMatchRecords().data(), rows.size() * sizeof(f3d_subset_match_record));
  if (nodes) std::memcpy(static_cast<void*>(nodes), rows.data(), rows.size() * sizeof(f3d_subset_match_node));
  return 0;
}

int f3d_flow_block_match(f3d_flow flow, int step, int window, int rx, int ry, int rz, size_t bins, const float* range, const int* centre,
                         double min_zncc, f3d_block_match_grid* grid, f3d_block_match_info* info, f3d_block_match_summary* summary)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_block_match: null driver");
  OpticalFlowE::BlockMatchParams p;
  p.step = step;
  p.window = window;
  p.radius[0] = rx, p.radius[1] = ry, p.radius[2] = rz;
  p.bins = bins;
  p.range = range;
  p.min_zncc = min_zncc;
  if (!flow->driver.BlockMatch(p, centre, info, summary)) return HostFail(flow->driver.InitialFlowError().c_str());
  if (grid) *grid = flow->driver.BlockMatchGrid();
  return 0;
}

int f3d_flow_block_match_rows(f3d_flow flow, size_t capacity, f3d_block_match_record* records, f3d_block_match_node* nodes)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_block_match_rows: null driver");
  const std::vector<f3d_block_match_node>& rows = flow->driver.BlockMatchNodes();
  if (rows.empty()) return HostFail("f3d_flow_block_match_rows: no node table is held (f3d_flow_block_match first)");
  if (rows.size() > capacity) return HostFail("f3d_flow_block_match_rows: the table has more nodes than there is room for");
  if (records) std::memcpy(records, flow->driver.BlockMatchRecords().data(), rows.size() * sizeof(f3d_block_match_record));
  if (nodes) std::memcpy(static_cast<void*>(nodes), rows.data(), rows.size() * sizeof(f3d_block_match_node));
  return 0;
}

int f3d_flow_initial_from_nodes(f3d_flow flow, f3d_validate_stats* validated, f3d_initial_info* info)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_initial_from_nodes: null driver");
  if (!flow->driver.SetInitialFromNodes(validated, info)) return HostFail(flow->driver.InitialFlowError().c_str());
  return 0;
}

int f3d_flow_labels_b_upload(f3d_flow flow, const int* labels)
{
  g_host_error.clear();
  if (!flow || !labels) return HostFail("f3d_flow_labels_b_upload: null argument");
  if (!flow->driver.UploadLabelsB(labels)) return HostFail(flow->driver.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_flow_labels_b_segment(f3d_flow flow, f3d_devptr frame, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels,
                              const unsigned long long** sizes, size_t* count, f3d_split_info* info)
{
  g_host_error.clear();
  if (!flow || !sizes || !count || !info) return HostFail("f3d_flow_labels_b_segment: null argument");
  OpticalFlowE& d = flow->driver;
  if (!d.ComputeLabelsB(frame, lo, hi, core_d2, min_voxels, &flow->label_b_sizes, info))
    return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  *sizes = flow->label_b_sizes.data();
  *count = flow->label_b_sizes.size();
  return 0;
}

int f3d_flow_overlap_compute(f3d_flow flow, int source, size_t n_a, size_t n_b, const struct f3d_overlap** rows, size_t* count,
                             f3d_overlap_info* info)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, rows && count && info, "f3d_flow_overlap_compute", &of)) return 1;
  OpticalFlowE& d = flow->driver;
  if (!d.ComputeOverlap(of, n_a, n_b, &flow->overlaps, info)) return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  *rows = flow->overlaps.data();
  *count = flow->overlaps.size();
  return 0;
}

int f3d_flow_overlap_end(f3d_flow flow)
{
  g_host_error.clear();
  if (!flow) return HostFail("f3d_flow_overlap_end: null driver");
  std::vector<f3d_overlap>().swap(flow->overlaps);
  return 0;
}

int f3d_flow_labels_b_relabel(f3d_flow flow, const int* map, size_t n_b)
{
  g_host_error.clear();
  if (!flow || !map) return HostFail("f3d_flow_labels_b_relabel: null argument");
  if (!flow->driver.RelabelB(map, n_b)) return HostFail(flow->driver.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_flow_labels_b_download(f3d_flow flow, int* labels)
{
  g_host_error.clear();
  if (!flow || !labels) return HostFail("f3d_flow_labels_b_download: null argument");
  if (!flow->driver.DownloadLabelsB(labels)) return HostFail(flow->driver.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_label_field_solve(const struct f3d_label_field_sums* sums, const unsigned* counts, size_t n_labels, int shift, float lo, float hi,
                          size_t bins, unsigned long long min_voxels, f3d_label_field_stat* stats, f3d_label_field_summary* summary)
{
  g_host_error.clear();
  std::string why;
  return SolveLabelField(sums, counts, n_labels, shift, lo, hi, bins, min_voxels, stats, summary, &why)
             ? 0
             : HostFail(("f3d_label_field_solve: " + why).c_str());
}

int f3d_flow_label_field_compute(f3d_flow flow, f3d_devptr field, size_t n_labels, int shift, const float* range, size_t bins,
                                 unsigned long long min_voxels, f3d_label_field_stat* stats, unsigned* counts, f3d_label_field_info* info,
                                 f3d_label_field_summary* summary)
{
  g_host_error.clear();
  if (!flow || !stats) return HostFail("f3d_flow_label_field_compute: null argument");
  OpticalFlowE& d = flow->driver;
  if (!d.ComputeLabelField(field, n_labels, shift, range, bins, min_voxels, stats, counts, info, summary))
    return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_label_field_shift(float min, float max, unsigned long long finite) { return LabelFieldShift(min, max, finite); }

int f3d_flow_label_field_range(f3d_flow flow, f3d_devptr field, float* min, float* max, f3d_range_info* info)
{
  g_host_error.clear();
  if (!flow || !min || !max || !info) return HostFail("f3d_flow_label_field_range: null argument");
  if (!flow->driver.LabelFieldRange(field, min, max, info)) return HostFail(flow->driver.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_flow_field_container(f3d_flow flow, const char* name, f3d_devptr* container)
{
  g_host_error.clear();
  if (!flow || !name || !container) return HostFail("f3d_flow_field_container: null argument");
  const f3d_devptr found = flow->driver.NamedField(name);
  if (!found) return HostFail((std::string("f3d_flow_field_container: no field '") + name + "' on the device (not a name, or not computed)").c_str());
  *container = found;
  return 0;
}

int f3d_flow_labels_paint(f3d_flow flow, const float* values, size_t n_labels, float* out)
{
  g_host_error.clear();
  if (!flow || !values || !out) return HostFail("f3d_flow_labels_paint: null argument");
  if (!flow->driver.PaintLabels(values, n_labels, out)) return HostFail(flow->driver.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_histogram_edge(float lo, float hi, size_t bins, size_t k, float* edge)
{
  g_host_error.clear();
  std::string why;
  return HistogramEdge(lo, hi, bins, k, edge, &why) ? 0 : HostFail(("f3d_histogram_edge: " + why).c_str());
}

int f3d_otsu(const unsigned long long* counts, size_t bins, int classes, unsigned* cuts, f3d_otsu_info* info)
{
  g_host_error.clear();
  std::string why;
  return OtsuCuts(counts, bins, classes, cuts, info, &why) ? 0 : HostFail(("f3d_otsu: " + why).c_str());
}

int f3d_histogram_rank(const unsigned long long* counts, size_t bins, unsigned long long r, unsigned* bin)
{
  g_host_error.clear();
  std::string why;
  return HistogramRank(counts, bins, r, bin, &why) ? 0 : HostFail(("f3d_histogram_rank: " + why).c_str());
}

int f3d_flow_histogram(f3d_flow flow, f3d_devptr frame, const float* range, size_t bins, unsigned long long* counts,
                       f3d_histogram_info* info, float* lo_used, float* hi_used)
{
  g_host_error.clear();
  if (!flow || !counts || !info) return HostFail("f3d_flow_histogram: null argument");
  OpticalFlowE& d = flow->driver;
  if (!d.ComputeHistogram(frame, range, bins, counts, info, lo_used, hi_used))
    return HostFail(d.DerivedError(OpticalFlowE::kLabelMotion).c_str());
  return 0;
}

int f3d_flow_validate_compute(f3d_flow flow, int source, unsigned step, float eps, float threshold, unsigned min_neighbours,
                              unsigned mode, unsigned fill_passes, float min_zncc, float* const out[4], f3d_validate_stats* stats)
{
  OpticalFlowE::Displacement of;
  if (!DerivedSource(flow, source, out != nullptr, "f3d_flow_validate_compute", &of)) return 1;
  const int d_given = (out[1] ? 1 : 0) + (out[2] ? 1 : 0) + (out[3] ? 1 : 0);
  if (d_given != 0 && d_given != 3) return HostFail("f3d_flow_validate_compute: out[1], out[2] and out[3] go together");
  const unsigned fields = (out[0] ? F3D_VALIDATE_R : 0u) | (d_given ? F3D_VALIDATE_D : 0u);
  if (!fields) return HostFail("f3d_flow_validate_compute: no output is asked for");
  DevicePtr weight = 0;
  if (min_zncc == min_zncc) {
    if (source == F3D_STRAIN_OF_TRAJECTORY)
      return HostFail("f3d_flow_validate_compute: min_zncc cannot mask the trajectory: the zncc of a match lives on the pair's grid");
    weight = flow->zncc_of_held_flow ? flow->driver.DerivedContainer(OpticalFlowE::kMatch, 1) : 0;
    if (!weight)
      return HostFail("f3d_flow_validate_compute: min_zncc needs the zncc of a match of this pair (f3d_flow_match_compute first)");
  }
  return DerivedDownload(flow, OpticalFlowE::kValidated,
                         flow->driver.ComputeValidated(of, weight, min_zncc, step, eps, threshold, min_neighbours, mode, fill_passes,
                                                       fields, stats),
                         out, fields);
}

int f3d_flow_validate_end(f3d_flow flow) { return DerivedEnd(flow, OpticalFlowE::kValidated, "f3d_flow_validate_end: null driver"); }

const char* f3d_host_last_error(void) { return g_host_error.empty() ? f3d_last_error() : g_host_error.c_str(); }

int f3d_flow_destroy(f3d_flow flow)
{
  delete flow;
  return 0;
}

int f3d_op_create(f3d_op* op, const char* name)
{
  if (!op || !name) return 1;
  const std::string n(name);
  CudaOperationBase* impl = nullptr;
  if (n == "add") impl = new CudaOperationAdd;
  else if (n == "convolution") impl = new CudaOperationConvolution3D;
  else if (n == "median") impl = new CudaOperationMedian;
  else if (n == "registration") impl = new CudaOperationRegistration;
  else if (n == "resample") impl = new CudaOperationResample;
  else if (n == "solve") impl = new CudaOperationSolve;
  else if (n == "stat") impl = new CudaOperationStat;
  else if (n == "add_p") impl = new CudaOperationAddP;
  else if (n == "resample_p") impl = new CudaOperationResampleP;
  else if (n == "registration_p") impl = new CudaOperationRegistrationP;
  else if (n == "solve_p") impl = new CudaOperationSolveP;
  else if (n == "stat_p") impl = new CudaOperationStatP;
  else if (n == "convolution_p") impl = new CudaOperationConvolution3DP;
  else if (n == "median_p") impl = new CudaOperationMedianP;
  if (!impl) return 1;
  *op = new f3d_op_s;
  (*op)->op = impl;
  return 0;
}

const char* f3d_op_name(f3d_op op) { return op ? op->op->GetName() : ""; }

int f3d_op_initialize(f3d_op op, const f3d_size4* container_size)
{
  if (!op) return 1;
  if (!container_size) return op->op->Initialize(nullptr) ? 0 : 1;
  DataSize4 c = {container_size->width, container_size->height, container_size->depth, container_size->pitch};
  OperationParameters bag;
  bag.PushValuePtr("container_size", &c);
  return op->op->Initialize(&bag) ? 0 : 1;
}

int f3d_op_execute(f3d_op op, const char* const* keys, void* const* value_ptrs, size_t count)
{
  if (!op) return 1;
  OperationParameters bag;
  for (size_t i = 0; i < count; ++i) bag.PushValuePtr(keys[i], value_ptrs[i]);
  if (auto* solve = dynamic_cast<CudaOperationSolve*>(op->op)) solve->silent = true;
  if (auto* solve_p = dynamic_cast<CudaOperationSolveP*>(op->op)) solve_p->silent = true;
  if (auto* stat_p = dynamic_cast<CudaOperationStatP*>(op->op)) stat_p->silent = true;
  op->op->Execute(bag);
  return 0;
}

int f3d_op_execute_batch(f3d_op op, const char* const* keys, void* const* value_ptrs, const size_t* counts, size_t bags)
{
  if (!op || !counts || bags == 0) return 1;
  std::vector<OperationParameters> bag(bags);
  size_t at = 0;
  for (size_t b = 0; b < bags; ++b)
    for (size_t i = 0; i < counts[b]; ++i, ++at) bag[b].PushValuePtr(keys[at], value_ptrs[at]);
  if (auto* add = dynamic_cast<CudaOperationAdd*>(op->op)) return add->ExecuteBatch(bag.data(), bags), 0;
  if (auto* median = dynamic_cast<CudaOperationMedian*>(op->op)) return median->ExecuteBatch(bag.data(), bags), 0;
  if (auto* resample = dynamic_cast<CudaOperationResample*>(op->op)) return resample->ExecuteBatch(bag.data(), bags), 0;
  return 1;  // the other operators take one bag at a time
}

int f3d_op_set_slab(f3d_op op, const f3d_slab* slab)
{
  if (!op) return 1;
  op->op->SetSlab(slab);
  return 0;
}

int f3d_op_destroy(f3d_op op)
{
  if (op) op->op->Destroy();
  delete op;
  return 0;
}

int f3d_op_solve_p_last(f3d_op op, int* chunk, int* outer_per_pass, int* halo, size_t* passes, int* overlapped)
{
  auto* solve_p = op ? dynamic_cast<CudaOperationSolveP*>(op->op) : nullptr;
  if (!solve_p) return 1;
  if (chunk) *chunk = solve_p->LastPlan().chunk;
  if (outer_per_pass) *outer_per_pass = solve_p->LastPlan().outer_per_pass;
  if (halo) *halo = solve_p->LastPlan().halo;
  if (passes) *passes = solve_p->LastPasses();
  if (overlapped) *overlapped = solve_p->LastPlan().overlapped ? 1 : 0;
  return 0;
}

int f3d_op_solve_p_fused_weights(f3d_op op, int* fused)
{
  auto* solve_p = op ? dynamic_cast<CudaOperationSolveP*>(op->op) : nullptr;
  if (!solve_p || !fused) return 1;
  *fused = solve_p->LastFusedWeights() ? 1 : 0;
  return 0;
}

int f3d_volume_wrap(f3d_volume* vol, float* data, size_t width, size_t height, size_t depth)
{
  if (!vol || !data || width == 0 || height == 0 || depth == 0) return 1;
  *vol = new (std::nothrow) f3d_volume_s(data, width, height, depth);
  return *vol ? 0 : 1;
}

void* f3d_volume_object(f3d_volume vol) { return vol ? &vol->view : nullptr; }

float* f3d_volume_data(f3d_volume vol) { return vol ? vol->view.DataPtr() : nullptr; }

int f3d_volume_destroy(f3d_volume vol)
{
  delete vol;
  return 0;
}

int f3d_pflow_create(f3d_pflow* flow)
{
  if (!flow) return 1;
  *flow = new (std::nothrow) f3d_pflow_s;
  return *flow ? 0 : 1;
}

int f3d_pflow_initialize(f3d_pflow flow, size_t width, size_t height, size_t depth)
{
  if (!flow) return 1;
  if (f3d_init(-1) != 0) {
    std::fprintf(stderr, "f3d_pflow_initialize: %s\n", f3d_last_error());
    return 1;
  }
  DataSize4 size = {width, height, depth, 0};
  return flow->driver.Initialize(size) ? 0 : 1;
}

int f3d_pflow_compute(f3d_pflow flow, const float* frame_0, const float* frame_1, size_t width, size_t height, size_t depth,
                      const f3d_flow_params* params, int silent, float* u, float* v, float* w, float* device_seconds)
{
  if (!flow || !frame_0 || !frame_1 || !params || !u || !v || !w) return 1;
  Data3D f0(const_cast<float*>(frame_0), width, height, depth), f1(const_cast<float*>(frame_1), width, height, depth);
  Data3D fu(u, width, height, depth), fv(v, width, height, depth), fw(w, width, height, depth);
  f3d_flow_params p = *params;
  OperationParameters bag;
  FillBag(bag, p);
  flow->driver.silent = silent != 0;
  flow->driver.ComputeFlow(f0, f1, fu, fv, fw, bag);
  if (device_seconds) *device_seconds = flow->driver.LastDeviceSeconds();
  // the driver hands every caller volume its own storage back; anything else would lose the result
  return (f0.DataPtr() == frame_0 && f1.DataPtr() == frame_1 && fu.DataPtr() == u && fv.DataPtr() == v && fw.DataPtr() == w) ? 0 : 1;
}

int f3d_pflow_stats(f3d_pflow flow, size_t* solve_passes, size_t* streamed_levels, size_t* resident_levels)
{
  if (!flow) return 1;
  if (solve_passes) *solve_passes = flow->driver.LastSolvePasses();
  if (streamed_levels) *streamed_levels = flow->driver.LastStreamedLevels();
  if (resident_levels) *resident_levels = flow->driver.LastResidentLevels();
  return 0;
}

int f3d_pflow_levels_registered_inside(f3d_pflow flow, size_t* levels)
{
  if (!flow || !levels) return 1;
  *levels = flow->driver.LastLevelsRegisteredInside();
  return 0;
}

int f3d_pflow_levels_with_constants_on_device(f3d_pflow flow, size_t* levels)
{
  if (!flow || !levels) return 1;
  *levels = flow->driver.LastLevelsWithConstantsOnDevice();
  return 0;
}

int f3d_pflow_originals_on_device(f3d_pflow flow, int* yes)
{
  if (!flow || !yes) return 1;
  *yes = flow->driver.LastOriginalsOnDevice() ? 1 : 0;
  return 0;
}

int f3d_pflow_set_full_pipeline(f3d_pflow flow, int enabled)
{
  if (!flow) return 1;
  flow->driver.full_pipeline = enabled != 0;
  return 0;
}

int f3d_pflow_set_resident(f3d_pflow flow, int enabled)
{
  if (!flow) return 1;
  flow->driver.resident_coarse_levels = enabled != 0;
  return 0;
}

int f3d_pflow_operator_seconds(f3d_pflow flow, double* seconds6)
{
  if (!flow || !seconds6) return 1;
  for (int i = 0; i < 6; ++i) seconds6[i] = flow->driver.LastOperatorSeconds()[i];
  return 0;
}

int f3d_pflow_destroy(f3d_pflow flow)
{
  delete flow;
  return 0;
}

size_t f3d_piecemeal_budget_bytes(void) { return PiecemealBudgetBytes(); }

int f3d_plan_solve_piecemeal(size_t budget_bytes, size_t width, size_t height, int depth, int inner_iterations, int outer_iterations,
                             int forced_outer_per_pass, int overlap_mode, int* chunk, int* outer_per_pass, int* halo, int* max_planes,
                             int* overlapped)
{
  const SolvePiecemealPlan plan = PlanSolvePiecemeal(budget_bytes, width, height, depth, inner_iterations, outer_iterations,
                                                     forced_outer_per_pass, overlap_mode);
  if (overlapped) *overlapped = plan.overlapped ? 1 : 0;
  if (chunk) *chunk = plan.chunk;
  if (outer_per_pass) *outer_per_pass = plan.outer_per_pass;
  if (halo) *halo = plan.halo;
  if (max_planes) *max_planes = plan.max_planes;
  return 0;
}

int f3d_plan_sweeps(int inner, int fused, int tri, int carry, int* sweeps, int* next_weights, int capacity)
{
  const std::vector<SweepLaunch> cut = CutSweeps(inner, fused != 0, tri != 0, carry != 0);
  if (static_cast<int>(cut.size()) > capacity || (!cut.empty() && (!sweeps || !next_weights))) return -1;
  for (size_t i = 0; i < cut.size(); ++i) {
    sweeps[i] = cut[i].sweeps;
    next_weights[i] = cut[i].next_weights ? 1 : 0;
  }
  return static_cast<int>(cut.size());
}

int f3d_plan_sweeps_weights_first(int inner, int* first, int* sweeps, int* weights_first, int* next_weights, int capacity)
{
  const std::vector<SweepLaunch> cut = CutSweepsWeightsFirst(inner);
  if (static_cast<int>(cut.size()) > capacity || (!cut.empty() && (!first || !sweeps || !weights_first || !next_weights))) return -1;
  for (size_t i = 0; i < cut.size(); ++i) {
    first[i] = cut[i].first;
    sweeps[i] = cut[i].sweeps;
    weights_first[i] = cut[i].weights_first ? 1 : 0;
    next_weights[i] = cut[i].next_weights ? 1 : 0;
  }
  return static_cast<int>(cut.size());
}

int f3d_pair8_plan(int width, int rows, int planes, int ty, int zc_limit, int per_round, int fold, long long* plan)
{
  if (!plan || width < 1 || rows < 1 || planes < 1 || ty < 1 || zc_limit < 1) return 1;
  const Pair8Plan p = pair8_plan_dims(width, rows, planes, ty, zc_limit, per_round > 0 ? per_round : pair8_per_round(256), fold != 0);
  const long long v[8] = {p.cut.tiles_a, p.cut.chunks_a, p.cut.chunks_b, p.cut.zc_a, p.cut.zc_b, pair8_cut_wgs(p.cut), p.cost,
                          p.cut.tiles_a + p.cut.tiles_b};
  std::copy(v, v + 8, plan);
  return 0;
}

int f3d_solver_chunk_limit(unsigned long long plane_bytes, int reach) { return solver_chunk_limit(plane_bytes, reach); }

int f3d_pair8_decode(int width, int rows, int ty, int fold, const long long* plan, int xcd_remap, int z_lo, int z_hi, int first,
                     int count, int* out, int* grid)
{
  if (!plan || width < 1 || rows < 1 || ty < 1 || z_hi <= z_lo || first < 0 || count < 0 || (count && !out)) return 1;
  const int ntx = (width + kPair8Lanes - 1) / kPair8Lanes, nty = (rows + ty - 1) / ty;
  const int tiles = pair8_tiles_per_chunk(ntx, nty, fold != 0);
  const Pair8Cut cut = {static_cast<int>(plan[0]), static_cast<int>(plan[1]), static_cast<int>(plan[3]),
                        tiles - static_cast<int>(plan[0]), static_cast<int>(plan[2]), static_cast<int>(plan[4]), 0, 0, 0};
  if (cut.tiles_a < 0 || cut.tiles_b < 0 || (cut.tiles_a && (cut.chunks_a < 1 || cut.zc_a < 1)) ||
      (cut.tiles_b && (cut.chunks_b < 1 || cut.zc_b < 1)))
    return 1;
  if (grid) *grid = pair8_cut_grid(cut, xcd_remap);
  for (int i = 0; i < count; ++i) {
    Pair8Wg w;
    int* o = out + 6 * static_cast<size_t>(i);
    if (pair8_decode(first + i, cut, ntx, nty, fold != 0, xcd_remap, z_lo, z_hi, 0, w)) {
      o[0] = w.tile; o[1] = w.tx; o[2] = w.ty; o[3] = w.folded ? 1 : 0; o[4] = w.z0; o[5] = w.z1;
    } else {
      std::fill(o, o + 6, -1);
    }
  }
  return 0;
}

int f3d_pair8_plan_wide(int width, int rows, int planes, int ty, int zc_limit, int per_round, int fold, long long* plan)
{
  if (!plan || width < 1 || rows < 1 || planes < 1 || ty < 1 || zc_limit < 1) return 1;
  const Pair8Plan p = pair8_plan_launch(width, rows, planes, ty, zc_limit, per_round > 0 ? per_round : pair8_per_round(256), fold != 0);
  const Pair8Cut& c = p.cut;
  const long long v[12] = {c.tiles_a, c.chunks_a, c.zc_a, c.tiles_b, c.chunks_b, c.zc_b, c.tiles_c, c.chunks_c, c.zc_c,
                           pair8_cut_wgs(c), p.cost, c.tiles_a + c.tiles_b + c.tiles_c};
  std::copy(v, v + 12, plan);
  return 0;
}

int f3d_pair8_decode_wide(int width, int rows, int ty, int fold, const long long* plan, int xcd_remap, int z_lo, int z_hi, int first,
                          int count, int* out, int* grid)
{
  if (!plan || width < 1 || rows < 1 || ty < 1 || z_hi <= z_lo || first < 0 || count < 0 || (count && !out)) return 1;
  const int ntx = (width + kPair8Lanes - 1) / kPair8Lanes, nty = (rows + ty - 1) / ty;
  int v[9];
  for (int i = 0; i < 9; ++i) v[i] = static_cast<int>(plan[i]);
  const Pair8Cut cut = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
  for (int i = 0; i < 9; i += 3)   // a class is empty or has tiles, chunks and planes per chunk
    if (v[i] < 0 || (v[i] && (v[i + 1] < 1 || v[i + 2] < 1))) return 1;
  if (cut.tiles_a + cut.tiles_b + cut.tiles_c != pair8_tiles_per_chunk(ntx, nty, fold != 0)) return 1;
  if (grid) *grid = pair8_cut_grid(cut, xcd_remap);
  for (int i = 0; i < count; ++i) {
    Pair8Wg w;
    int* o = out + 6 * static_cast<size_t>(i);
    if (pair8_decode(first + i, cut, ntx, nty, fold != 0, xcd_remap, z_lo, z_hi, 0, w)) {
      o[0] = w.tile; o[1] = w.tx; o[2] = w.ty; o[3] = w.folded ? 1 : 0; o[4] = w.z0; o[5] = w.z1;
    } else {
      std::fill(o, o + 6, -1);
    }
  }
  return 0;
}

size_t f3d_max_warp_level(size_t width, size_t height, size_t depth, float scale_factor)
{
  return OpticalFlowBase::GetMaxWarpLevel(width, height, depth, scale_factor);
}

int f3d_level_geometry(size_t width, size_t height, size_t depth, float scale_factor, int level, f3d_size4* size,
                       float* hx, float* hy, float* hz)
{
  if (!size || !hx || !hy || !hz) return 1;
  DataSize4 original = {width, height, depth, 0};
  PyramidLevel lv = OpticalFlowBase::GetLevel(original, scale_factor, level);
  *size = {lv.size.width, lv.size.height, lv.size.depth, 0};
  *hx = lv.hx;
  *hy = lv.hy;
  *hz = lv.hz;
  return 0;
}

int f3d_gaussian_taps(float sigma, float* taps, size_t capacity, size_t* radius)
{
  if (!taps || !radius) return 1;
  CudaOperationConvolution3D conv;
  conv.ComputeGaussianKernel(sigma, 3, 1.0);
  const size_t n = 2 * conv.KernelRadius() + 1;
  if (n > capacity || n > 51) return 1;
  std::memcpy(taps, conv.Kernel(), n * sizeof(float));
  *radius = conv.KernelRadius();
  return 0;
}

int f3d_raw_read_u8(const char* path, size_t width, size_t height, size_t depth, float* out)
{
  Data3D vol;
  if (!vol.ReadRAWFromFileU8(path, width, height, depth)) return 1;
  std::memcpy(out, vol.DataPtr(), width * height * depth * sizeof(float));
  return 0;
}

int f3d_raw_read_f32(const char* path, size_t width, size_t height, size_t depth, float* out)
{
  Data3D vol;
  if (!vol.ReadRAWFromFileF32(path, width, height, depth)) return 1;
  std::memcpy(out, vol.DataPtr(), width * height * depth * sizeof(float));
  return 0;
}

int f3d_raw_write_u8(const char* path, const float* in, size_t width, size_t height, size_t depth)
{
  Data3D vol(const_cast<float*>(in), width, height, depth);
  return vol.WriteRAWToFileU8(path) ? 0 : 1;
}

int f3d_raw_write_f32(const char* path, const float* in, size_t width, size_t height, size_t depth)
{
  Data3D vol(const_cast<float*>(in), width, height, depth);
  return vol.WriteRAWToFileF32(path) ? 0 : 1;
}

int f3d_vtk_write_flow(const char* path, const float* u, const float* v, const float* w, size_t width, size_t height,
                       size_t depth)
{
  Data3D fu(const_cast<float*>(u), width, height, depth), fv(const_cast<float*>(v), width, height, depth),
      fw(const_cast<float*>(w), width, height, depth);
  return Data3D::WriteFlowToFileVTK(path, fu, fv, fw) ? 0 : 1;
}

int f3d_synth_pair(size_t width, size_t height, size_t depth, float* frame_0, float* frame_1)
{
  if (!frame_0 || !frame_1 || width == 0 || height == 0 || depth == 0) return 1;
  f3d_synth::TranslatedGaussianPair(width, height, depth, frame_0, frame_1);
  return 0;
}

int f3d_synth_planes(size_t width, size_t height, size_t depth, size_t z_lo, size_t z_hi, float* frame_0, float* frame_1,
                      float* frame_0_max)
{
  if (!frame_0 || !frame_1 || !frame_0_max || z_lo > z_hi || z_hi > depth) return 1;
  *frame_0_max = f3d_synth::TranslatedGaussianPlanes(width, height, depth, z_lo, z_hi, frame_0, frame_1);
  return 0;
}

int f3d_slabflow_create(f3d_slabflow* flow, int n_ranks, const int* local_ranks, int n_local, int halo_capacity)
{
  if (!flow || !local_ranks || n_local < 1 || n_ranks < 1) return 1;
  *flow = new (std::nothrow) f3d_slabflow_s;
  if (!*flow) return 1;
  (*flow)->driver = new OpticalFlowSlab(n_ranks, std::vector<int>(local_ranks, local_ranks + n_local),
                                        halo_capacity > 0 ? halo_capacity : 16);
  return 0;
}

int f3d_slabflow_initialize(f3d_slabflow flow, size_t width, size_t height, size_t depth)
{
  if (!flow) return 1;
  if (f3d_init(-1) != 0) {
    std::fprintf(stderr, "f3d_slabflow_initialize: %s\n", f3d_last_error());
    return 1;
  }
  DataSize4 size = {width, height, depth, 0};
  return flow->driver->Initialize(size) ? 0 : 1;
}

namespace {
struct FullVolumes {
  Data3D f0, f1;
  FullVolumes(const float* a, const float* b, size_t w, size_t h, size_t d)
      : f0(const_cast<float*>(a), w, h, d), f1(const_cast<float*>(b), w, h, d) {}
};
}  // namespace

int f3d_slabflow_upload(f3d_slabflow flow, const float* frame_0, const float* frame_1)
{
  if (!flow || !frame_0 || !frame_1) return 1;
  const DataSize4 s = flow->driver->FullSize();
  FullVolumes v(frame_0, frame_1, s.width, s.height, s.depth);
  flow->driver->UploadFrames(v.f0, v.f1);
  return flow->driver->failed() ? 1 : 0;
}

int f3d_slabflow_compute_resident(f3d_slabflow flow, const f3d_flow_params* params, float* device_seconds)
{
  if (!flow || !params) return 1;
  f3d_flow_params p = *params;
  OperationParameters bag;
  FillBag(bag, p);
  const bool ok = flow->driver->ComputeResident(bag);
  if (device_seconds) *device_seconds = flow->driver->LastDeviceSeconds();
  return ok ? 0 : 1;
}

int f3d_slabflow_download(f3d_slabflow flow, float* u, float* v, float* w)
{
  if (!flow || !u || !v || !w) return 1;
  const DataSize4 s = flow->driver->FullSize();
  Data3D fu(u, s.width, s.height, s.depth), fv(v, s.width, s.height, s.depth), fw(w, s.width, s.height, s.depth);
  flow->driver->DownloadFlow(fu, fv, fw);
  return flow->driver->failed() ? 1 : 0;
}

int f3d_slabflow_compute(f3d_slabflow flow, const float* frame_0, const float* frame_1, const f3d_flow_params* params,
                         float* u, float* v, float* w)
{
  if (f3d_slabflow_upload(flow, frame_0, frame_1) != 0) return 1;
  if (f3d_slabflow_compute_resident(flow, params, nullptr) != 0) return 1;
  return f3d_slabflow_download(flow, u, v, w);
}

int f3d_slabflow_overlapped_iterations(f3d_slabflow flow, size_t* count)
{
  if (!flow || !count) return 1;
  *count = flow->driver->OverlappedIterations();
  return 0;
}

int f3d_slabflow_batched_exchanges(f3d_slabflow flow, size_t* count)
{
  if (!flow || !flow->driver || !count) return 1;
  *count = flow->driver->BatchedExchanges();
  return 0;
}

int f3d_slabflow_stage_exchanges(f3d_slabflow flow, size_t* count)
{
  if (!flow || !flow->driver || !count) return 1;
  *count = flow->driver->StageExchanges();
  return 0;
}

int f3d_slabflow_set_exchange_per_stage(f3d_slabflow flow, int per_stage)
{
  if (!flow || !flow->driver) return 1;
  flow->driver->SetExchangePerStage(per_stage != 0);
  return 0;
}

int f3d_slabflow_gathered_warps(f3d_slabflow flow, size_t* count)
{
  if (!flow || !flow->driver || !count) return 1;
  *count = flow->driver->GatheredWarps();
  return 0;
}

int f3d_slabflow_destroy(f3d_slabflow flow)
{
  delete flow;
  return 0;
}

int f3d_plan_owned(int depth, int rank, int n_ranks, int* lo, int* hi)
{
  if (!lo || !hi || n_ranks < 1 || rank < 0 || rank >= n_ranks || depth < 0) return 1;
  const PlaneRange r = OwnedPlanes(depth, rank, n_ranks);
  *lo = r.lo;
  *hi = r.hi;
  return 0;
}

int f3d_plan_exchange(int depth, int rank, int n_ranks, int need_lo, int need_hi, int* peer, int* send_lo, int* send_hi,
                      int* recv_lo, int* recv_hi, int capacity)
{
  if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return -1;
  const std::vector<HaloTransfer> plan = PlanHaloExchange(depth, rank, n_ranks, need_lo, need_hi);
  if (static_cast<int>(plan.size()) > capacity) return -1;
  for (size_t i = 0; i < plan.size(); ++i) {
    peer[i] = plan[i].peer;
    send_lo[i] = plan[i].send.lo;
    send_hi[i] = plan[i].send.hi;
    recv_lo[i] = plan[i].recv.lo;
    recv_hi[i] = plan[i].recv.hi;
  }
  return static_cast<int>(plan.size());
}

int f3d_plan_resample_source(int in_depth, int out_depth, int out_lo, int out_hi, int* lo, int* hi)
{
  if (!lo || !hi || in_depth < 1 || out_depth < 1) return 1;
  PlaneRange out;
  out.lo = out_lo;
  out.hi = out_hi;
  const PlaneRange r = ResampleSourcePlanes(in_depth, out_depth, out);
  *lo = r.lo;
  *hi = r.hi;
  return 0;
}

int f3d_host_shutdown(void)
{
  if (!f3d_is_initialized()) return 0;
  PiecemealReleaseArena();
  f3d_comm_destroy();
  return f3d_shutdown();
}

}  // extern "C"
