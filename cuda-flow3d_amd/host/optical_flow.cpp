// Coarse-to-fine driver.  Sequence of operations, buffer counts, parameter keys and console lines follow
// OpticalFlowE::ComputeFlow (src/optical_flow/optical_flow_e.cpp:132-601) and OpticalFlowBase
// (src/optical_flow/optical_flow_base.cpp); the code is organised around a container pool and one
// RunPyramid() shared by the host-volume entry point and the device-resident one.
#include "optical_flow.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "block_match.h"
#include "common_utils.h"
#include "operator_calls.h"
#include "hip_utils.h"
#include "label_field.h"
#include "label_shape.h"
#include "motion_fit.h"
#include "subset_match.h"

// Declared weak: the host library keeps loading against a device library that lacks the entry (the address is then null and the
// trajectory calls fail with a message instead of the whole library failing to load).
extern "C" int f3d_compose_flow(f3d_devptr acc_u, f3d_devptr acc_v, f3d_devptr acc_w, f3d_devptr inc_u, f3d_devptr inc_v,
                                f3d_devptr inc_w, size_t width, size_t height, size_t depth, unsigned long long* lost)
    __attribute__((weak));
extern "C" int f3d_block_match(f3d_devptr a, f3d_devptr b, float lo, float hi, size_t bins, size_t width, size_t height, size_t depth,
                               const f3d_block_match_grid* grid, const int* centre, f3d_block_match_record* records,
                               f3d_block_match_info* info) __attribute__((weak));
extern "C" int f3d_subset_match(f3d_devptr a, f3d_devptr b, size_t width, size_t height, size_t depth, const f3d_subset_match_grid* grid,
                                int model, const double* start, int max_iterations, double tolerance, double reach,
                                f3d_subset_match_record* records, f3d_subset_match_info* info) __attribute__((weak));
extern "C" int f3d_expand_nodes(const float* u, const float* v, const float* w, int ox, int oy, int oz, int step, int nx, int ny, int nz,
                                f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w, size_t width, size_t height, size_t depth)
    __attribute__((weak));
extern "C" int f3d_initial_flow(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w,
                                size_t width, size_t height, size_t depth, f3d_initial_info* info) __attribute__((weak));
extern "C" int f3d_flow_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[8], unsigned fields, size_t width,
                               size_t height, size_t depth, f3d_strain_stats* stats) __attribute__((weak));
extern "C" int f3d_window_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[17], unsigned fields, unsigned radius,
                                 unsigned min_count, size_t width, size_t height, size_t depth, f3d_window_strain_stats* stats)
    __attribute__((weak));
extern "C" int f3d_principal_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[10], unsigned fields,
                                    size_t width, size_t height, size_t depth, f3d_principal_stats* stats) __attribute__((weak));
extern "C" int f3d_polar_decomposition(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[7], unsigned fields,
                                       size_t width, size_t height, size_t depth, f3d_polar_stats* stats) __attribute__((weak));
extern "C" int f3d_principal_from_gradient(const f3d_devptr grad[9], const f3d_devptr out[10], unsigned fields, size_t width,
                                           size_t height, size_t depth, f3d_principal_stats* stats) __attribute__((weak));
extern "C" int f3d_polar_from_gradient(const f3d_devptr grad[9], const f3d_devptr out[7], unsigned fields, size_t width, size_t height,
                                       size_t depth, f3d_polar_stats* stats) __attribute__((weak));
extern "C" int f3d_invert_displacement(f3d_devptr d_u, f3d_devptr d_v, f3d_devptr d_w, f3d_devptr g_u, f3d_devptr g_v,
                                       f3d_devptr g_w, f3d_devptr err, size_t width, size_t height, size_t depth,
                                       unsigned iterations, float tolerance, f3d_inverse_stats* stats) __attribute__((weak));
extern "C" int f3d_carry_field(f3d_devptr field, f3d_devptr m_u, f3d_devptr m_v, f3d_devptr m_w, f3d_devptr out, size_t width,
                               size_t height, size_t depth, unsigned mode, unsigned long long* lost) __attribute__((weak));
extern "C" int f3d_local_correlation(f3d_devptr a, f3d_devptr b, const f3d_devptr out[2], unsigned fields, unsigned radius,
                                     float threshold, size_t width, size_t height, size_t depth, f3d_correlation_stats* stats)
    __attribute__((weak));
extern "C" int f3d_motion_sums(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr weight, float weight_min, size_t width,
                               size_t height, size_t depth, struct f3d_motion_sums* out) __attribute__((weak));
extern "C" int f3d_remove_motion(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w,
                                 const f3d_motion_fit* fit, size_t width, size_t height, size_t depth, f3d_motion_residual* stats)
    __attribute__((weak));
extern "C" int f3d_label_motion_sums(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr labels, size_t n_labels, f3d_devptr weight,
                                     float weight_min, size_t width, size_t height, size_t depth, struct f3d_motion_sums* out,
                                     f3d_label_info* info) __attribute__((weak));
extern "C" int f3d_remove_label_motion(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr labels, size_t n_labels,
                                       const f3d_motion_fit* fits, const int* status, f3d_devptr out_u, f3d_devptr out_v,
                                       f3d_devptr out_w, size_t width, size_t height, size_t depth, f3d_motion_residual* stats)
    __attribute__((weak));
extern "C" int f3d_label_contacts(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr labels, size_t n_labels, size_t width, size_t height,
                                  size_t depth, size_t capacity, struct f3d_contact* out, f3d_contact_info* info) __attribute__((weak));
extern "C" int f3d_label_shape_sums(f3d_devptr labels, size_t n_labels, size_t width, size_t height, size_t depth,
                                    struct f3d_label_shape_sums* out, f3d_label_shape_info* info) __attribute__((weak));
extern "C" int f3d_label_overlap(f3d_devptr labels_a, size_t n_a, f3d_devptr labels_b, size_t n_b, f3d_devptr u, f3d_devptr v, f3d_devptr w,
                                 size_t width, size_t height, size_t depth, size_t capacity, struct f3d_overlap* out, f3d_overlap_info* info)
    __attribute__((weak));
extern "C" int f3d_relabel_labels(f3d_devptr labels, size_t n, const int* map, f3d_devptr out, size_t width, size_t height, size_t depth,
                                  unsigned long long* foreign) __attribute__((weak));
extern "C" int f3d_label_field_sums(f3d_devptr field, f3d_devptr labels, size_t n_labels, int shift, float lo, float hi, size_t bins,
                                    size_t width, size_t height, size_t depth, struct f3d_label_field_sums* out, unsigned* counts,
                                    f3d_label_field_info* info) __attribute__((weak));
extern "C" int f3d_paint_labels(f3d_devptr labels, size_t n_labels, const float* values, f3d_devptr out, size_t width, size_t height,
                                size_t depth) __attribute__((weak));
extern "C" int f3d_label_components(f3d_devptr src, float lo, float hi, unsigned long long min_voxels, f3d_devptr labels_out, size_t width,
                                    size_t height, size_t depth, unsigned long long* sizes, size_t capacity, f3d_component_info* info)
    __attribute__((weak));
extern "C" int f3d_split_components(f3d_devptr src, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels,
                                    f3d_devptr labels_out, size_t width, size_t height, size_t depth, unsigned long long* sizes, size_t capacity,
                                    f3d_split_info* info) __attribute__((weak));
extern "C" int f3d_value_range(f3d_devptr src, f3d_devptr mask, size_t width, size_t height, size_t depth, float* min, float* max,
                               f3d_range_info* info) __attribute__((weak));
extern "C" int f3d_histogram(f3d_devptr src, f3d_devptr mask, float lo, float hi, size_t bins, size_t width, size_t height, size_t depth,
                             unsigned long long* counts, f3d_histogram_info* info) __attribute__((weak));
extern "C" int f3d_validate_displacement(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr weight, float weight_min, unsigned step,
                                         float eps, float threshold, unsigned min_neighbours, unsigned mode, const f3d_devptr out[4],
                                         unsigned fields, size_t width, size_t height, size_t depth, f3d_validate_stats* stats)
    __attribute__((weak));

// ---- base --------------------------------------------------------------------------------------------------

size_t OpticalFlowBase::GetMaxWarpLevel(size_t width, size_t height, size_t depth, float scale_factor)
{
  // count levels while every axis of ceil(dim * sf^level) keeps at least 4 voxels (optical_flow_base.cpp:31-56)
  size_t rw = 1, rh = 1, rd = 1;
  size_t level_counter = 1;
  while (scale_factor < 1.f) {
    const float scale = std::pow(scale_factor, static_cast<float>(level_counter));
    rw = static_cast<size_t>(std::ceil(width * scale));
    rh = static_cast<size_t>(std::ceil(height * scale));
    rd = static_cast<size_t>(std::ceil(depth * scale));
    if (rw < 4 || rh < 4 || rd < 4) break;
    ++level_counter;
  }
  if (rw == 1 || rh == 1 || rd == 1) --level_counter;
  return level_counter;
}

PyramidLevel OpticalFlowBase::GetLevel(const DataSize4& original, float scale_factor, int level)
{
  // optical_flow_e.cpp:262-268: float product, std::ceil, spacing = original / current
  PyramidLevel out;
  const float scale = std::pow(scale_factor, static_cast<float>(level));
  out.size.width = static_cast<size_t>(std::ceil(original.width * scale));
  out.size.height = static_cast<size_t>(std::ceil(original.height * scale));
  out.size.depth = static_cast<size_t>(std::ceil(original.depth * scale));
  out.size.pitch = 0;
  out.hx = original.width / static_cast<float>(out.size.width);
  out.hy = original.height / static_cast<float>(out.size.height);
  out.hz = original.depth / static_cast<float>(out.size.depth);
  return out;
}

bool OpticalFlowBase::IsInitialized() const
{
  if (!initialized_) std::printf("Error: '%s' was not initialized.\n", name_);
  return initialized_;
}

void OpticalFlowBase::ComputeFlow(Data3D&, Data3D&, Data3D&, Data3D&, Data3D&, OperationParameters&)
{
  std::printf("Warning: '%s' ComputeFlow() was not defined.\n", name_);
}

void OpticalFlowBase::Destroy() { initialized_ = false; }

OpticalFlowBase::~OpticalFlowBase() {}

// ---- single-GPU driver ---------------------------------------------------------------------------------------

// the F3D_* bit that selects each output of f3d_flow_strain and f3d_principal_strain (the inverse has no selection)
namespace {

const unsigned kStrainGroups[8] = {F3D_STRAIN_VOL, F3D_STRAIN_E, F3D_STRAIN_E, F3D_STRAIN_E,
                                   F3D_STRAIN_E,   F3D_STRAIN_E, F3D_STRAIN_E, F3D_STRAIN_EQ};
const unsigned kWindowStrainGroups[17] = {F3D_STRAIN_VOL, F3D_STRAIN_E,  F3D_STRAIN_E,  F3D_STRAIN_E,  F3D_STRAIN_E,  F3D_STRAIN_E,
                                          F3D_STRAIN_E,   F3D_STRAIN_EQ, F3D_WSTRAIN_G, F3D_WSTRAIN_G, F3D_WSTRAIN_G, F3D_WSTRAIN_G,
                                          F3D_WSTRAIN_G,  F3D_WSTRAIN_G, F3D_WSTRAIN_G, F3D_WSTRAIN_G, F3D_WSTRAIN_G};
const unsigned kWindowStrainAll = F3D_STRAIN_VOL | F3D_STRAIN_E | F3D_STRAIN_EQ | F3D_WSTRAIN_G;
const unsigned kPrincipalGroups[10] = {F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_SHEAR,
                                       F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR1,   F3D_PRINCIPAL_DIR3,
                                       F3D_PRINCIPAL_DIR3,   F3D_PRINCIPAL_DIR3};
const unsigned kPrincipalAll = F3D_PRINCIPAL_VALUES | F3D_PRINCIPAL_SHEAR | F3D_PRINCIPAL_DIR1 | F3D_PRINCIPAL_DIR3;
const unsigned kPolarGroups[7] = {F3D_POLAR_ANGLE,   F3D_POLAR_VECTOR,  F3D_POLAR_VECTOR, F3D_POLAR_VECTOR,
                                  F3D_POLAR_STRETCH, F3D_POLAR_STRETCH, F3D_POLAR_STRETCH};
const unsigned kPolarAll = F3D_POLAR_ANGLE | F3D_POLAR_VECTOR | F3D_POLAR_STRETCH;
const unsigned kMatchGroups[3] = {OpticalFlowE::kMatchWarped, OpticalFlowE::kMatchZncc, OpticalFlowE::kMatchRmsd};
const unsigned kMatchAll = OpticalFlowE::kMatchWarped | OpticalFlowE::kMatchZncc | OpticalFlowE::kMatchRmsd;
// r, u, v, w, and the second u, v, w the fill passes alternate with (a bit of its own, never downloaded)
const unsigned kValidatedSpare = 4u;
const int kValidatedContainers = 7;
const unsigned kValidatedGroups[kValidatedContainers] = {F3D_VALIDATE_R, F3D_VALIDATE_D, F3D_VALIDATE_D, F3D_VALIDATE_D,
                                                         kValidatedSpare,  kValidatedSpare,  kValidatedSpare};
// the residual u, v, w of the per-label motion, and the container of the labels (a bit of its own, never downloaded)
const unsigned kLabelResidual = 1u, kLabelLabels = 2u;
const unsigned kLabelMotionGroups[4] = {kLabelResidual, kLabelResidual, kLabelResidual, kLabelLabels};
const int kDerivedFields[OpticalFlowE::kDerivedCount] = {8, 10, 4, 3, 3, 4, 7, 4, 17, 10, 7};
const unsigned* const kDerivedGroups[OpticalFlowE::kDerivedCount] = {kStrainGroups, kPrincipalGroups, nullptr,
                                                                     kMatchGroups,  nullptr,          kValidatedGroups,
                                                                     kPolarGroups,  kLabelMotionGroups, kWindowStrainGroups,
                                                                     kPrincipalGroups, kPolarGroups};
const char* const kTrajectoryNotStarted = "the trajectory was not started (ResetTrajectory first)";

}  // namespace

OpticalFlowE::OpticalFlowE()
    : OpticalFlowBase("Optical Flow Single GPU"),
      trajectory_{this, 3, nullptr, "the three trajectory containers do not fit beside the driver's on the device",
                  kTrajectoryNotStarted, "no host volume for a trajectory component",
                  "the device library has no f3d_compose_flow (trajectory composition)", "no flow to compose"},
      initial_{this, 3, nullptr, "the three containers of the initial flow do not fit beside the driver's on the device",
               "no initial flow is held (SetInitialFlow first)", "no host volume for a component of the initial flow",
               "the device library has no f3d_initial_flow (a solve started from a given displacement)",
               "no displacement to start from"},
      derived_{{this, kDerivedFields[kStrain], kStrainGroups, "the strain containers do not fit beside the driver's on the device",
                "a requested strain field has not been computed", "no host volume for a requested strain field",
                "the device library has no f3d_flow_strain (strain fields)", "no displacement to differentiate"},
               {this, kDerivedFields[kPrincipal], kPrincipalGroups, "the principal strain containers do not fit beside the driver's on the device",
                "a requested principal strain field has not been computed", "no host volume for a requested principal strain field",
                "the device library has no f3d_principal_strain (principal strains)", "no displacement to differentiate"},
               {this, kDerivedFields[kInverse], nullptr, "the inverse displacement containers do not fit beside the driver's on the device",
                "the inverse displacement has not been computed", "no host volume for an inverse displacement field",
                "the device library has no f3d_invert_displacement (inverse displacement)", "no displacement to invert"},
               {this, kDerivedFields[kMatch], kMatchGroups, "the match quality containers do not fit beside the driver's on the device",
                "a requested match quality field has not been computed", "no host volume for a requested match quality field",
                "the device library has no f3d_local_correlation (match quality)", "no displacement to carry frame 1 through"},
               {this, kDerivedFields[kMotion], nullptr, "the motion residual containers do not fit beside the driver's on the device",
                "the motion residual has not been computed", "no host volume for a motion residual field",
                "the device library has no f3d_motion_sums (motion fit)", "no displacement to fit a motion to"},
               {this, kValidatedContainers, kValidatedGroups,
                "the validated displacement's containers do not fit beside the driver's on the device",
                "a requested field of the validated displacement has not been computed",
                "no host volume for a requested field of the validated displacement",
                "the device library has no f3d_validate_displacement (displacement validation)", "no displacement to validate"},
               {this, kDerivedFields[kPolar], kPolarGroups, "the rotation and stretch containers do not fit beside the driver's on the device",
                "a requested rotation or stretch field has not been computed", "no host volume for a requested rotation or stretch field",
                "the device library has no f3d_polar_decomposition (local rotation and stretches)", "no displacement to differentiate"},
               {this, kDerivedFields[kLabelMotion], kLabelMotionGroups,
                "the containers of the per-label motion do not fit beside the driver's on the device",
                "the residual of the per-label motion has not been computed", "no host volume for a field of the per-label residual",
                "the device library has no f3d_label_motion_sums (per-label motion)", "no displacement to fit the motion of the labels to"},
               {this, kDerivedFields[kWindowStrain], kWindowStrainGroups,
                "the window strain containers do not fit beside the driver's on the device",
                "a requested window strain field has not been computed", "no host volume for a requested window strain field",
                "the device library has no f3d_window_strain (strain over a window)", "no displacement to differentiate"},
               {this, kDerivedFields[kWindowPrincipal], kPrincipalGroups,
                "the window principal strain containers do not fit beside the driver's on the device",
                "a requested window principal strain field has not been computed",
                "no host volume for a requested window principal strain field",
                "the device library has no f3d_principal_from_gradient (principal strains of a stored gradient)",
                "no displacement to differentiate"},
               {this, kDerivedFields[kWindowPolar], kPolarGroups,
                "the window rotation and stretch containers do not fit beside the driver's on the device",
                "a requested window rotation or stretch field has not been computed",
                "no host volume for a requested window rotation or stretch field",
                "the device library has no f3d_polar_from_gradient (local rotation and stretches of a stored gradient)",
                "no displacement to differentiate"}}
{
  // same initialisation order as the reference's forward_list built with push_front (optical_flow_e.cpp:34-39)
  cuda_operations_ = {&cuop_solve_, &cuop_resample_, &cuop_register_, &cuop_median_, &cuop_convolution_, &cuop_add_};
}

OpticalFlowE::~OpticalFlowE() { Destroy(); }

bool OpticalFlowE::Initialize(const DataSize4& data_size)
{
  dev_container_size_ = data_size;
  dev_container_size_.pitch = 0;
  initialized_ = InitCudaMemory() && InitCudaOperations();
  return initialized_;
}

bool OpticalFlowE::InitCudaMemory()
{
  std::printf("Allocating memory on the device...\n");
  size_t free_memory = 0, total_memory = 0;
  CheckDeviceError(f3d_mem_info(&free_memory, &total_memory));
  const float mb = 1024.f * 1024.f;
  std::printf("Available\t:\t%.0fMB / %.0fMB\n", free_memory / mb, total_memory / mb);

  const size_t rows = dev_container_size_.height * dev_container_size_.depth;
  const size_t row_bytes = dev_container_size_.width * sizeof(float);
  const size_t pitch_guess = (row_bytes + 255) / 256 * 256;
  const size_t needed_memory = pitch_guess * rows * kContainers;
  // the solve operator allocates up to six more container-sized volumes on first use (second weight pair of the fused last
  // sweep, frame derivatives); it runs the unfused schedule when they do not fit, so they are reported, not required
  const size_t optional_memory = pitch_guess * rows * CudaOperationSolve::ScratchVolumes();
  std::printf("Needed (approx.):\t%.0fMB (+ %.0fMB optional solver scratch)\n", needed_memory / mb, optional_memory / mb);
  if (needed_memory >= free_memory) return false;
  // the fit decision counts the 15 containers only; what the optional scratch will meet is said here, so that a run that ends up on
  // the schedules without it (frame builds, separate phi/ksi launches) is not a surprise (advisor, round 3)
  if (optional_memory > 0 && needed_memory + optional_memory >= free_memory)
    std::printf("Solver scratch	:	does not fit beside the containers: the solver will take the launches that need none\n");

  size_t allocated_memory = 0;
  for (size_t i = 0; i < kContainers; ++i) {
    DevicePtr container = 0;
    size_t pitch = 0;
    const bool error = CheckDeviceError(f3d_alloc_pitched(&container, &pitch, row_bytes, rows));
    if (!error) free_containers_.push_back(container);
    // every container must come back with the same pitch
    if (error || (i != 0 && pitch != dev_container_size_.pitch)) {
      std::printf("Error during device memory allocation.");
      Destroy();
      return false;
    }
    dev_container_size_.pitch = pitch;
    allocated_memory += pitch * rows;
  }
  std::printf("Allocated\t:\t%.0fMB\n", allocated_memory / mb);
  return true;
}

bool OpticalFlowE::InitCudaOperations()
{
  if (dev_container_size_.pitch == 0) {
    std::printf("Initialization failed. Device pitch is 0.\n");
    return false;
  }
  std::printf("Initialization of cuda operations...\n");
  OperationParameters op;
  op.PushValuePtr("container_size", &dev_container_size_);
  for (CudaOperationBase* cuop : cuda_operations_) {
    std::printf("%-18s: ", cuop->GetName());
    if (!cuop->Initialize(&op)) {
      Destroy();
      return false;
    }
    std::printf("OK\n");
  }
  return true;
}

DevicePtr OpticalFlowE::Borrow()
{
  // ComputeFlow holds at most 13 of the 15 containers at a time (ten roles + three temps of the batched flow resampling); a caller
  // that keeps more -- results not yet released, a driver extended in place -- gets a fresh container instead of an empty stack
  if (free_containers_.empty()) {
    DevicePtr extra = 0;
    size_t pitch = 0;
    const size_t rows = dev_container_size_.height * dev_container_size_.depth;
    if (CheckDeviceError(f3d_alloc_pitched(&extra, &pitch, dev_container_size_.width * sizeof(float), rows)) ||
        pitch != dev_container_size_.pitch) {
      std::printf("'%s': the container pool is empty and another container could not be allocated.\n", GetName());
      if (extra) f3d_free(extra);
      return 0;
    }
    return extra;   // joins the pool when it is given back
  }
  DevicePtr p = free_containers_.back();
  free_containers_.pop_back();
  return p;
}

void OpticalFlowE::GiveBack(DevicePtr p) { free_containers_.push_back(p); }

void OpticalFlowE::ReleaseResult()
{
  for (DevicePtr& p : result_flow_) {
    if (p) GiveBack(p);
    p = 0;
  }
}

bool OpticalFlowE::AllocateResidentFrames()
{
  if (!IsInitialized()) return false;
  if (resident_frame_[0]) return true;
  const size_t rows = dev_container_size_.height * dev_container_size_.depth;
  for (int i = 0; i < 2; ++i) {
    size_t pitch = 0;
    if (CheckDeviceError(f3d_alloc_pitched(&resident_frame_[i], &pitch, dev_container_size_.width * sizeof(float), rows)) ||
        pitch != dev_container_size_.pitch)
      return false;
  }
  return true;
}

void OpticalFlowE::UploadResidentFrames(Data3D& frame_0, Data3D& frame_1)
{
  if (!AllocateResidentFrames()) return;
  CopyData3DtoDevice(frame_0, resident_frame_[0], dev_container_size_.height, dev_container_size_.pitch);
  CopyData3DtoDevice(frame_1, resident_frame_[1], dev_container_size_.height, dev_container_size_.pitch);
}

void OpticalFlowE::ComputeFlow(Data3D& frame_0, Data3D& frame_1, Data3D& flow_u, Data3D& flow_v, Data3D& flow_w,
                               OperationParameters& params)
{
  ComputeFlow(frame_0, frame_1, flow_u, flow_v, flow_w, params, false);
}

bool OpticalFlowE::CheckInitial(bool use_initial)
{
  initial_.error.clear();
  if (use_initial && !HasInitialFlow()) return initial_.Fail(initial_.not_computed);
  return true;
}

bool OpticalFlowE::ComputeFlow(Data3D& frame_0, Data3D& frame_1, Data3D& flow_u, Data3D& flow_v, Data3D& flow_w,
                               OperationParameters& params, bool use_initial)
{
  if (!IsInitialized()) return false;
  if (!CheckInitial(use_initial)) return false;
  const DevicePtr initial[3] = {initial_.ptr[0], initial_.ptr[1], initial_.ptr[2]};
  if (frame_0.Width() != dev_container_size_.width || frame_0.Height() != dev_container_size_.height ||
      frame_0.Depth() != dev_container_size_.depth || frame_1.Width() != frame_0.Width() ||
      frame_1.Height() != frame_0.Height() || frame_1.Depth() != frame_0.Depth()) {
    std::printf("Error: '%s'. Frame dimensions differ from the initialised container.\n", GetName());
    return false;
  }
  ReleaseResult();

  // the reference's timer spans H2D .. D2H (optical_flow_e.cpp:169,579)
  f3d_event ev_start = nullptr, ev_stop = nullptr;
  CheckDeviceError(f3d_event_create(&ev_start));
  CheckDeviceError(f3d_event_create(&ev_stop));
  CheckDeviceError(f3d_event_record(ev_start));

  DevicePtr raw_0 = Borrow(), raw_1 = Borrow();
  CopyData3DtoDevice(frame_0, raw_0, dev_container_size_.height, dev_container_size_.pitch);
  CopyData3DtoDevice(frame_1, raw_1, dev_container_size_.height, dev_container_size_.pitch);

  const bool ok = RunPyramid(params, raw_0, raw_1, true, use_initial ? &initial : nullptr);
  if (ok) {
    DownloadFlow(flow_u, flow_v, flow_w);
    float elapsed_ms = 0.f;
    CheckDeviceError(f3d_event_record(ev_stop));
    CheckDeviceError(f3d_event_sync(ev_stop));
    CheckDeviceError(f3d_event_elapsed_ms(&elapsed_ms, ev_start, ev_stop));
    std::printf("Total GPU computation time: % 4.4fs\n", elapsed_ms / 1000.);
  } else {
    GiveBack(raw_0);
    GiveBack(raw_1);
  }
  ReleaseResult();
  f3d_event_destroy(ev_start);
  f3d_event_destroy(ev_stop);
  return ok;
}

void OpticalFlowE::ComputeFlowResident(OperationParameters& params) { ComputeFlowResident(params, false); }

bool OpticalFlowE::ComputeFlowResident(OperationParameters& params, bool use_initial)
{
  if (!IsInitialized()) return false;
  if (!CheckInitial(use_initial)) return false;
  const DevicePtr initial[3] = {initial_.ptr[0], initial_.ptr[1], initial_.ptr[2]};
  if (!resident_frame_[0]) {
    std::printf("Error: '%s'. Resident frames were not allocated.\n", GetName());
    return false;
  }
  ReleaseResult();
  f3d_event ev_start = nullptr, ev_stop = nullptr;
  CheckDeviceError(f3d_event_create(&ev_start));
  CheckDeviceError(f3d_event_create(&ev_stop));
  CheckDeviceError(f3d_event_record(ev_start));
  const bool ok = RunPyramid(params, resident_frame_[0], resident_frame_[1], false, use_initial ? &initial : nullptr);
  if (ok) {
    float elapsed_ms = 0.f;
    CheckDeviceError(f3d_event_record(ev_stop));
    CheckDeviceError(f3d_event_sync(ev_stop));
    CheckDeviceError(f3d_event_elapsed_ms(&elapsed_ms, ev_start, ev_stop));
    last_device_seconds_ = elapsed_ms / 1000.f;
  }
  f3d_event_destroy(ev_start);
  f3d_event_destroy(ev_stop);
  return ok;
}

bool OpticalFlowE::AllocateSequenceFrames()
{
  if (!AllocateResidentFrames()) return false;
  if (sequence_frame_[2]) return true;
  sequence_frame_[0] = resident_frame_[0];
  sequence_frame_[1] = resident_frame_[1];
  size_t pitch = 0;
  const size_t rows = dev_container_size_.height * dev_container_size_.depth;
  if (CheckDeviceError(f3d_alloc_pitched(&sequence_frame_[2], &pitch, dev_container_size_.width * sizeof(float), rows)) ||
      pitch != dev_container_size_.pitch) {
    sequence_frame_[2] = 0;
    return false;
  }
  return true;
}

void OpticalFlowE::SelectResidentPair(int slot_0, int slot_1)
{
  if (!sequence_frame_[2]) return;
  resident_frame_[0] = sequence_frame_[slot_0 % 3];
  resident_frame_[1] = sequence_frame_[slot_1 % 3];
}

void OpticalFlowE::BeginComputeFlowResident(OperationParameters& params) { BeginComputeFlowResident(params, false); }

bool OpticalFlowE::BeginComputeFlowResident(OperationParameters& params, bool use_initial)
{
  if (!IsInitialized() || !resident_frame_[0] || ev_begin_) return false;
  if (!CheckInitial(use_initial)) return false;
  const DevicePtr initial[3] = {initial_.ptr[0], initial_.ptr[1], initial_.ptr[2]};
  ReleaseResult();
  CheckDeviceError(f3d_event_create(&ev_begin_));
  CheckDeviceError(f3d_event_create(&ev_end_));
  CheckDeviceError(f3d_event_record(ev_begin_));
  // enqueues; nothing in it waits for the device when silent
  const bool ok = RunPyramid(params, resident_frame_[0], resident_frame_[1], false, use_initial ? &initial : nullptr);
  CheckDeviceError(f3d_event_record(ev_end_));
  return ok;
}

void OpticalFlowE::EndComputeFlowResident()
{
  if (!ev_begin_) return;
  float elapsed_ms = 0.f;
  CheckDeviceError(f3d_event_sync(ev_end_));
  CheckDeviceError(f3d_event_elapsed_ms(&elapsed_ms, ev_begin_, ev_end_));
  last_device_seconds_ = elapsed_ms / 1000.f;
  f3d_event_destroy(ev_begin_);
  f3d_event_destroy(ev_end_);
  ev_begin_ = ev_end_ = nullptr;
}

bool OpticalFlowE::TakeResult(DevicePtr (&flow)[3])
{
  if (!result_flow_[0]) return false;
  // the pool keeps its fifteen: three spare containers replace the ones that leave (allocated once, recycled afterwards)
  const size_t rows = dev_container_size_.height * dev_container_size_.depth;
  while (free_containers_.size() < kContainers) {
    DevicePtr p = 0;
    size_t pitch = 0;
    if (CheckDeviceError(f3d_alloc_pitched(&p, &pitch, dev_container_size_.width * sizeof(float), rows)) || pitch != dev_container_size_.pitch)
      return false;
    free_containers_.push_back(p);
    ++extra_containers_;
  }
  for (int i = 0; i < 3; ++i) {
    flow[i] = result_flow_[i];
    result_flow_[i] = 0;
  }
  return true;
}

void OpticalFlowE::GiveResultBack(DevicePtr (&flow)[3])
{
  for (DevicePtr& p : flow) {
    if (p) free_containers_.push_back(p);
    p = 0;
  }
}

void OpticalFlowE::DownloadFlow(Data3D& flow_u, Data3D& flow_v, Data3D& flow_w)
{
  if (!result_flow_[0]) return;
  CopyData3DFromDevice(result_flow_[0], flow_u, dev_container_size_.height, dev_container_size_.pitch);
  CopyData3DFromDevice(result_flow_[1], flow_v, dev_container_size_.height, dev_container_size_.pitch);
  CopyData3DFromDevice(result_flow_[2], flow_w, dev_container_size_.height, dev_container_size_.pitch);
}

bool OpticalFlowE::ResultStatistics(Stat3& stat)
{
  if (!IsInitialized() || !result_flow_[0]) return false;
  OperationParameters init;
  init.PushValuePtr("container_size", &dev_container_size_);
  if (!cuop_stat_.Initialize(&init)) return false;
  DataSize4 data_size = {dev_container_size_.width, dev_container_size_.height, dev_container_size_.depth, 0};
  OperationParameters bag;
  calls::Statistics(bag, {&result_flow_[0], &result_flow_[1], &result_flow_[2]}, &data_size, &stat);
  cuop_stat_.silent = true;
  cuop_stat_.Execute(bag);
  return true;
}

bool OpticalFlowE::ResidualOf(DevicePtr frame_0, DevicePtr warped, const DataSize4& size, Residual& out)
{
  double ssq = 0.0, sab = 0.0;
  float mx = 0.f;
  if (CheckDeviceError(f3d_residual_stats(frame_0, warped, size.width, size.height, size.depth, nullptr, &ssq, &sab, &mx))) return false;
  const double n = static_cast<double>(size.width) * static_cast<double>(size.height) * static_cast<double>(size.depth);
  out.rms = std::sqrt(ssq / n);
  out.mean_abs = sab / n;
  out.max_abs = mx;
  return true;
}

bool OpticalFlowE::FinalResidual(Residual& registered, Residual& unregistered)
{
  if (!IsInitialized() || !result_flow_[0] || !resident_frame_[0]) return false;
  DataSize4 size = {dev_container_size_.width, dev_container_size_.height, dev_container_size_.depth, 0};
  DevicePtr dev_temp = Borrow();
  float h = 1.f;
  OperationParameters op;
  calls::Registration(op, &resident_frame_[0], &resident_frame_[1], {&result_flow_[0], &result_flow_[1], &result_flow_[2]}, &dev_temp, &size,
                      {&h, &h, &h});
  cuop_register_.Execute(op);
  const bool ok = ResidualOf(resident_frame_[0], dev_temp, size, registered) &&
                  ResidualOf(resident_frame_[0], resident_frame_[1], size, unregistered);
  GiveBack(dev_temp);
  return ok;
}

// ---- containers of the trajectory and of the derived fields ------------------------------------------------------------------

int OpticalFlowE::DerivedFieldCount(Derived which) { return kDerivedFields[which]; }

bool OpticalFlowE::DerivedSelected(Derived which, int field, unsigned fields)
{
  return kDerivedGroups[which] ? (fields & kDerivedGroups[which][field]) != 0 : fields != 0;
}

bool OpticalFlowE::FieldSet::Fail(const char* what)
{
  error = std::string("'") + driver->GetName() + "': " + what;
  std::printf("Error: %s\n", error.c_str());
  return false;
}

bool OpticalFlowE::FieldSet::Allocate(unsigned mask)
{
  const DataSize4& c = driver->dev_container_size_;
  for (int i = 0; i < count; ++i) {
    if (!Selected(i, mask) || ptr[i]) continue;
    size_t pitch = 0;
    if (f3d_alloc_pitched(&ptr[i], &pitch, c.width * sizeof(float), c.height * c.depth) != 0) ptr[i] = 0;
    if (!ptr[i] || pitch != c.pitch) {
      Release();
      return Fail(fit);
    }
  }
  return true;
}

bool OpticalFlowE::FieldSet::Download(Data3D* const* out, unsigned mask)
{
  error.clear();
  const DataSize4& c = driver->dev_container_size_;
  for (int i = 0; i < count; ++i) {
    if (!Selected(i, mask)) continue;
    if (!ptr[i]) return Fail(not_computed);
    if (!out[i]) return Fail(no_volume);
    if (!Check(CheckDeviceError(f3d_copy3d_d2h(out[i]->DataPtr(), out[i]->Width(), out[i]->Height(), out[i]->Depth(), ptr[i], c.pitch,
                                               c.height, 0))))
      return false;
  }
  return true;
}

void OpticalFlowE::FieldSet::Release()
{
  for (DevicePtr& p : ptr) {
    if (p) CheckDeviceError(f3d_free(p));
    p = 0;
  }
}

f3d_size4 OpticalFlowE::Container() const
{
  return {dev_container_size_.width, dev_container_size_.height, dev_container_size_.depth, dev_container_size_.pitch};
}

// ---- trajectory of a frame sequence ------------------------------------------------------------------------------------------

bool OpticalFlowE::AllocateTrajectory()
{
  trajectory_.error.clear();
  if (!f3d_compose_flow) return trajectory_.Fail(trajectory_.no_entry);
  if (!initialized_) return trajectory_.Fail("the driver was not initialized");
  return trajectory_.Allocate(0);
}

bool OpticalFlowE::ResetTrajectory()
{
  if (!AllocateTrajectory()) return false;
  const size_t rows = dev_container_size_.height * dev_container_size_.depth;
  for (int i = 0; i < 3; ++i)
    if (!trajectory_.Check(CheckDeviceError(f3d_memset2d(trajectory_.ptr[i], dev_container_size_.pitch, 0,
                                                         dev_container_size_.width * sizeof(float), rows))))
      return false;
  return true;
}

bool OpticalFlowE::ComposeTrajectory()
{
  if (!result_flow_[0]) {
    trajectory_.error.clear();
    return trajectory_.Fail("no flow is held on the device (ComputeFlowResident first)");
  }
  const DevicePtr flow[3] = {result_flow_[0], result_flow_[1], result_flow_[2]};
  return ComposeTrajectory(flow);
}

bool OpticalFlowE::ComposeTrajectory(const DevicePtr (&flow)[3])
{
  trajectory_.error.clear();
  if (!f3d_compose_flow) return trajectory_.Fail(trajectory_.no_entry);
  if (!trajectory_.ptr[0]) return trajectory_.Fail(kTrajectoryNotStarted);
  if (!flow[0] || !flow[1] || !flow[2]) return trajectory_.Fail(trajectory_.no_displacement);
  const f3d_size4 c = Container();
  return trajectory_.Check(CheckDeviceError(f3d_set_container(&c))) &&
         trajectory_.Check(CheckDeviceError(f3d_compose_flow(trajectory_.ptr[0], trajectory_.ptr[1], trajectory_.ptr[2], flow[0],
                                                             flow[1], flow[2], c.width, c.height, c.depth, nullptr)));
}

bool OpticalFlowE::DownloadTrajectory(Data3D& u, Data3D& v, Data3D& w, unsigned long long* lost)
{
  Data3D* const out[3] = {&u, &v, &w};
  if (!trajectory_.Download(out, 0)) return false;
  if (lost) {
    const float* p = u.DataPtr();
    const size_t n = u.Width() * u.Height() * u.Depth();
    unsigned long long count = 0;
    for (size_t i = 0; i < n; ++i) count += std::isnan(p[i]) ? 1 : 0;
    *lost = count;
  }
  return true;
}

// ---- the flow a solve starts from ----------------------------------------------------------------------------------------------

bool OpticalFlowE::SetInitialFlow(Data3D& u, Data3D& v, Data3D& w, f3d_initial_info* info)
{
  initial_.error.clear();
  if (!f3d_initial_flow) return initial_.Fail(initial_.no_entry);
  if (!initialized_) return initial_.Fail("the driver was not initialized");
  Data3D* const in[3] = {&u, &v, &w};
  for (Data3D* a : in)
    if (a->Width() != dev_container_size_.width || a->Height() != dev_container_size_.height || a->Depth() != dev_container_size_.depth)
      return initial_.Fail("the components of the initial flow must have the dimensions the driver was initialized with");
  initial_set_ = false;
  if (!initial_.Allocate(0)) return false;
  for (int i = 0; i < 3; ++i) CopyData3DtoDevice(*in[i], initial_.ptr[i], dev_container_size_.height, dev_container_size_.pitch);
  const f3d_size4 c = Container();
  initial_set_ = initial_.Check(CheckDeviceError(f3d_set_container(&c))) &&
                 initial_.Check(CheckDeviceError(f3d_initial_flow(initial_.ptr[0], initial_.ptr[1], initial_.ptr[2], initial_.ptr[0],
                                                                  initial_.ptr[1], initial_.ptr[2], c.width, c.height, c.depth, info)));
  return initial_set_;
}

bool OpticalFlowE::SetInitialFlow(const Displacement& of, f3d_initial_info* info)
{
  DevicePtr d[3];
  if (!ResolveDisplacement(initial_, of, f3d_initial_flow != nullptr, d)) return false;
  for (DevicePtr p : d)
    for (int i = 0; i < 3; ++i)
      if (p == initial_.ptr[i]) return initial_.Fail("the initial flow cannot be set from its own containers");
  initial_set_ = false;
  if (!initial_.Allocate(0)) return false;
  const f3d_size4 c = Container();
  initial_set_ = initial_.Check(CheckDeviceError(f3d_set_container(&c))) &&
                 initial_.Check(CheckDeviceError(f3d_initial_flow(d[0], d[1], d[2], initial_.ptr[0], initial_.ptr[1], initial_.ptr[2],
                                                                  c.width, c.height, c.depth, info)));
  return initial_set_;
}

bool OpticalFlowE::DownloadInitialFlow(Data3D& u, Data3D& v, Data3D& w)
{
  initial_.error.clear();
  if (!HasInitialFlow()) return initial_.Fail(initial_.not_computed);
  Data3D* const out[3] = {&u, &v, &w};
  return initial_.Download(out, 0);
}

void OpticalFlowE::ReleaseInitialFlow()
{
  initial_.Release();
  initial_set_ = false;
}

// ---- the guess from the frames themselves: block matching on a grid of nodes -------------------------------------

bool OpticalFlowE::BlockMatch(const BlockMatchParams& params, const int* centre, f3d_block_match_info* info,
                              f3d_block_match_summary* summary)
{
  initial_.error.clear();
  if (!initialized_) return initial_.Fail("the driver was not initialized");
  if (!f3d_block_match) return initial_.Fail("the device library has no f3d_block_match (coarse block matching of two frames)");
  if (!params.range && !f3d_value_range)
    return initial_.Fail("the device library has no f3d_value_range (finite minimum and maximum of a frame)");
  if (!resident_frame_[0] || !resident_frame_[1])
    return initial_.Fail("no frames on the device (AllocateResidentFrames and UploadResidentFrames first)");
  const f3d_size4 c = Container();
  f3d_block_match_grid grid;
  std::string why;
  if (!LayoutBlockMatch(c.width, c.height, c.depth, params.step, params.window, params.radius[0], params.radius[1], params.radius[2],
                        &grid, &why))
    return initial_.Fail(why.c_str());
  if (!initial_.Check(CheckDeviceError(f3d_set_container(&c)))) return false;
  float lo = 0.f, hi = 0.f;
  if (params.range) {
    lo = params.range[0];
    hi = params.range[1];
  } else {
    f3d_range_info found = {};
    if (!initial_.Check(CheckDeviceError(f3d_value_range(resident_frame_[0], 0, c.width, c.height, c.depth, &lo, &hi, &found))))
      return false;
    if (found.finite == 0 || !(lo < hi)) return initial_.Fail("frame 0 has no two finite values: there is no range to lay the codes over");
  }
  const size_t nodes = static_cast<size_t>(grid.nx) * grid.ny * grid.nz;
  std::vector<f3d_block_match_record> records(nodes);
  std::vector<f3d_block_match_node> rows(nodes);
  if (!initial_.Check(CheckDeviceError(f3d_block_match(resident_frame_[0], resident_frame_[1], lo, hi, params.bins, c.width, c.height,
                                                       c.depth, &grid, centre, records.data(), info))))
    return false;
  if (!SolveBlockMatch(records.data(), &grid, centre, params.min_zncc, rows.data(), summary, &why)) return initial_.Fail(why.c_str());
  match_grid_ = grid;
  match_records_.swap(records);
  match_nodes_.swap(rows);
  return true;
}

bool OpticalFlowE::SetInitialFromNodes(f3d_validate_stats* validated, f3d_initial_info* info)
{
  initial_.error.clear();
  if (!f3d_initial_flow) return initial_.Fail(initial_.no_entry);
  if (!f3d_expand_nodes) return initial_.Fail("the device library has no f3d_expand_nodes (node vectors to a dense field)");
  if (!f3d_validate_displacement) return initial_.Fail("the device library has no f3d_validate_displacement (displacement validation)");
  if (match_nodes_.empty()) return initial_.Fail("no node table is held (BlockMatch first)");
  const f3d_block_match_grid& g = match_grid_;
  const size_t nx = g.nx, ny = g.ny, nz = g.nz, nodes = nx * ny * nz;
  std::vector<float> node[3];
  for (int i = 0; i < 3; ++i) node[i].resize(nodes);
  for (size_t at = 0; at < nodes; ++at) {
    node[0][at] = match_nodes_[at].u;
    node[1][at] = match_nodes_[at].v;
    node[2][at] = match_nodes_[at].w;
  }
  // the median test on the node grid: six small containers of the grid's own geometry
  f3d_devptr small[6] = {0, 0, 0, 0, 0, 0};
  f3d_size4 grid_box = {nx, ny, nz, 0};
  bool ok = true;
  for (int i = 0; i < 6 && ok; ++i) {
    size_t pitch = 0;
    ok = initial_.Check(CheckDeviceError(f3d_alloc_pitched(&small[i], &pitch, nx * sizeof(float), ny * nz)));
    if (ok && grid_box.pitch && pitch != grid_box.pitch) ok = initial_.Fail("the node containers came back with different pitches");
    grid_box.pitch = pitch;
  }
  for (int i = 0; i < 3 && ok; ++i)
    ok = initial_.Check(CheckDeviceError(f3d_copy3d_h2d(small[i], grid_box.pitch, ny, 0, node[i].data(), nx, ny, nz)));
  const f3d_devptr out[4] = {0, small[3], small[4], small[5]};
  f3d_validate_stats stats = {};
  ok = ok && initial_.Check(CheckDeviceError(f3d_set_container(&grid_box))) &&
       initial_.Check(CheckDeviceError(f3d_validate_displacement(small[0], small[1], small[2], 0, 0.8f, 1, 0.1f, 2.0f, 9, F3D_VALIDATE_REPLACE,
                                                                 out, F3D_VALIDATE_D, nx, ny, nz, &stats)));
  for (int i = 0; i < 3 && ok; ++i)
    ok = initial_.Check(CheckDeviceError(f3d_copy3d_d2h(node[i].data(), nx, ny, nz, small[3 + i], grid_box.pitch, ny, 0)));
  for (f3d_devptr p : small)
    if (p) f3d_free(p);
  const f3d_size4 c = Container();
  const bool restored = initial_.Check(CheckDeviceError(f3d_set_container(&c)));
  if (!ok || !restored) return false;
  if (validated) *validated = stats;
  initial_set_ = false;
  if (!initial_.Allocate(0)) return false;
  initial_set_ = initial_.Check(CheckDeviceError(f3d_expand_nodes(node[0].data(), node[1].data(), node[2].data(), g.ox, g.oy, g.oz, g.step,
                                                                  g.nx, g.ny, g.nz, initial_.ptr[0], initial_.ptr[1], initial_.ptr[2],
                                                                  c.width, c.height, c.depth))) &&
                 initial_.Check(CheckDeviceError(f3d_initial_flow(initial_.ptr[0], initial_.ptr[1], initial_.ptr[2], initial_.ptr[0],
                                                                  initial_.ptr[1], initial_.ptr[2], c.width, c.height, c.depth, info)));
  return initial_set_;
}

// ---- subset correlation on the resident pair ------------------------------------------------------------------------

bool OpticalFlowE::SubsetMatch(const SubsetMatchParams& params, f3d_subset_match_info* info, f3d_subset_match_summary* summary)
{
  initial_.error.clear();
  if (!initialized_) return initial_.Fail("the driver was not initialized");
  if (!f3d_subset_match) return initial_.Fail("the device library has no f3d_subset_match (subset correlation of two frames)");
  if (!resident_frame_[0] || !resident_frame_[1])
    return initial_.Fail("no frames on the device (AllocateResidentFrames and UploadResidentFrames first)");
  if (params.start != kSubsetZero && params.start != kSubsetNodes && params.start != kSubsetFlow)
    return initial_.Fail("subset correlation: the start is zero, the node table or the flow");
  if (params.start == kSubsetNodes && match_nodes_.empty()) return initial_.Fail("no node table is held (BlockMatch first)");
  if (params.start == kSubsetFlow && !result_flow_[0]) return initial_.Fail("no flow is held on the device (ComputeFlowResident first)");
  const f3d_size4 c = Container();
  f3d_subset_match_grid grid;
  std::string why;
  if (!LayoutSubsetMatch(c.width, c.height, c.depth, params.step, params.window, &grid, &why)) return initial_.Fail(why.c_str());
  const size_t nx = grid.nx, ny = grid.ny, nz = grid.nz, nodes = nx * ny * nz;

  // the held flow at the node voxels: one plane per node plane and component
  std::vector<float> at_nodes[3];
  if (result_flow_[0]) {
    std::vector<float> plane(c.width * c.height);
    for (int i = 0; i < 3; ++i) {
      at_nodes[i].resize(nodes);
      for (size_t k = 0; k < nz; ++k) {
        const size_t z = static_cast<size_t>(grid.oz) + k * grid.step;
        if (!initial_.Check(CheckDeviceError(f3d_copy3d_d2h(plane.data(), c.width, c.height, 1, result_flow_[i], c.pitch, c.height, z))))
          return false;
        for (size_t j = 0; j < ny; ++j)
          for (size_t n = 0; n < nx; ++n)
            at_nodes[i][(k * ny + j) * nx + n] = plane[(grid.oy + j * grid.step) * c.width + grid.ox + n * grid.step];
      }
    }
  }
  std::vector<double> start;
  if (params.start != kSubsetZero) {
    start.assign(nodes * 12, 0.0);
    const f3d_block_match_grid& m = match_grid_;
    auto nearest = [](int x, int origin, int step, int count) {  // the node nearest to x, the lower of two equally near
      const int below = x <= origin ? 0 : (x - origin) / step;
      const int i = below >= count - 1 ? count - 1 : ((x - origin) - below * step) * 2 > step ? below + 1 : below;
      return static_cast<size_t>(i);
    };
    size_t at = 0;
    for (size_t k = 0; k < nz; ++k)
      for (size_t j = 0; j < ny; ++j)
        for (size_t n = 0; n < nx; ++n, ++at) {
          float v[3];
          if (params.start == kSubsetFlow) {
            for (int i = 0; i < 3; ++i) v[i] = at_nodes[i][at];
          } else {
            const size_t from = (nearest(grid.oz + static_cast<int>(k) * grid.step, m.oz, m.step, m.nz) * m.ny +
                                 nearest(grid.oy + static_cast<int>(j) * grid.step, m.oy, m.step, m.ny)) * m.nx +
                                nearest(grid.ox + static_cast<int>(n) * grid.step, m.ox, m.step, m.nx);
            v[0] = match_nodes_[from].u;
            v[1] = match_nodes_[from].v;
            v[2] = match_nodes_[from].w;
          }
          for (int i = 0; i < 3; ++i) start[12 * at + 4 * i] = static_cast<double>(v[i]);
        }
  }
  if (!initial_.Check(CheckDeviceError(f3d_set_container(&c)))) return false;
  std::vector<f3d_subset_match_record> records(nodes);
  std::vector<f3d_subset_match_node> rows(nodes);
  const double reach = params.reach > 0.0 ? params.reach : static_cast<double>(params.window);
  if (!initial_.Check(CheckDeviceError(f3d_subset_match(resident_frame_[0], resident_frame_[1], c.width, c.height, c.depth, &grid, params.model,
                                                        start.empty() ? nullptr : start.data(), params.max_iterations, params.tolerance,
                                                        reach, records.data(), info))))
    return false;
  const float* compare[3] = {at_nodes[0].data(), at_nodes[1].data(), at_nodes[2].data()};
  if (!TableSubsetMatch(records.data(), &grid, params.min_zncc, result_flow_[0] ? compare : nullptr, rows.data(), summary, &why))
    return initial_.Fail(why.c_str());
  subset_grid_ = grid;
  subset_records_.swap(records);
  subset_nodes_.swap(rows);
  return true;
}

// ---- derived fields of a displacement: strain, principal strain, inverse, match quality -------------------------------------------

bool OpticalFlowE::ResolveDisplacement(FieldSet& set, const Displacement& of, bool have_entry, DevicePtr (&disp)[3])
{
  set.error.clear();
  const DevicePtr* from = of.containers;
  if (of.kind == Displacement::kHeldFlow) {
    if (!result_flow_[0]) return set.Fail("no flow is held on the device (ComputeFlowResident first)");
    from = result_flow_;
  } else if (of.kind == Displacement::kTrajectory) {
    if (!trajectory_.ptr[0]) return set.Fail(kTrajectoryNotStarted);
    from = trajectory_.ptr;
  }
  if (!have_entry) return set.Fail(set.no_entry);
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!from[0] || !from[1] || !from[2]) return set.Fail(set.no_displacement);
  for (int i = 0; i < 3; ++i) disp[i] = from[i];
  return true;
}

bool OpticalFlowE::ComputeStrain(const Displacement& of, unsigned fields, f3d_strain_stats* stats)
{
  FieldSet& set = derived_[kStrain];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_flow_strain != nullptr, d)) return false;
  if (fields == 0 || (fields & ~(F3D_STRAIN_VOL | F3D_STRAIN_E | F3D_STRAIN_EQ)))
    return set.Fail("fields must be a non-empty combination of F3D_STRAIN_VOL, F3D_STRAIN_E, F3D_STRAIN_EQ");
  if (!set.Allocate(fields)) return false;
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_flow_strain(d[0], d[1], d[2], set.ptr, fields, c.width, c.height, c.depth, stats)));
}

bool OpticalFlowE::ComputeWindowStrain(const Displacement& of, unsigned fields, unsigned radius, unsigned min_count,
                                       f3d_window_strain_stats* stats)
{
  FieldSet& set = derived_[kWindowStrain];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_window_strain != nullptr, d)) return false;
  if (fields == 0 || (fields & ~kWindowStrainAll))
    return set.Fail("fields must be a non-empty combination of F3D_STRAIN_VOL, F3D_STRAIN_E, F3D_STRAIN_EQ, F3D_WSTRAIN_G");
  if (radius < 1 || radius > 3) return set.Fail("radius must be 1 .. 3");
  if (!set.Allocate(fields)) return false;
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_window_strain(d[0], d[1], d[2], set.ptr, fields, radius, min_count, c.width, c.height, c.depth,
                                                      stats)));
}

bool OpticalFlowE::ComputePrincipal(const Displacement& of, unsigned fields, f3d_principal_stats* stats)
{
  FieldSet& set = derived_[kPrincipal];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_principal_strain != nullptr, d)) return false;
  if (fields == 0 || (fields & ~kPrincipalAll))
    return set.Fail("fields must be a non-empty combination of F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_SHEAR, F3D_PRINCIPAL_DIR1, "
                    "F3D_PRINCIPAL_DIR3");
  if (!set.Allocate(fields)) return false;
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_principal_strain(d[0], d[1], d[2], set.ptr, fields, c.width, c.height, c.depth, stats)));
}

bool OpticalFlowE::ComputePolar(const Displacement& of, unsigned fields, f3d_polar_stats* stats)
{
  FieldSet& set = derived_[kPolar];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_polar_decomposition != nullptr, d)) return false;
  if (fields == 0 || (fields & ~kPolarAll))
    return set.Fail("fields must be a non-empty combination of F3D_POLAR_ANGLE, F3D_POLAR_VECTOR, F3D_POLAR_STRETCH");
  if (!set.Allocate(fields)) return false;
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_polar_decomposition(d[0], d[1], d[2], set.ptr, fields, c.width, c.height, c.depth, stats)));
}

bool OpticalFlowE::ComputeWindowGradient(FieldSet& set, const Displacement& of, bool have_entry, unsigned radius, unsigned min_count)
{
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, have_entry, d)) return false;
  if (!f3d_window_strain) return set.Fail("the device library has no f3d_window_strain (strain over a window)");
  if (radius < 1 || radius > 3) return set.Fail("radius must be 1 .. 3");
  const DataSize4& s = dev_container_size_;
  for (DevicePtr& p : window_gradient_) {
    if (p) continue;
    size_t pitch = 0;
    if (f3d_alloc_pitched(&p, &pitch, s.width * sizeof(float), s.height * s.depth) != 0) p = 0;
    if (!p || pitch != s.pitch) {
      ReleaseWindowGradient();
      return set.Fail("the nine containers of the window gradient do not fit beside the driver's on the device");
    }
  }
  DevicePtr out[17] = {};
  for (int k = 0; k < 9; ++k) out[8 + k] = window_gradient_[k];
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_window_strain(d[0], d[1], d[2], out, F3D_WSTRAIN_G, radius, min_count, c.width, c.height, c.depth,
                                                      nullptr)));
}

void OpticalFlowE::ReleaseWindowGradient()
{
  for (DevicePtr& p : window_gradient_) {
    if (p) CheckDeviceError(f3d_free(p));
    p = 0;
  }
}

void OpticalFlowE::ReleaseDerived(Derived which)
{
  derived_[which].Release();
  if (which != kWindowPrincipal && which != kWindowPolar) return;
  // the gradient goes with the last container of the two kinds that read it
  for (const FieldSet* set : {&derived_[kWindowPrincipal], &derived_[kWindowPolar]})
    for (DevicePtr p : set->ptr)
      if (p) return;
  ReleaseWindowGradient();
}

bool OpticalFlowE::ComputeWindowPrincipal(const Displacement& of, unsigned fields, unsigned radius, unsigned min_count,
                                          f3d_principal_stats* stats)
{
  FieldSet& set = derived_[kWindowPrincipal];
  set.error.clear();
  if (fields == 0 || (fields & ~kPrincipalAll))
    return set.Fail("fields must be a non-empty combination of F3D_PRINCIPAL_VALUES, F3D_PRINCIPAL_SHEAR, F3D_PRINCIPAL_DIR1, "
                    "F3D_PRINCIPAL_DIR3");
  if (!ComputeWindowGradient(set, of, f3d_principal_from_gradient != nullptr, radius, min_count)) return false;
  if (!set.Allocate(fields)) return false;
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_principal_from_gradient(window_gradient_, set.ptr, fields, c.width, c.height, c.depth, stats)));
}

bool OpticalFlowE::ComputeWindowPolar(const Displacement& of, unsigned fields, unsigned radius, unsigned min_count,
                                      f3d_polar_stats* stats)
{
  FieldSet& set = derived_[kWindowPolar];
  set.error.clear();
  if (fields == 0 || (fields & ~kPolarAll))
    return set.Fail("fields must be a non-empty combination of F3D_POLAR_ANGLE, F3D_POLAR_VECTOR, F3D_POLAR_STRETCH");
  if (!ComputeWindowGradient(set, of, f3d_polar_from_gradient != nullptr, radius, min_count)) return false;
  if (!set.Allocate(fields)) return false;
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_polar_from_gradient(window_gradient_, set.ptr, fields, c.width, c.height, c.depth, stats)));
}

bool OpticalFlowE::ComputeInverse(const Displacement& of, unsigned iterations, float tolerance, f3d_inverse_stats* stats)
{
  FieldSet& set = derived_[kInverse];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_invert_displacement != nullptr, d)) return false;
  if (!set.Allocate(0)) return false;
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_invert_displacement(d[0], d[1], d[2], set.ptr[0], set.ptr[1], set.ptr[2], set.ptr[3], c.width,
                                                            c.height, c.depth, iterations, tolerance, stats)));
}

bool OpticalFlowE::ComputeMatch(const Displacement& of, DevicePtr frame_0, DevicePtr frame_1, unsigned fields, unsigned radius,
                                float threshold, f3d_correlation_stats* stats)
{
  FieldSet& set = derived_[kMatch];
  if (of.kind == Displacement::kTrajectory) {
    set.error.clear();
    return set.Fail("the match quality of a trajectory is not available: frame 0 of a sequence is not kept (use a pair's flow)");
  }
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_local_correlation != nullptr, d)) return false;
  if (!f3d_carry_field) return set.Fail("the device library has no f3d_carry_field (match quality carries frame 1 through the flow)");
  if (fields == 0 || (fields & ~kMatchAll)) return set.Fail("fields must be a non-empty combination of kMatchWarped, kMatchZncc, kMatchRmsd");
  if (!frame_0) frame_0 = resident_frame_[0];
  if (!frame_1) frame_1 = resident_frame_[1];
  if (!frame_0 || !frame_1) return set.Fail("no frames on the device (AllocateResidentFrames and UploadResidentFrames first)");
  // the kernel stores at least one field: zncc when only the warped frame was asked for
  const unsigned stored = fields & (kMatchZncc | kMatchRmsd) ? fields & (kMatchZncc | kMatchRmsd) : kMatchZncc;
  if (!set.Allocate(kMatchWarped | stored)) return false;
  const f3d_size4 c = Container();
  const DevicePtr out[2] = {set.ptr[1], set.ptr[2]};
  const unsigned device_fields = (stored & kMatchZncc ? F3D_CORRELATION_ZNCC : 0u) | (stored & kMatchRmsd ? F3D_CORRELATION_RMSD : 0u);
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_carry_field(frame_1, d[0], d[1], d[2], set.ptr[0], c.width, c.height, c.depth, F3D_CARRY_LINEAR,
                                                    nullptr))) &&
         set.Check(CheckDeviceError(f3d_local_correlation(frame_0, set.ptr[0], out, device_fields, radius, threshold, c.width, c.height,
                                                          c.depth, stats)));
}

bool OpticalFlowE::ComputeMotion(const Displacement& of, int model, DevicePtr weight, float weight_min, f3d_motion_fit* fit,
                                 f3d_motion_residual* residual)
{
  FieldSet& set = derived_[kMotion];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_motion_sums != nullptr, d)) return false;
  if (!f3d_remove_motion) return set.Fail("the device library has no f3d_remove_motion (motion fit)");
  if (!fit) return set.Fail("no fit to write to");
  if (!set.Allocate(0)) return false;
  const f3d_size4 c = Container();
  struct f3d_motion_sums sums;
  if (!set.Check(CheckDeviceError(f3d_set_container(&c))) ||
      !set.Check(CheckDeviceError(f3d_motion_sums(d[0], d[1], d[2], weight, weight_min, c.width, c.height, c.depth, &sums))))
    return false;
  f3d_motion_fit solved = {};
  solved.centre[0] = 0.5 * static_cast<double>(c.width - 1);
  solved.centre[1] = 0.5 * static_cast<double>(c.height - 1);
  solved.centre[2] = 0.5 * static_cast<double>(c.depth - 1);
  std::string why;
  if (!SolveMotion(sums, model, &solved, &why)) return set.Fail(why.c_str());
  if (!set.Check(CheckDeviceError(f3d_remove_motion(d[0], d[1], d[2], set.ptr[0], set.ptr[1], set.ptr[2], &solved, c.width, c.height,
                                                    c.depth, residual))))
    return false;
  *fit = solved;
  return true;
}

bool OpticalFlowE::UploadLabels(const int* labels)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!labels) return set.Fail("no labels to upload");
  if (!set.Allocate(kLabelLabels)) return false;
  const DataSize4& c = dev_container_size_;
  // the copy moves bytes: the int32 labels arrive as they are
  return set.Check(CheckDeviceError(f3d_copy3d_h2d(set.ptr[3], c.pitch, c.height, 0, reinterpret_cast<const float*>(labels), c.width,
                                                   c.height, c.depth)));
}

bool OpticalFlowE::DownloadLabels(int* labels)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!labels) return set.Fail("no labels to download to");
  if (!set.ptr[3]) return set.Fail("no labels on the device (UploadLabels or ComputeLabels first)");
  const DataSize4& c = dev_container_size_;
  // the copy moves bytes: the int32 labels arrive as they are
  return set.Check(CheckDeviceError(f3d_copy3d_d2h(reinterpret_cast<float*>(labels), c.width, c.height, c.depth, set.ptr[3], c.pitch,
                                                   c.height, 0)));
}

bool OpticalFlowE::ComputeLabels(DevicePtr frame, float lo, float hi, unsigned long long min_voxels, std::vector<unsigned long long>* sizes,
                                 f3d_component_info* info)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!f3d_label_components) return set.Fail("the device library has no f3d_label_components (connected bodies of a thresholded volume)");
  if (!info) return set.Fail("no info to write to");
  if (!frame) frame = resident_frame_[0];
  if (!frame) return set.Fail("no frame on the device (AllocateResidentFrames and UploadResidentFrames first)");
  if (!set.Allocate(kLabelLabels)) return false;
  const f3d_size4 c = Container();
  if (!set.Check(CheckDeviceError(f3d_set_container(&c)))) return false;
  if (!sizes) return set.Check(CheckDeviceError(f3d_label_components(frame, lo, hi, min_voxels, set.ptr[3], c.width, c.height, c.depth, nullptr, 0, info)));
  // the number of bodies is known only afterwards: a first call without sizes, and when there are bodies a second one with room for all
  // (the labels are the same bytes both times)
  sizes->clear();
  if (!set.Check(CheckDeviceError(f3d_label_components(frame, lo, hi, min_voxels, set.ptr[3], c.width, c.height, c.depth, nullptr, 0, info))))
    return false;
  if (info->n_labels == 0) return true;
  sizes->resize(static_cast<size_t>(info->n_labels));
  return set.Check(CheckDeviceError(f3d_label_components(frame, lo, hi, min_voxels, set.ptr[3], c.width, c.height, c.depth, sizes->data(),
                                                         sizes->size(), info)));
}

bool OpticalFlowE::ComputeSplitLabels(DevicePtr frame, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels,
                                      std::vector<unsigned long long>* sizes, f3d_split_info* info)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!f3d_split_components) return set.Fail("the device library has no f3d_split_components (bodies of a thresholded volume, touching bodies apart)");
  if (!info) return set.Fail("no info to write to");
  if (!frame) frame = resident_frame_[0];
  if (!frame) return set.Fail("no frame on the device (AllocateResidentFrames and UploadResidentFrames first)");
  if (!set.Allocate(kLabelLabels)) return false;
  const f3d_size4 c = Container();
  if (!set.Check(CheckDeviceError(f3d_set_container(&c)))) return false;
  // as in ComputeLabels: the number of bodies is known only afterwards, and the labels are the same bytes both times
  if (sizes) sizes->clear();
  if (!set.Check(CheckDeviceError(f3d_split_components(frame, lo, hi, core_d2, min_voxels, set.ptr[3], c.width, c.height, c.depth, nullptr, 0, info))))
    return false;
  if (!sizes || info->n_labels == 0) return true;
  sizes->resize(static_cast<size_t>(info->n_labels));
  return set.Check(CheckDeviceError(f3d_split_components(frame, lo, hi, core_d2, min_voxels, set.ptr[3], c.width, c.height, c.depth,
                                                         sizes->data(), sizes->size(), info)));
}

bool OpticalFlowE::ComputeHistogram(DevicePtr frame, const float* range, size_t bins, unsigned long long* counts, f3d_histogram_info* info,
                                    float* lo_used, float* hi_used)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!f3d_histogram) return set.Fail("the device library has no f3d_histogram (grey-value histogram of a frame)");
  if (!range && !f3d_value_range) return set.Fail("the device library has no f3d_value_range (finite minimum and maximum of a frame)");
  if (!counts || !info) return set.Fail("no counts or info to write to");
  if (!frame) frame = resident_frame_[0];
  if (!frame) return set.Fail("no frame on the device (AllocateResidentFrames and UploadResidentFrames first)");
  const f3d_size4 c = Container();
  if (!set.Check(CheckDeviceError(f3d_set_container(&c)))) return false;
  float lo = 0.f, hi = 0.f;
  if (range) {
    lo = range[0];
    hi = range[1];
  } else {
    f3d_range_info found = {};
    if (!set.Check(CheckDeviceError(f3d_value_range(frame, 0, c.width, c.height, c.depth, &lo, &hi, &found)))) return false;
    if (found.finite == 0) return set.Fail("the frame has no finite voxel: there is no range to lay the bins over");
    if (!(lo < hi)) {
      char text[160];
      std::snprintf(text, sizeof(text), "the frame is constant (every finite voxel is %.9g): there is no range to lay the bins over",
                    static_cast<double>(lo));
      return set.Fail(text);
    }
  }
  if (!set.Check(CheckDeviceError(f3d_histogram(frame, 0, lo, hi, bins, c.width, c.height, c.depth, counts, info)))) return false;
  if (lo_used) *lo_used = lo;
  if (hi_used) *hi_used = hi;
  return true;
}

bool OpticalFlowE::ComputeLabelMotion(const Displacement& of, size_t n_labels, int model, unsigned long long min_voxels,
                                      f3d_motion_fit* fits, int* status, double* rms_after, f3d_label_info* info)
{
  FieldSet& set = derived_[kLabelMotion];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_label_motion_sums != nullptr, d)) return false;
  if (!f3d_remove_label_motion) return set.Fail("the device library has no f3d_remove_label_motion (per-label motion)");
  if (!fits || !status) return set.Fail("no fits or status to write to");
  if (n_labels == 0 || n_labels > (static_cast<size_t>(1) << 22)) return set.Fail("n_labels must be 1 .. 2^22");
  const DevicePtr labels = set.ptr[3];
  if (!labels) return set.Fail("no labels on the device (UploadLabels first)");
  if (!set.Allocate(kLabelResidual)) return false;
  const f3d_size4 c = Container();
  std::vector<struct f3d_motion_sums> sums(n_labels);
  if (!set.Check(CheckDeviceError(f3d_set_container(&c))) ||
      !set.Check(CheckDeviceError(f3d_label_motion_sums(d[0], d[1], d[2], labels, n_labels, 0, 0.f, c.width, c.height, c.depth,
                                                        sums.data(), info))))
    return false;
  const double centre[3] = {0.5 * static_cast<double>(c.width - 1), 0.5 * static_cast<double>(c.height - 1),
                            0.5 * static_cast<double>(c.depth - 1)};
  std::string why;
  if (!SolveLabelMotions(sums.data(), n_labels, model, min_voxels, centre, fits, status, &why)) return set.Fail(why.c_str());
  if (!set.Check(CheckDeviceError(f3d_remove_label_motion(d[0], d[1], d[2], labels, n_labels, fits, status, set.ptr[0], set.ptr[1],
                                                          set.ptr[2], c.width, c.height, c.depth, nullptr))))
    return false;
  if (!rms_after) return true;
  if (!set.Check(CheckDeviceError(f3d_label_motion_sums(set.ptr[0], set.ptr[1], set.ptr[2], labels, n_labels, 0, 0.f, c.width, c.height,
                                                        c.depth, sums.data(), nullptr))))
    return false;
  for (size_t l = 0; l < n_labels; ++l) {
    const struct f3d_motion_sums& s = sums[l];
    rms_after[l] = s.n ? std::sqrt(((s.Sdd[0] + s.Sdd[1]) + s.Sdd[2]) / static_cast<double>(s.n)) : std::nan("");
  }
  return true;
}

bool OpticalFlowE::ComputeContacts(const Displacement& of, size_t n_labels, std::vector<f3d_contact>* contacts, f3d_contact_info* info)
{
  FieldSet& set = derived_[kLabelMotion];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, true, d)) return false;
  if (!f3d_label_contacts) return set.Fail("the device library has no f3d_label_contacts (contacts between labels)");
  if (!contacts || !info) return set.Fail("no contacts or info to write to");
  if (n_labels == 0 || n_labels > (static_cast<size_t>(1) << 22)) return set.Fail("n_labels must be 1 .. 2^22");
  const DevicePtr labels = set.ptr[3];
  if (!labels) return set.Fail("no labels on the device (UploadLabels first)");
  const f3d_size4 c = Container();
  if (!set.Check(CheckDeviceError(f3d_set_container(&c)))) return false;
  // The entry wants room for `capacity` rows and writes n_contacts of them: the room is left uninitialised (no page of it is touched
  // beyond what comes down), and the first capacity is capped so that many labels do not ask for 1.8 GB at once.
  const size_t most = static_cast<size_t>(1) << 24, first = static_cast<size_t>(1) << 20;
  contacts->clear();
  for (size_t capacity = std::min(8 * n_labels, first);; capacity = std::min(2 * capacity, most)) {
    std::unique_ptr<f3d_contact[]> room(new f3d_contact[capacity]);
    if (!set.Check(CheckDeviceError(f3d_label_contacts(d[0], d[1], d[2], labels, n_labels, c.width, c.height, c.depth, capacity,
                                                       room.get(), info))))
      return false;
    if (info->complete) {
      contacts->assign(room.get(), room.get() + static_cast<size_t>(info->n_contacts));
      return true;
    }
    if (capacity == most) break;
  }
  contacts->clear();
  return set.Fail("the labels have more than 2^24 distinct contacts");
}

// The second label volume lives in the slot behind the set's four fields: no mask selects it, so Allocate, Download and the loops over
// the fields never see it, and Release (which walks every slot) frees it with the rest.
bool OpticalFlowE::AllocateLabelsB()
{
  FieldSet& set = derived_[kLabelMotion];
  DevicePtr& b = set.ptr[kLabelsBSlot];
  if (b) return true;
  const DataSize4& c = dev_container_size_;
  size_t pitch = 0;
  if (f3d_alloc_pitched(&b, &pitch, c.width * sizeof(float), c.height * c.depth) != 0) b = 0;
  if (b && pitch != c.pitch) {
    CheckDeviceError(f3d_free(b));
    b = 0;
  }
  return b ? true : set.Fail("the container of the second label volume does not fit beside the driver's on the device");
}

bool OpticalFlowE::UploadLabelsB(const int* labels)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!labels) return set.Fail("no labels to upload");
  if (!AllocateLabelsB()) return false;
  const DataSize4& c = dev_container_size_;
  // the copy moves bytes: the int32 labels arrive as they are
  return set.Check(CheckDeviceError(f3d_copy3d_h2d(set.ptr[kLabelsBSlot], c.pitch, c.height, 0, reinterpret_cast<const float*>(labels),
                                                   c.width, c.height, c.depth)));
}

bool OpticalFlowE::DownloadLabelsB(int* labels)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!labels) return set.Fail("no labels to download to");
  if (!set.ptr[kLabelsBSlot]) return set.Fail("no second label volume on the device (UploadLabelsB or ComputeLabelsB first)");
  const DataSize4& c = dev_container_size_;
  return set.Check(CheckDeviceError(f3d_copy3d_d2h(reinterpret_cast<float*>(labels), c.width, c.height, c.depth, set.ptr[kLabelsBSlot],
                                                   c.pitch, c.height, 0)));
}

bool OpticalFlowE::ComputeLabelsB(DevicePtr frame, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels,
                                  std::vector<unsigned long long>* sizes, f3d_split_info* info)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (core_d2 == 0 && !f3d_label_components)
    return set.Fail("the device library has no f3d_label_components (connected bodies of a thresholded volume)");
  if (core_d2 != 0 && !f3d_split_components)
    return set.Fail("the device library has no f3d_split_components (bodies of a thresholded volume, touching bodies apart)");
  if (!info) return set.Fail("no info to write to");
  if (!frame) frame = resident_frame_[1];
  if (!frame) return set.Fail("no later frame on the device (AllocateResidentFrames and UploadResidentFrames first)");
  if (!AllocateLabelsB()) return false;
  const DevicePtr b = set.ptr[kLabelsBSlot];
  const f3d_size4 c = Container();
  if (!set.Check(CheckDeviceError(f3d_set_container(&c)))) return false;
  *info = f3d_split_info{};
  // one call of either entry: its first eight counters are f3d_component_info's, field for field
  auto run = [&](unsigned long long* room, size_t capacity) {
    if (core_d2 != 0)
      return set.Check(CheckDeviceError(f3d_split_components(frame, lo, hi, core_d2, min_voxels, b, c.width, c.height, c.depth, room, capacity, info)));
    f3d_component_info plain = {};
    if (!set.Check(CheckDeviceError(f3d_label_components(frame, lo, hi, min_voxels, b, c.width, c.height, c.depth, room, capacity, &plain))))
      return false;
    info->foreground = plain.foreground;
    info->background = plain.background;
    info->nan = plain.nan;
    info->n_components = plain.n_components;
    info->n_labels = plain.n_labels;
    info->dropped_components = plain.dropped_components;
    info->dropped_voxels = plain.dropped_voxels;
    info->largest = plain.largest;
    return true;
  };
  // as in ComputeLabels: the number of bodies is known only afterwards, and the labels are the same bytes both times
  if (sizes) sizes->clear();
  if (!run(nullptr, 0)) return false;
  if (!sizes || info->n_labels == 0) return true;
  sizes->resize(static_cast<size_t>(info->n_labels));
  return run(sizes->data(), sizes->size());
}

bool OpticalFlowE::ComputeOverlap(const Displacement& of, size_t n_a, size_t n_b, std::vector<f3d_overlap>* rows, f3d_overlap_info* info)
{
  FieldSet& set = derived_[kLabelMotion];
  DevicePtr d[3];
  set.error.clear();
  if (!f3d_label_overlap) return set.Fail("the device library has no f3d_label_overlap (overlap of two label volumes)");
  if (!ResolveDisplacement(set, of, true, d)) return false;
  if (!rows || !info) return set.Fail("no rows or info to write to");
  const size_t most_labels = static_cast<size_t>(1) << 22;
  if (n_a == 0 || n_a > most_labels || n_b == 0 || n_b > most_labels) return set.Fail("n_a and n_b must be 1 .. 2^22");
  const DevicePtr labels_a = set.ptr[3], labels_b = set.ptr[kLabelsBSlot];
  if (!labels_a) return set.Fail("no labels on the device (UploadLabels or ComputeLabels first)");
  if (!labels_b) return set.Fail("no second label volume on the device (UploadLabelsB or ComputeLabelsB first)");
  const f3d_size4 c = Container();
  if (!set.Check(CheckDeviceError(f3d_set_container(&c)))) return false;
  // as in ComputeContacts: the room is left uninitialised, and the first capacity is capped
  const size_t most = static_cast<size_t>(1) << 24, first = static_cast<size_t>(1) << 20;
  rows->clear();
  for (size_t capacity = std::min(8 * (n_a + n_b), first);; capacity = std::min(2 * capacity, most)) {
    std::unique_ptr<f3d_overlap[]> room(new f3d_overlap[capacity]);
    if (!set.Check(CheckDeviceError(f3d_label_overlap(labels_a, n_a, labels_b, n_b, d[0], d[1], d[2], c.width, c.height, c.depth, capacity,
                                                      room.get(), info))))
      return false;
    if (info->complete) {
      rows->assign(room.get(), room.get() + static_cast<size_t>(info->n_pairs));
      return true;
    }
    if (capacity == most) break;
  }
  rows->clear();
  return set.Fail("the two label volumes have more than 2^24 distinct pairs");
}

bool OpticalFlowE::RelabelB(const int* map, size_t n_b)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!f3d_relabel_labels) return set.Fail("the device library has no f3d_relabel_labels (new numbers for labelled bodies)");
  if (!map) return set.Fail("no map to relabel with");
  const DevicePtr b = set.ptr[kLabelsBSlot];
  if (!b) return set.Fail("no second label volume on the device (UploadLabelsB or ComputeLabelsB first)");
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_relabel_labels(b, n_b, map, b, c.width, c.height, c.depth, nullptr)));
}

bool OpticalFlowE::ComputeLabelShapes(size_t n_labels, f3d_label_shape* shapes, f3d_label_shape_info* info)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!f3d_label_shape_sums) return set.Fail("the device library has no f3d_label_shape_sums (shapes of labelled bodies)");
  if (!shapes) return set.Fail("no shapes to write to");
  if (n_labels == 0 || n_labels > (static_cast<size_t>(1) << 22)) return set.Fail("n_labels must be 1 .. 2^22");
  const DevicePtr labels = set.ptr[3];
  if (!labels) return set.Fail("no labels on the device (UploadLabels or ComputeLabels first)");
  const f3d_size4 c = Container();
  std::vector<struct f3d_label_shape_sums> sums(n_labels);
  if (!set.Check(CheckDeviceError(f3d_set_container(&c))) ||
      !set.Check(CheckDeviceError(f3d_label_shape_sums(labels, n_labels, c.width, c.height, c.depth, sums.data(), info))))
    return false;
  SolveLabelShapes(sums.data(), n_labels, shapes);
  return true;
}

bool OpticalFlowE::ComputeLabelField(DevicePtr field, size_t n_labels, int shift, const float* range, size_t bins,
                                     unsigned long long min_voxels, f3d_label_field_stat* stats, unsigned* counts,
                                     f3d_label_field_info* info, f3d_label_field_summary* summary)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!f3d_label_field_sums) return set.Fail("the device library has no f3d_label_field_sums (statistics of a field per labelled body)");
  if (!stats) return set.Fail("no stats to write to");
  if (n_labels == 0 || n_labels > (static_cast<size_t>(1) << 22)) return set.Fail("n_labels must be 1 .. 2^22");
  if ((bins != 0) != (range != nullptr)) return set.Fail("a range goes with bins, and bins with a range");
  if ((bins != 0) != (counts != nullptr)) return set.Fail("counts go with bins, and bins with counts");
  const DevicePtr labels = set.ptr[3];
  if (!labels) return set.Fail("no labels on the device (UploadLabels or ComputeLabels first)");
  if (!field) field = resident_frame_[0];
  if (!field) return set.Fail("no frame on the device (AllocateResidentFrames and UploadResidentFrames first)");
  const f3d_size4 c = Container();
  const float lo = range ? range[0] : 0.f, hi = range ? range[1] : 0.f;
  std::vector<struct f3d_label_field_sums> sums(n_labels);
  if (!set.Check(CheckDeviceError(f3d_set_container(&c))) ||
      !set.Check(CheckDeviceError(f3d_label_field_sums(field, labels, n_labels, shift, lo, hi, bins, c.width, c.height, c.depth, sums.data(),
                                                       counts, info))))
    return false;
  std::string why;
  if (!SolveLabelField(sums.data(), counts, n_labels, shift, lo, hi, bins, min_voxels, stats, summary, &why)) return set.Fail(why.c_str());
  return true;
}

bool OpticalFlowE::LabelFieldRange(DevicePtr field, float* lo, float* hi, f3d_range_info* info)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!f3d_value_range) return set.Fail("the device library has no f3d_value_range (finite minimum and maximum of a frame)");
  if (!lo || !hi || !info) return set.Fail("no range or info to write to");
  const DevicePtr labels = set.ptr[3];
  if (!labels) return set.Fail("no labels on the device (UploadLabels or ComputeLabels first)");
  if (!field) field = resident_frame_[0];
  if (!field) return set.Fail("no frame on the device (AllocateResidentFrames and UploadResidentFrames first)");
  const f3d_size4 c = Container();
  return set.Check(CheckDeviceError(f3d_set_container(&c))) &&
         set.Check(CheckDeviceError(f3d_value_range(field, labels, c.width, c.height, c.depth, lo, hi, info)));
}

bool OpticalFlowE::PaintLabels(const float* values, size_t n_labels, float* out)
{
  FieldSet& set = derived_[kLabelMotion];
  set.error.clear();
  if (!initialized_) return set.Fail("the driver was not initialized");
  if (!f3d_paint_labels) return set.Fail("the device library has no f3d_paint_labels (a value per label painted into a volume)");
  if (!values || !out) return set.Fail("no values to paint or no volume to paint into");
  const DevicePtr labels = set.ptr[3];
  if (!labels) return set.Fail("no labels on the device (UploadLabels or ComputeLabels first)");
  const f3d_size4 c = Container();
  const DevicePtr painted = Borrow();
  if (!painted) return set.Fail("no container to paint into");
  const bool ok = set.Check(CheckDeviceError(f3d_set_container(&c))) &&
                  set.Check(CheckDeviceError(f3d_paint_labels(labels, n_labels, values, painted, c.width, c.height, c.depth))) &&
                  set.Check(CheckDeviceError(f3d_copy3d_d2h(out, c.width, c.height, c.depth, painted, c.pitch, c.height, 0)));
  GiveBack(painted);
  return ok;
}

DevicePtr OpticalFlowE::NamedField(const char* name) const
{
  static const struct {
    const char* name;
    Derived which;
    int field;
  } kNamed[] = {{"vol", kStrain, 0},  {"eq", kStrain, 7}, {"gmax", kPrincipal, 3},     {"angle", kPolar, 0},
                {"zncc", kMatch, 1}, {"rmsd", kMatch, 2}, {"wvol", kWindowStrain, 0}, {"weq", kWindowStrain, 7}};
  if (!name) return 0;
  if (std::strcmp(name, "grey") == 0) return resident_frame_[0];
  for (const auto& f : kNamed)
    if (std::strcmp(name, f.name) == 0) return derived_[f.which].ptr[f.field];
  return 0;
}

bool OpticalFlowE::ComputeValidated(const Displacement& of, DevicePtr weight, float weight_min, unsigned step, float eps,
                                    float threshold, unsigned min_neighbours, unsigned mode, unsigned fill_passes, unsigned fields,
                                    f3d_validate_stats* stats)
{
  FieldSet& set = derived_[kValidated];
  DevicePtr d[3];
  if (!ResolveDisplacement(set, of, f3d_validate_displacement != nullptr, d)) return false;
  if (fields == 0 || (fields & ~(F3D_VALIDATE_R | F3D_VALIDATE_D)))
    return set.Fail("fields must be a non-empty combination of F3D_VALIDATE_R, F3D_VALIDATE_D");
  if (fill_passes && !(fields & F3D_VALIDATE_D)) return set.Fail("fill passes need the validated displacement (F3D_VALIDATE_D)");
  if (!set.Allocate(fields | (fill_passes ? kValidatedSpare : 0u))) return false;
  const f3d_size4 c = Container();
  f3d_validate_stats first = {};
  if (!set.Check(CheckDeviceError(f3d_set_container(&c))) ||
      !set.Check(CheckDeviceError(f3d_validate_displacement(d[0], d[1], d[2], weight, weight_min, step, eps, threshold, min_neighbours,
                                                            mode, set.ptr, fields, c.width, c.height, c.depth,
                                                            stats || fill_passes ? &first : nullptr))))
    return false;
  // the fill: no weight, nothing is an outlier, absent voxels with enough present neighbours receive their median
  for (unsigned pass = 0; pass < fill_passes && first.undefined; ++pass) {
    const DevicePtr out[4] = {0, set.ptr[4], set.ptr[5], set.ptr[6]};
    f3d_validate_stats filled = {};
    if (!set.Check(CheckDeviceError(f3d_validate_displacement(set.ptr[1], set.ptr[2], set.ptr[3], 0, 0.f, step, eps, INFINITY,
                                                              min_neighbours, F3D_VALIDATE_REPLACE, out, F3D_VALIDATE_D, c.width,
                                                              c.height, c.depth, &filled))))
      return false;
    for (int i = 1; i <= 3; ++i) std::swap(set.ptr[i], set.ptr[i + 3]);
    const bool fell = filled.undefined < first.undefined;
    first.replaced += filled.replaced;
    first.undefined = filled.undefined;
    if (!fell) break;
  }
  if (stats) *stats = first;
  return true;
}

// The coarse-to-fine solve on two frames that are already on the device (optical_flow_e.cpp:208-533 is the sequence of operator
// calls this reproduces: pre-blur; per level frames from the originals, flow from the level before, registration, solve, update,
// median).  Containers are named by what they hold:
//   blurred[2]   the two full-size frames the pyramid reads (pre-blurred copies, or the raw frames when sigma <= 0)
//   level[2]     the two frames at the current level; level[1] is replaced by its registered version
//   flow[3]      u, v, w so far        step[3]   the level's increments du, dv, dw (and, between levels, ping-pong room)
bool OpticalFlowE::RunPyramid(OperationParameters& params, DevicePtr raw_0, DevicePtr raw_1, bool raw_is_pooled,
                              const DevicePtr (*initial)[3])
{
  size_t warp_levels_count, outer_iterations_count, inner_iterations_count, median_radius;
  float warp_scale_factor, equation_alpha, equation_smoothness, equation_data, gaussian_sigma;
  GET_PARAM_OR_RETURN_VALUE(params, size_t, warp_levels_count, "warp_levels_count", false);
  GET_PARAM_OR_RETURN_VALUE(params, float, warp_scale_factor, "warp_scale_factor", false);
  GET_PARAM_OR_RETURN_VALUE(params, size_t, outer_iterations_count, "outer_iterations_count", false);
  GET_PARAM_OR_RETURN_VALUE(params, size_t, inner_iterations_count, "inner_iterations_count", false);
  GET_PARAM_OR_RETURN_VALUE(params, float, equation_alpha, "equation_alpha", false);
  GET_PARAM_OR_RETURN_VALUE(params, float, equation_smoothness, "equation_smoothness", false);
  GET_PARAM_OR_RETURN_VALUE(params, float, equation_data, "equation_data", false);
  GET_PARAM_OR_RETURN_VALUE(params, size_t, median_radius, "median_radius", false);
  GET_PARAM_OR_RETURN_VALUE(params, float, gaussian_sigma, "gaussian_sigma", false);
  calls::SolverSettings settings = {&outer_iterations_count, &inner_iterations_count, &equation_alpha, &equation_smoothness, &equation_data};

  if (!silent) std::printf("\nStarting optical flow computation...\n");

  DataSize4 whole = {dev_container_size_.width, dev_container_size_.height, dev_container_size_.depth, 0};
  const size_t deepest = GetMaxWarpLevel(whole.width, whole.height, whole.depth, warp_scale_factor);
  const int first_level = static_cast<int>(std::min(warp_levels_count, deepest)) - 1;
  const size_t container_rows = dev_container_size_.height * dev_container_size_.depth;
  const size_t container_row_bytes = dev_container_size_.width * sizeof(float);
  auto zero_container = [&](DevicePtr p) { CheckDeviceError(f3d_memset2d(p, dev_container_size_.pitch, 0, container_row_bytes, container_rows)); };
  OperationParameters bag;

  // ---- the frames the pyramid reads ------------------------------------------------------------------------------------------
  DevicePtr raw[2] = {raw_0, raw_1};
  DevicePtr blurred[2];
  if (gaussian_sigma > 0.0) {
    DevicePtr scratch = Borrow();
    for (int f = 0; f < 2; ++f) {
      blurred[f] = Borrow();
      cuop_convolution_.Execute(calls::Convolution(bag, &raw[f], &blurred[f], &scratch, &whole, &gaussian_sigma));
    }
    GiveBack(scratch);
    if (raw_is_pooled)
      for (DevicePtr p : raw) GiveBack(p);
  } else if (raw_is_pooled) {
    blurred[0] = raw[0];   // nothing to blur: the uploaded containers themselves
    blurred[1] = raw[1];
  } else {
    // resident frames must survive the solve (level 0 takes the containers of `blurred` over): work on copies
    for (int f = 0; f < 2; ++f) {
      blurred[f] = Borrow();
      CheckDeviceError(f3d_copy_d2d(blurred[f], raw[f], dev_container_size_.pitch * container_rows));
    }
  }

  DevicePtr level_frame[2] = {Borrow(), Borrow()};
  DevicePtr flow[3] = {Borrow(), Borrow(), Borrow()};
  DevicePtr step[3] = {Borrow(), Borrow(), Borrow()};
  const calls::Flow flow_roles = {&flow[0], &flow[1], &flow[2]}, step_roles = {&step[0], &step[1], &step[2]};

  // the initial flow as it is (whole containers: the box is the whole volume)
  auto copy_initial = [&]() {
    for (int c = 0; c < 3; ++c) CheckDeviceError(f3d_copy_d2d(flow[c], (*initial)[c], dev_container_size_.pitch * container_rows));
  };

  level_stats_.clear();
  if (first_level < 0) {  // no level requested: the flow is identically zero, or the initial flow
    if (initial)
      copy_initial();
    else
      for (DevicePtr p : flow) zero_container(p);
  }

  // `count` (<= 3) volumes of one box through the three resampling passes together: three launches, a scratch container each
  auto resample_together = [&](DevicePtr* in, DevicePtr* out, size_t count, DataSize4& from, DataSize4& to) {
    OperationParameters bags[3];
    DevicePtr scratch[3] = {0, 0, 0};
    for (size_t i = 0; i < count; ++i) {
      scratch[i] = Borrow();
      calls::Resample(bags[i], &in[i], &out[i], &scratch[i], &from, &to);
    }
    cuop_resample_.ExecuteBatch(bags, count);
    for (size_t i = 0; i < count; ++i) GiveBack(scratch[i]);
  };

  DataSize4 coarser = {0, 0, 0, 0};   // the box of the level before (none yet)
  for (int level = first_level; level >= 0; --level) {
    PyramidLevel geometry = GetLevel(whole, warp_scale_factor, level);
    DataSize4 box = geometry.size;
    const calls::Spacing spacing = {&geometry.hx, &geometry.hy, &geometry.hz};
    char range_name[64];
    std::snprintf(range_name, sizeof(range_name), "level %d (%zu x %zu x %zu)", level, box.width, box.height, box.depth);
    ProfilerRange level_range(range_name);
    if (!silent) std::printf("Solve level %2d (%4zu x%4zu x%4zu) \n", level, box.width, box.height, box.depth);

    // 1. the two frames at this size: always from the ORIGINAL-size frames; at the finest level those are the level's frames
    if (level == 0)
      for (int f = 0; f < 2; ++f) std::swap(blurred[f], level_frame[f]);
    else
      resample_together(blurred, level_frame, 2, whole, box);

    // 2. the flow so far at this size (zero, or the initial flow, before the first level): resampled into the increments' containers, roles swapped;
    //    the values are not rescaled -- the flow is kept in original-voxel units
    if (coarser.width == 0 && !initial) {
      for (DevicePtr p : flow) zero_container(p);
    } else if (coarser.width == 0) {
      // a given start: at the original size as it is, at any other level through the resampling the frames take (also when the
      // box happens to have the whole's dimensions)
      if (level == 0) {
        copy_initial();
      } else {
        DevicePtr from[3] = {(*initial)[0], (*initial)[1], (*initial)[2]};
        resample_together(from, flow, 3, whole, box);
      }
    } else {
      resample_together(flow, step, 3, coarser, box);
      for (int c = 0; c < 3; ++c) std::swap(flow[c], step[c]);
    }

    // 3. frame 1 registered with that flow
    {
      DevicePtr registered = Borrow();
      cuop_register_.Execute(calls::Registration(bag, &level_frame[0], &level_frame[1], flow_roles, &registered, &box, spacing));
      std::swap(level_frame[1], registered);
      GiveBack(registered);
    }
    if (collect_level_statistics) {
      LevelStatistics st;
      st.level = level;
      st.size = box;
      ResidualOf(level_frame[0], level_frame[1], box, st.before);
      level_stats_.push_back(st);
    }

    // 4. the increments of this level: weights + sweeps; five containers on loan for the duration.  The solve is asked to add the
    //    increments to the flow in its last launch (the sweep has both in registers); it says whether it did.
    bool flow_updated = false;
    {
      DevicePtr phi = Borrow(), ksi = Borrow();
      DevicePtr partner[3] = {Borrow(), Borrow(), Borrow()};
      const calls::Flow partner_roles = {&partner[0], &partner[1], &partner[2]};
      cuop_solve_.silent = silent;
      cuop_solve_.Execute(calls::SolveAndUpdate(bag, &level_frame[0], &level_frame[1], flow_roles, step_roles, partner_roles, &phi, &ksi,
                                                settings, &box, spacing, &flow_updated));
      for (DevicePtr p : {phi, ksi, partner[0], partner[1], partner[2]}) GiveBack(p);
    }

    // 5. flow += increments, then the median of every component.  The components are independent through both, so the three go out
    //    in one launch each; the increments are consumed by "+=", so their containers receive the filtered flow and the roles swap
    //    (the reference filters through one scratch container, a component at a time).  Where the solve has left the sums in the
    //    increments' containers there is nothing to add: the median reads them there and writes the flow's containers, no swap.
    {
      OperationParameters bags[3];
      if (flow_updated) {
        for (int c = 0; c < 3; ++c) calls::Median(bags[c], &step[c], &flow[c], &box, &median_radius);
        cuop_median_.ExecuteBatch(bags, 3);
      } else {
        for (int c = 0; c < 3; ++c) calls::Add(bags[c], &flow[c], &step[c], &box);
        cuop_add_.ExecuteBatch(bags, 3);
        for (int c = 0; c < 3; ++c) calls::Median(bags[c], &flow[c], &step[c], &box, &median_radius);
        cuop_median_.ExecuteBatch(bags, 3);
        for (int c = 0; c < 3; ++c) std::swap(flow[c], step[c]);
      }
    }

    if (collect_level_statistics) {
      float mn = 0.f, mx = 0.f;
      double sum = 0.0;
      if (!CheckDeviceError(f3d_flow_stats(flow[0], flow[1], flow[2], box.width, box.height, box.depth, nullptr, &mn, &mx, &sum))) {
        const double n = static_cast<double>(box.width) * static_cast<double>(box.height) * static_cast<double>(box.depth);
        level_stats_.back().flow = {mn, mx, static_cast<float>(sum / n)};
      }
      if (!silent) {
        const LevelStatistics& st = level_stats_.back();
        std::printf("  residual before the solve: rms %.5f  mean |.| %.5f  max %.4f;  flow after it: min %.4f  max %.4f  avg %.4f\n",
                    st.before.rms, st.before.mean_abs, st.before.max_abs, st.flow.min, st.flow.max, st.flow.avg);
      }
    }
    coarser = box;
  }

  // (u, v, w) stay out until they are downloaded or taken; everything else returns to the pool
  for (int c = 0; c < 3; ++c) result_flow_[c] = flow[c];
  for (DevicePtr p : {blurred[0], blurred[1], level_frame[0], level_frame[1], step[0], step[1], step[2]}) GiveBack(p);
  return true;
}

void OpticalFlowE::Destroy()
{
  for (CudaOperationBase* cuop : cuda_operations_) cuop->Destroy();
  ReleaseResult();
  trajectory_.Release();
  ReleaseInitialFlow();
  for (FieldSet& set : derived_) set.Release();
  ReleaseWindowGradient();
  size_t freed = 0;
  while (!free_containers_.empty()) {
    CheckDeviceError(f3d_free(free_containers_.back()));
    free_containers_.pop_back();
    ++freed;
  }
  if (sequence_frame_[2]) {  // sequence mode: the three frame containers, two of which resident_frame_ points at
    for (DevicePtr& p : sequence_frame_) {
      if (p) CheckDeviceError(f3d_free(p));
      p = 0;
    }
    resident_frame_[0] = resident_frame_[1] = 0;
  }
  for (DevicePtr& p : resident_frame_) {
    if (p) CheckDeviceError(f3d_free(p));
    p = 0;
  }
  if (freed && freed != kContainers + extra_containers_) std::printf("Warning. Not all device memory allocations were freed.\n");
  extra_containers_ = 0;
  initialized_ = false;
}
