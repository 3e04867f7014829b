// Flow drivers of the drop-in surface (interfaces of src/optical_flow/optical_flow_base.h:24-45 and
// src/optical_flow/optical_flow_e.h:38-66), re-implemented on the operator layer in operations.h.
#ifndef F3D_HOST_OPTICAL_FLOW_H_
#define F3D_HOST_OPTICAL_FLOW_H_

#include <string>
#include <vector>

#include "data_types.h"
#include "f3d_host.h"
#include "operations.h"

// One level of the coarse-to-fine pyramid: size and grid spacing in original-voxel units.
struct PyramidLevel {
  DataSize4 size;
  float hx, hy, hz;
};

class OpticalFlowBase {
 public:
  const char* GetName() const { return name_; }

  virtual bool Initialize(const DataSize4& data_size) = 0;
  virtual void ComputeFlow(Data3D& frame_0, Data3D& frame_1, Data3D& flow_u, Data3D& flow_v, Data3D& flow_w,
                           OperationParameters& params);
  virtual void Destroy();
  virtual ~OpticalFlowBase();

  // Pyramid depth rule and per-level geometry (optical_flow_base.cpp:31-56, optical_flow_e.cpp:262-268);
  // public and static so the slab planner and the tests can use them without a device.
  static size_t GetMaxWarpLevel(size_t width, size_t height, size_t depth, float scale_factor);
  static PyramidLevel GetLevel(const DataSize4& original, float scale_factor, int level);

 protected:
  explicit OpticalFlowBase(const char* name) : name_(name) {}
  bool IsInitialized() const;

  bool initialized_ = false;

 private:
  const char* name_ = nullptr;
};

// Everything resident on one GPU: 15 pitched containers of the original size, pre-blur, then per level
// {resample frames, upsample flow, warp, solve, add, median}.
class OpticalFlowE : public OpticalFlowBase {
 public:
  OpticalFlowE();
  ~OpticalFlowE() override;

  bool Initialize(const DataSize4& data_size) override;
  void ComputeFlow(Data3D& frame_0, Data3D& frame_1, Data3D& flow_u, Data3D& flow_v, Data3D& flow_w,
                   OperationParameters& params) override;
  void Destroy() override;

  bool silent = false;

  // Device-resident variant (benchmarks, frame sequences): two extra containers hold the raw frames in HBM,
  // ComputeFlowResident() runs the same pyramid from them and leaves (u, v, w) on the device until
  // DownloadFlow().  The raw frames are never overwritten, so the call can be repeated.
  bool AllocateResidentFrames();
  void UploadResidentFrames(Data3D& frame_0, Data3D& frame_1);
  DevicePtr ResidentFrame(int which) const { return resident_frame_[which ? 1 : 0]; }
  const DataSize4& ContainerSize() const { return dev_container_size_; }
  void ComputeFlowResident(OperationParameters& params);
  void DownloadFlow(Data3D& flow_u, Data3D& flow_v, Data3D& flow_w);

  // Frame sequences (bin/flow3d --frames f0 f1 f2 ...).  The reference sets the driver up, uploads both
  // frames, solves, downloads and tears everything down for every pair (src/main.cpp:132-185).  Here the frames live in THREE
  // rotating device containers, so a frame is uploaded once although it serves two pairs, and a solve is split into
  // BeginComputeFlowResident (enqueues the whole pyramid on the library stream and returns) and EndComputeFlowResident (waits):
  // in between the caller reads the next file and uploads it on a copy queue, and downloads / writes the previous pair's flow,
  // which TakeResult() has moved out of the driver's way (three spare containers join the pool the first time).
  bool AllocateSequenceFrames();                                    // the third frame container
  DevicePtr SequenceFrame(int slot) const { return sequence_frame_[slot % 3]; }
  void SelectResidentPair(int slot_0, int slot_1);                  // which two of the three are frame_0 / frame_1 of the next solve
  void BeginComputeFlowResident(OperationParameters& params);
  void EndComputeFlowResident();
  bool TakeResult(DevicePtr (&flow)[3]);                            // the caller owns the three containers until GiveResultBack
  void GiveResultBack(DevicePtr (&flow)[3]);
  // min / max / average magnitude of the flow ComputeFlowResident() left on the device (CudaOperationStat); false when there
  // is none
  bool ResultStatistics(Stat3& stat);
  float LastDeviceSeconds() const { return last_device_seconds_; }

  // Diagnostics per pyramid level and for the result (the reference's counterpart is the disabled
  // "apply the flow and dump the registered volume" block, optical_flow_e.cpp:536-571).  Collected only when asked for: every
  // level costs two small reductions and a read-back.
  struct Residual {
    double rms = 0.0, mean_abs = 0.0;
    float max_abs = 0.f;
  };
  struct LevelStatistics {
    int level = 0;
    DataSize4 size = {0, 0, 0, 0};
    Residual before;  // frame_1 warped with the flow handed down from the coarser level, against frame_0, at this level's size
    Stat3 flow = {0.f, 0.f, 0.f};  // min / max / average flow magnitude after this level's median
  };
  bool collect_level_statistics = false;
  const std::vector<LevelStatistics>& LevelStats() const { return level_stats_; }
  // The reference's debug block made measurable: the ORIGINAL frame_1 registered with the final flow (h = 1) against the
  // original frame_0, and the same difference without any flow.  Needs the resident raw frames and a computed flow.
  bool FinalResidual(Residual& registered, Residual& unregistered);

  // Trajectory of a frame sequence: the displacement of every voxel of frame 0 to the frame the sequence has reached (Lagrangian,
  // frame 0's grid, voxel units), kept in three containers of its own that are allocated on request and freed by Destroy().  Each
  // pair's flow is composed into it on the device (f3d_compose_flow: acc += flow sampled at x + acc; a point that leaves the
  // volume becomes NaN and stays NaN).  Compose enqueues on the library stream and does not wait.  Every call returns false with
  // TrajectoryError() set when it cannot run -- among other reasons when the device library lacks f3d_compose_flow.
  bool AllocateTrajectory();                                        // three containers; false with a message when they do not fit
  bool ResetTrajectory();                                           // allocates on first use, then zero
  bool ComposeTrajectory();                                         // with the flow ComputeFlowResident() left on the device
  bool ComposeTrajectory(const DevicePtr (&flow)[3]);               // with three given containers (TakeResult's)
  bool DownloadTrajectory(Data3D& u, Data3D& v, Data3D& w, unsigned long long* lost);  // lost: voxels whose u is NaN
  DevicePtr TrajectoryContainer(int component) const { return trajectory_.ptr[component]; }
  void ReleaseTrajectory() { trajectory_.Release(); }
  const std::string& TrajectoryError() const { return trajectory_.error; }

  // Derived fields of a displacement (include/f3d.h has the definitions):
  //   kStrain     f3d_flow_strain: vol = J - 1, Green-Lagrange E, equivalent strain.  Eight outputs in the order vol, exx, eyy, ezz,
  //               exy, exz, eyz, eq, selected in groups by F3D_STRAIN_* bits.
  //   kPrincipal  f3d_principal_strain: e1 >= e2 >= e3 of E, maximum shear, the directions of e1 and e3.  Ten outputs in the order
  //               e1, e2, e3, gmax, d1x, d1y, d1z, d3x, d3y, d3z, selected by F3D_PRINCIPAL_VALUES / _SHEAR / _DIR1 / _DIR3.
  //   kPolar      f3d_polar_decomposition: the rotation angle and rotation vector of the R of F = R U, and the principal stretches.
  //               Seven outputs in the order theta, rx, ry, rz, l1, l2, l3, selected by F3D_POLAR_ANGLE / _VECTOR / _STRETCH.
  //   kInverse    f3d_invert_displacement: g on the deformed frame's grid with g(y) = -d(y + g(y)), and the round-trip residual
  //               of the stored g.  Four outputs g_u, g_v, g_w, err, always all of them (fields is ignored).
  //   kMatch      f3d_local_correlation of frame 0 against frame 1 carried onto frame 0's grid through the displacement
  //               (f3d_carry_field, linear; NaN where the point leaves the volume).  Three outputs warped, zncc, rmsd selected by
  //               kMatchWarped / kMatchZncc / kMatchRmsd.  The warped container is the kernel's input and is always allocated; it
  //               is downloaded only when selected.
  //   kMotion     f3d_motion_sums, the host solve (motion_fit.h) and f3d_remove_motion: the displacement with its best translation,
  //               rigid motion or affine map taken out.  Three outputs, the residual u, v, w, always all of them.
  //   kValidated  f3d_validate_displacement: the normalised median test and the repair of what it rejects.  Four outputs r, u, v, w
  //               selected by F3D_VALIDATE_R (r) and F3D_VALIDATE_D (u, v, w); the fill passes keep a second u, v, w beside them.
  //   kLabelMotion f3d_label_motion_sums, the host solve per label (motion_fit.h) and f3d_remove_label_motion: the displacement with the
  //               fit of each voxel's label taken out.  Three outputs, the residual u, v, w, always all of them, and a fourth container
  //               that holds the labels (UploadLabels; never downloaded).  A second label volume (UploadLabelsB, ComputeLabelsB) lives
  //               in a slot behind these four that no mask selects, and is freed with them.
  //   kWindowStrain f3d_window_strain: the strain fields of kStrain from the least-squares gradient over a (2 radius + 1)^3 window, and
  //               that gradient.  Seventeen outputs in the order vol, exx, eyy, ezz, exy, exz, eyz, eq, G00 .. G22, selected by
  //               F3D_STRAIN_VOL / _E / _EQ and F3D_WSTRAIN_G.
  //   kWindowPrincipal f3d_window_strain's gradient (F3D_WSTRAIN_G alone) into nine containers the driver keeps to itself, then
  //               f3d_principal_from_gradient on them: kPrincipal's ten outputs and bits from the least-squares gradient.
  //   kWindowPolar the same with f3d_polar_from_gradient: kPolar's seven outputs and bits.  Both depend on their arguments only: no
  //               earlier ComputeWindowStrain is needed, and what kWindowStrain holds is left as it is.  The nine gradient
  //               containers are allocated on first use and freed when neither kind holds a container any more, and by Destroy().
  // Each selected output gets a container of its own, allocated on first use and freed by ReleaseDerived() and Destroy().  Compute
  // enqueues on the library stream and waits only when stats is given.  Every call returns false with DerivedError() set when it
  // cannot run -- among other reasons when the device library lacks the entry point.
  enum Derived { kStrain = 0, kPrincipal, kInverse, kMatch, kMotion, kValidated, kPolar, kLabelMotion, kWindowStrain, kWindowPrincipal,
                 kWindowPolar, kDerivedCount };
  static constexpr int kMaxDerivedFields = 17;  // the most outputs a Derived has (kWindowStrain)
  enum MatchField : unsigned { kMatchWarped = 1u, kMatchZncc = 2u, kMatchRmsd = 4u };
  // the displacement a derived field is computed of
  struct Displacement {
    enum Kind { kHeldFlow, kTrajectory, kContainers } kind;
    DevicePtr containers[3];
  };
  static Displacement HeldFlow() { return {Displacement::kHeldFlow, {0, 0, 0}}; }      // what ComputeFlowResident() left on the device
  static Displacement Trajectory() { return {Displacement::kTrajectory, {0, 0, 0}}; }  // ResetTrajectory first
  static Displacement Containers(const DevicePtr (&d)[3]) { return {Displacement::kContainers, {d[0], d[1], d[2]}}; }  // TakeResult's
  // Initial flow: a displacement a solve starts its pyramid from instead of zero (a guess from outside, the flow of the pair before,
  // the displacement frame 0 -> frame k-1 for a direct solve frame 0 -> frame k).  It is data in three containers of the driver's
  // own, allocated on first use and kept until it is set again, ReleaseInitialFlow() or Destroy() -- no solve consumes it, and only
  // the calls that are told to (use_initial) read it.  Each setter fills the containers through f3d_initial_flow (include/f3d.h:
  // a voxel with a component that is not finite becomes zero) and, when info is given, waits for the stream and reports what was
  // found.  The second setter copies on the library stream at once, so the containers of `of` may go back to the pool afterwards.
  // Every call returns false with InitialFlowError() set when it cannot run -- among other reasons when the device library lacks
  // f3d_initial_flow.  The pyramid resamples the three components from the original size to its first level (they are copied when
  // that level is the original size, level 0); values are not rescaled: a flow is in original-voxel units at every level.
  bool SetInitialFlow(Data3D& u, Data3D& v, Data3D& w, f3d_initial_info* info);
  bool SetInitialFlow(const Displacement& of, f3d_initial_info* info);
  bool HasInitialFlow() const { return initial_.ptr[0] != 0 && initial_set_; }
  bool DownloadInitialFlow(Data3D& u, Data3D& v, Data3D& w);
  void ReleaseInitialFlow();
  const std::string& InitialFlowError() const { return initial_.error; }
  // The guess from the frames themselves (include/f3d_block_match.h).  BlockMatch searches the resident pair on the
  // grid f3d_block_match_layout lays (f3d_block_match on the library stream, then f3d_block_match_solve); range null: the finite
  // minimum and maximum of frame 0 (f3d_value_range).  The records, the rows and the grid stay with the driver.
  // SetInitialFromNodes puts the node vectors of the last BlockMatch through f3d_validate_displacement as an nx x ny x nz volume
  // (replace mode, step 1, eps 0.1, threshold 2, 9 neighbours: the defaults of --validate), expands the result into the containers of
  // the initial flow (f3d_expand_nodes) and prepares them (f3d_initial_flow).  False with InitialFlowError() set when they cannot
  // run, among other reasons when the device library lacks one of the entries.
  struct BlockMatchParams {
    int step = 16, window = 8, radius[3] = {8, 8, 8};
    size_t bins = 256;
    const float* range = nullptr;  // lo, hi
    double min_zncc = 0.5;
  };
  bool BlockMatch(const BlockMatchParams& params, const int* centre, f3d_block_match_info* info, f3d_block_match_summary* summary);
  const f3d_block_match_grid& BlockMatchGrid() const { return match_grid_; }
  const std::vector<f3d_block_match_record>& BlockMatchRecords() const { return match_records_; }
  const std::vector<f3d_block_match_node>& BlockMatchNodes() const { return match_nodes_; }
  bool SetInitialFromNodes(f3d_validate_stats* validated, f3d_initial_info* info);
  // Subset correlation on the resident pair (include/f3d_subset_match.h): f3d_subset_match on the grid
  // f3d_subset_match_layout lays, on the library stream, then f3d_subset_match_table.  The start translations come from `start`
  // (the start gradients are zero): kSubsetZero; kSubsetNodes, the block-match table the driver holds, each subset node taking the
  // vector of the block-match node nearest to it per axis (the lower of two equally near), which is NaN unless that node is ok or
  // edge; kSubsetFlow, the held flow read at the node voxels.  Whenever a flow is held, its values at the node voxels are the
  // comparison of the table.  The records, the rows and the grid stay with the driver.  False with InitialFlowError() set.
  enum SubsetStart { kSubsetZero = 0, kSubsetNodes = 1, kSubsetFlow = 2 };
  struct SubsetMatchParams {
    int step = 16, window = 8, model = F3D_SUBSET_AFFINE, max_iterations = 20, start = kSubsetZero;
    double tolerance = 1e-3, reach = 0.0;  // reach 0: the window radius
    double min_zncc = 0.8;
  };
  bool SubsetMatch(const SubsetMatchParams& params, f3d_subset_match_info* info, f3d_subset_match_summary* summary);
  const f3d_subset_match_grid& SubsetMatchGrid() const { return subset_grid_; }
  const std::vector<f3d_subset_match_record>& SubsetMatchRecords() const { return subset_records_; }
  const std::vector<f3d_subset_match_node>& SubsetMatchNodes() const { return subset_nodes_; }
  // The three compute calls started from the initial flow that is held (use_initial) or, with use_initial false, exactly as their
  // namesakes above; false with InitialFlowError() set when use_initial is asked for and none is held.
  bool ComputeFlow(Data3D& frame_0, Data3D& frame_1, Data3D& flow_u, Data3D& flow_v, Data3D& flow_w, OperationParameters& params,
                   bool use_initial);
  bool ComputeFlowResident(OperationParameters& params, bool use_initial);
  bool BeginComputeFlowResident(OperationParameters& params, bool use_initial);

  bool ComputeStrain(const Displacement& of, unsigned fields, f3d_strain_stats* stats);
  bool ComputePrincipal(const Displacement& of, unsigned fields, f3d_principal_stats* stats);
  // radius 1 .. 3; a voxel with fewer than min_count (1 .. (2 radius + 1)^3) present points in its window is undefined
  bool ComputeWindowStrain(const Displacement& of, unsigned fields, unsigned radius, unsigned min_count,
                           f3d_window_strain_stats* stats);
  bool ComputePolar(const Displacement& of, unsigned fields, f3d_polar_stats* stats);
  // fields and stats as in ComputePrincipal / ComputePolar, radius and min_count as in ComputeWindowStrain
  bool ComputeWindowPrincipal(const Displacement& of, unsigned fields, unsigned radius, unsigned min_count, f3d_principal_stats* stats);
  bool ComputeWindowPolar(const Displacement& of, unsigned fields, unsigned radius, unsigned min_count, f3d_polar_stats* stats);
  bool ComputeInverse(const Displacement& of, unsigned iterations, float tolerance, f3d_inverse_stats* stats);
  // frame_0 / frame_1: the containers of the two frames the displacement belongs to; 0 means the resident pair.  A trajectory is
  // refused: frame 0 of a sequence is not kept.
  bool ComputeMatch(const Displacement& of, DevicePtr frame_0, DevicePtr frame_1, unsigned fields, unsigned radius, float threshold,
                    f3d_correlation_stats* stats);
  // model: F3D_MOTION_*.  weight: a container whose voxels below weight_min (or NaN) take no part in the fit, 0 for none -- in
  // practice DerivedContainer(kMatch, 1), the zncc of the same pair.  Enqueues the sums, waits for them, solves on the host, enqueues
  // the subtraction and waits again only when residual is given.  fit (required) receives the fit with its centre.
  bool ComputeMotion(const Displacement& of, int model, DevicePtr weight, float weight_min, f3d_motion_fit* fit,
                     f3d_motion_residual* residual);
  // weight / weight_min as in ComputeMotion; step, eps, threshold, min_neighbours, mode (F3D_VALIDATE_MARK / _REPLACE) and fields
  // (F3D_VALIDATE_R | F3D_VALIDATE_D) as in include/f3d.h.  fill_passes (needs F3D_VALIDATE_D): after the first call up to that many
  // further calls on its own output with threshold +inf, no weight and F3D_VALIDATE_REPLACE, between two container sets: each gives
  // the absent voxels with enough present neighbours their median; they stop when no voxel is undefined or the count stops falling,
  // and they wait for the stream.  stats (nullable) are those of the first call with replaced and undefined brought to the final
  // state; r is that of the first call.  DerivedContainer(kValidated, 1 .. 3) is the validated displacement afterwards, which
  // Containers() hands to the strain, principal strain, polar and motion calls.
  bool ComputeValidated(const Displacement& of, DevicePtr weight, float weight_min, unsigned step, float eps, float threshold,
                        unsigned min_neighbours, unsigned mode, unsigned fill_passes, unsigned fields, f3d_validate_stats* stats);
  // Per-label motion.  UploadLabels: width * height * depth int32 on frame 0's grid (0 background, 1 .. n_labels the bodies) into a
  // container the driver keeps until ReleaseDerived(kLabelMotion) or Destroy().  ComputeLabelMotion: the sums of every label, waits,
  // the solves on the host (fits and status: n_labels entries each, required; a label with fewer than min_voxels voxels is not
  // fitted), the subtraction, and -- when rms_after (n_labels entries) is given -- the sums of the residual and a second wait:
  // rms_after[L-1] = sqrt((Sdd_u + Sdd_v + Sdd_w) / n) of label L's residual, NaN where the label has none.  info (nullable) are the
  // voxel counts of the first sums.
  bool UploadLabels(const int* labels);
  bool ComputeLabelMotion(const Displacement& of, size_t n_labels, int model, unsigned long long min_voxels, f3d_motion_fit* fits,
                          int* status, double* rms_after, f3d_label_info* info);
  // Contacts between the labels UploadLabels left on the device (f3d_label_contacts of include/f3d.h): the capacity starts at
  // 8 * n_labels (at most 2^20) and doubles until the table is complete; contacts receives them sorted by (lo, hi), info (required) the counters of
  // the call that sufficed.  Waits for the stream.  Errors are reported through DerivedError(kLabelMotion), whose labels these are.
  bool ComputeContacts(const Displacement& of, size_t n_labels, std::vector<f3d_contact>* contacts, f3d_contact_info* info);
  // The labels made on the device instead of uploaded (f3d_label_components of include/f3d.h): the connected bodies of the voxels of
  // `frame` with lo <= value <= hi, those of at least min_voxels voxels numbered 1 .. info->n_labels, into the container UploadLabels
  // fills; ComputeLabelMotion and ComputeContacts then run on them with n_labels = info->n_labels.  frame 0 means the resident frame
  // 0, the one ComputeMatch uses: the RAW frame as it was uploaded (the pre-blurred copies of the pyramid live in pooled containers and
  // are not kept).  sizes (nullable) receives the size of every label, which costs a second run of the entry once their number is
  // known; info is required.  Waits for the stream.  DownloadLabels copies the label container, however it was filled, to
  // width * height * depth int32.  Errors of both are reported through DerivedError(kLabelMotion).
  bool ComputeLabels(DevicePtr frame, float lo, float hi, unsigned long long min_voxels, std::vector<unsigned long long>* sizes,
                     f3d_component_info* info);
  // The same with touching bodies taken apart (f3d_split_components of include/f3d.h): the cores are the foreground voxels whose
  // squared distance to the background is at least core_d2, and every foreground voxel goes to the nearest core of its component.  It
  // fills the same label container, so ComputeLabelMotion and ComputeContacts run on it unchanged.
  bool ComputeSplitLabels(DevicePtr frame, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels,
                          std::vector<unsigned long long>* sizes, f3d_split_info* info);
  bool DownloadLabels(int* labels);
  // The shapes of the labels on the device (f3d_label_shape_sums of include/f3d.h, then f3d_label_shape_solve of include/f3d_host.h):
  // shapes has n_labels entries (required), info is nullable.  It needs the label container alone, however it was filled, so it runs
  // before any solve.  Waits for the stream.  Errors are reported through DerivedError(kLabelMotion), whose labels these are.
  bool ComputeLabelShapes(size_t n_labels, f3d_label_shape* shapes, f3d_label_shape_info* info);
  // Statistics of a scalar field over the labels on the device (f3d_label_field_sums of include/f3d.h, then f3d_label_field_solve of
  // include/f3d_host.h).  field: a container of the driver's geometry -- DerivedContainer() or NamedField() of a computed field -- or 0
  // for the resident frame 0.  range: {lo, hi}, null iff bins == 0; counts: n_labels * bins entries, null iff bins == 0; stats has
  // n_labels entries (required); info and summary are nullable.  PaintLabels: values[l - 1] into the voxels of label l and NaN elsewhere
  // (f3d_paint_labels) in a pooled container, and down to out (width * height * depth floats).  Both wait for the stream; errors are
  // reported through DerivedError(kLabelMotion), whose labels these are.  NamedField: the container of grey (the resident frame 0),
  // vol, eq (kStrain), gmax (kPrincipal), angle (kPolar), zncc, rmsd (kMatch), wvol, weq (kWindowStrain); 0 for another name and
  // until the field is computed.
  bool ComputeLabelField(DevicePtr field, size_t n_labels, int shift, const float* range, size_t bins, unsigned long long min_voxels,
                         f3d_label_field_stat* stats, unsigned* counts, f3d_label_field_info* info,
                         f3d_label_field_summary* summary = nullptr);
  // the finite minimum and maximum of `field` (0: the resident frame 0) over the voxels whose label is not 0 (f3d_value_range masked by
  // the labels): what the shift and the range of ComputeLabelField are chosen from when the caller gives none
  bool LabelFieldRange(DevicePtr field, float* lo, float* hi, f3d_range_info* info);
  bool PaintLabels(const float* values, size_t n_labels, float* out);
  bool PaintLabels(const float* values, size_t n_labels, Data3D* out) { return PaintLabels(values, n_labels, out ? out->DataPtr() : nullptr); }
  DevicePtr NamedField(const char* name) const;
  // A second label volume, "B", beside the one UploadLabels fills ("A"): the bodies of a later frame, on the grid a displacement
  // leads to, in a container of its own that goes with ReleaseDerived(kLabelMotion) or Destroy().  UploadLabelsB / DownloadLabelsB as
  // their namesakes.  ComputeLabelsB: f3d_label_components (core_d2 == 0; only the first eight counters of info, those of
  // f3d_component_info, are then written, the rest are 0) or f3d_split_components (core_d2 >= 1) of `frame` into B; frame 0 means the
  // resident frame 1, the RAW later frame of the pair; sizes is nullable, info required.  ComputeOverlap: f3d_label_overlap of A and B
  // through `of` (include/f3d.h), the capacity starting at 8 * (n_a + n_b) (at most 2^20) and doubling until the table is complete;
  // rows receives them sorted by (a, b), info (required) the counters of the call that sufficed.  RelabelB: f3d_relabel_labels of B
  // in place (map has n_b entries).  All wait for the stream but RelabelB; errors are reported through DerivedError(kLabelMotion).
  bool UploadLabelsB(const int* labels);
  bool ComputeLabelsB(DevicePtr frame, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels,
                      std::vector<unsigned long long>* sizes, f3d_split_info* info);
  bool ComputeOverlap(const Displacement& of, size_t n_a, size_t n_b, std::vector<f3d_overlap>* rows, f3d_overlap_info* info);
  bool RelabelB(const int* map, size_t n_b);
  bool DownloadLabelsB(int* labels);
  // The histogram of the frame ComputeLabels thresholds (f3d_histogram of include/f3d.h; frame 0 means the resident frame 0).  range:
  // {lo, hi}, or null for the frame's finite minimum and maximum (f3d_value_range); a constant frame and one without a finite voxel
  // then fail with a message that says which.  counts has bins entries, info is required, *lo_used and *hi_used (nullable) receive the
  // bounds the bins were laid over.  Waits for the stream.  Errors are reported through DerivedError(kLabelMotion).
  bool ComputeHistogram(DevicePtr frame, const float* range, size_t bins, unsigned long long* counts, f3d_histogram_info* info,
                        float* lo_used, float* hi_used);
  static int DerivedFieldCount(Derived which);
  static bool DerivedSelected(Derived which, int field, unsigned fields);
  DevicePtr DerivedContainer(Derived which, int field) const { return derived_[which].ptr[field]; }  // 0 until computed
  bool DownloadDerived(Derived which, Data3D* const* out, unsigned fields) { return derived_[which].Download(out, fields); }
  void ReleaseDerived(Derived which);
  const std::string& DerivedError(Derived which) const { return derived_[which].error; }

 private:
  static constexpr size_t kContainers = 15;  // optical_flow_e.h:40

  bool InitCudaMemory();
  bool InitCudaOperations();
  DevicePtr Borrow();
  void GiveBack(DevicePtr p);
  // initial (nullable): the three full-size components the first level starts from instead of zero
  bool RunPyramid(OperationParameters& params, DevicePtr raw_0, DevicePtr raw_1, bool raw_is_pooled,
                  const DevicePtr (*initial)[3] = nullptr);
  bool CheckInitial(bool use_initial);  // false with the error set when use_initial is asked for and no initial flow is held
  void ReleaseResult();

  DataSize4 dev_container_size_ = {0, 0, 0, 0};
  std::vector<DevicePtr> free_containers_;  // LIFO like the reference's std::stack
  DevicePtr resident_frame_[2] = {0, 0};
  DevicePtr sequence_frame_[3] = {0, 0, 0};  // sequence mode: resident_frame_ aliases two of these
  size_t extra_containers_ = 0;               // spares allocated for TakeResult
  f3d_event ev_begin_ = nullptr, ev_end_ = nullptr;
  DevicePtr result_flow_[3] = {0, 0, 0};
  float last_device_seconds_ = 0.f;
  // A set of device containers one feature owns: the trajectory's three, the outputs of a derived field.
  struct FieldSet {
    OpticalFlowE* driver;
    int count;
    const unsigned* groups;    // the F3D_* bit that selects each field; null: every field, whatever the mask
    const char* fit;           // what Allocate says when the device has no room
    const char* not_computed;  // what Download says of a field without a container, and of one without a host volume
    const char* no_volume;
    const char* no_entry;      // what Compute says when the device library lacks the entry point, and when there is no displacement
    const char* no_displacement;
    DevicePtr ptr[kMaxDerivedFields] = {};
    std::string error;

    bool Selected(int field, unsigned mask) const { return !groups || (mask & groups[field]) != 0; }
    bool Fail(const char* what);
    bool Check(bool device_error) { return device_error ? Fail(f3d_last_error()) : true; }  // of a CheckDeviceError(call)
    bool Allocate(unsigned mask);                      // a container for each selected field that has none
    bool Download(Data3D* const* out, unsigned mask);  // the selected fields (entries of others ignored)
    void Release();
  };
  FieldSet trajectory_;
  FieldSet initial_;
  bool initial_set_ = false;  // the three containers hold a prepared flow (they can exist without one after a failed upload)
  f3d_block_match_grid match_grid_ = {};  // of the last BlockMatch; match_nodes_ empty: none yet
  std::vector<f3d_block_match_record> match_records_;
  std::vector<f3d_block_match_node> match_nodes_;
  f3d_subset_match_grid subset_grid_ = {};  // of the last SubsetMatch; subset_nodes_ empty: none yet
  std::vector<f3d_subset_match_record> subset_records_;
  std::vector<f3d_subset_match_node> subset_nodes_;
  FieldSet derived_[kDerivedCount];
  // the gradient of kWindowPrincipal and kWindowPolar (G00 .. G22), never downloaded
  DevicePtr window_gradient_[9] = {};
  // the window pass of both: checks, the nine containers on first use, f3d_window_strain with F3D_WSTRAIN_G alone into them
  bool ComputeWindowGradient(FieldSet& set, const Displacement& of, bool have_entry, unsigned radius, unsigned min_count);
  void ReleaseWindowGradient();
  // the slot of derived_[kLabelMotion] that holds the second label volume, behind the set's four fields
  static constexpr int kLabelsBSlot = 4;
  bool AllocateLabelsB();
  // clears set's error and gives the three containers of `of`, or fails with the text that says what is missing
  bool ResolveDisplacement(FieldSet& set, const Displacement& of, bool have_entry, DevicePtr (&disp)[3]);
  f3d_size4 Container() const;
  std::vector<LevelStatistics> level_stats_;
  bool ResidualOf(DevicePtr frame_0, DevicePtr warped, const DataSize4& size, Residual& out);

  CudaOperationAdd cuop_add_;
  CudaOperationMedian cuop_median_;
  CudaOperationConvolution3D cuop_convolution_;
  CudaOperationRegistration cuop_register_;
  CudaOperationResample cuop_resample_;
  CudaOperationSolve cuop_solve_;
  CudaOperationStat cuop_stat_;  // not in the list below: the reference's single-GPU driver has six operators
  std::vector<CudaOperationBase*> cuda_operations_;
};

#endif
