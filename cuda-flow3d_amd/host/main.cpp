// flow3d -- command-line application of the MI355X-native 3-D optical-flow solver.
//
// Mirrors what src/main.cpp:53-239 of the reference does (load a pair of RAW volumes, run OpticalFlowE with
// the nine-key parameter bag, write flow-u/v/w as RAW float32), with the compile-time constants turned into
// flags:  flow3d --dims W H D --frames f0.raw f1.raw [f2.raw ...] [--f32] [--out prefix] [--levels N] [--scale s]
//                [--outer N] [--inner N] [--alpha a] [--eps-smooth e] [--eps-data e] [--median r] [--sigma s]
//                [--synthetic] [--vtk] [--stats] [--silent] [--partial [--full] [--budget-mb N]] [--concurrent N] [--cumulative]
//                [--initial-flow U V W] [--warm-start | --total]
//                [--strain vol,e,eq] [--principal val,shear,dir1,dir3] [--rotation angle,vector,stretch] [--inverse]
//                [--window-strain vol,e,eq,grad [--window-radius R] [--window-min-count K]]
//                [--window-principal val,shear,dir1,dir3] [--window-rotation angle,vector,stretch]
//                [--match warped,zncc,rmsd [--match-radius R]]
//                [--detrend translation|rigid|affine [--detrend-min-zncc T]]
//                [--validate mark|replace [--validate-step S] [--validate-threshold T] [--validate-eps E]
//                 [--validate-min-neighbours K] [--validate-fill N] [--validate-min-zncc Z] [--use-validated]]
//                [--labels FILE --label-motion translation|rigid|affine [--label-min-voxels K]]
//                [--labels FILE --contacts [--contact-min-faces K]]
//                [--segment LO:HI [--segment-min-voxels K]]
//                [--segment-split R | --segment-split-d2 N]
//                [--segment otsu|otsu1|otsu2 on either side of the colon] [--segment-bins B] [--segment-range A:B] [--histogram]
// More than two frames make a sequence: the driver, its containers and operators are set up once (the reference does
// Initialize / Destroy per pair, src/main.cpp:150,184) and the flow of every consecutive pair is written as
// <prefix>_<k>_flow-{u,v,w}-W-H-D.raw.  --partial runs the out-of-core driver (the reference's use_partial_gpu branch,
// src/main.cpp:187-220): volumes stay in host memory, output files end in "-partial.raw"; --full adds the pre-blur and the
// median the reference's piecemeal driver leaves out, which makes the result equal the resident mode's.
// --concurrent N solves N pairs of a sequence AT ONCE: N host threads, each with a driver and a lane of its own (f3d_lane_*: its
// own stream and container geometry), pair k going to thread k mod N.  Pair k+1 does not depend on pair k, and a small volume
// (up to ~128^3) is a chain of dependent launches of 10-20 us that leaves most of the chip idle: two such chains side by side
// nearly double the pairs per second.  Large volumes fill the chip by themselves and gain nothing.
// --cumulative (resident driver, pairs in order) also composes every pair's flow into the displacement of each voxel of frame 0 on
// the device (f3d_compose_flow) and writes <prefix>_<k>_disp-{u,v,w}-W-H-D.raw: frame 0 -> frame k+1 on frame 0's grid, NaN where
// the point has left the volume.
// --initial-flow U V W (resident driver, pairs in order) starts the pyramid of pair 0 from a displacement instead of zero: three float32
// raw files of W x H x D in the layout the flows are written in (a coarse DVC, an FE prediction, a rigid pre-registration).  A voxel
// with a component that is not finite starts from zero (f3d_initial_flow); one line per pair that starts from a displacement says how
// many such voxels there were, how many end points leave the volume and the largest component.
// --block-match (resident driver, pairs in order) makes that guess from the frames themselves: on a grid of nodes
// --block-match-step apart (default 16) the integer shift within --block-match-search R or RX:RY:RZ (default 8) that maximises the
// ZNCC of a window of radius --block-match-window (default 8) of the pair's first frame against its second, refined to a sub-voxel
// peak; nodes below --block-match-min-zncc (default 0.5) have no vector.  Per pair: <tag>_blockmatch.csv (per node the position, the
// shift, the offset, the ZNCC, the status and the counts of candidates), one line (nodes ok / low / flat / edge / none, the median and
// the largest |shift|), then the node vectors go through the median test on the node grid, are expanded over the volume and start
// the pair's solve; the initial flow: line follows.  --block-match-only (one pair) stops after the table.
// --subset-match (resident driver, pairs in order) measures every pair a second time after its solve, independently of the flow (DESIGN.md
// 30): on a grid of nodes --subset-step apart (default 16), the displacement and, for --subset-model affine (the default; or
// translation), its gradient that carry the subset of radius --subset-window (default 8) of the first frame onto the second, by at
// most --subset-iterations (default 20) Gauss-Newton steps down to --subset-tolerance (default 1e-3), started from --subset-start
// flow (the default: the solved flow at the nodes), block-match (the table of --block-match) or zero.  <tag>_subset.csv has the node
// table; one line gives the nodes per status, the median ZNCC and the rms, median and p95 of |flow - subset| over the nodes that
// ended ok with a ZNCC of at least --subset-min-zncc (default 0.8).
// --warm-start starts pair k >= 1 from the flow of pair k-1 as it stands (steady motion); the pairs stay the consecutive ones.
// --total makes pair k frame 0 -> frame k+1, solved directly and started from the result of pair k-1: the other route to the
// displacement from frame 0, which --cumulative composes from the consecutive pairs with one interpolation per step.  The flow of a
// pair is then a displacement on frame 0's grid, so whatever needs --cumulative with more than two frames takes --total as well; the
// outputs carry the pair's tags.  With two frames both do nothing.  Not with each other, and --total not with --cumulative.
// With --levels N a started pyramid can be shallow: its depth has to cover the error of the guess, not the displacement.
// --strain LIST (resident driver, pairs in order; LIST a comma-separated subset of vol,e,eq) also differentiates every pair's flow --
// with --cumulative the displacement frame 0 -> frame k+1 instead -- on the device (f3d_flow_strain) and writes the selected fields
// as <tag>_strain-{vol | exx,eyy,ezz,exy,exz,eyz | eq}-W-H-D.raw with the flow's (or the displacement's) tag, and one line of
// statistics per pair.
// --window-strain LIST (same conditions and the same source as --strain, --use-validated included; LIST a comma-separated subset of
// vol,e,eq,grad) takes the gradient of that displacement as the slope of the least-squares plane through the (2R+1)^3 neighbourhood of
// every voxel on the device (f3d_window_strain; --window-radius R, 1 .. 3, default 2) and forms the strain fields of --strain from it.
// A voxel with fewer than --window-min-count present neighbours (default a quarter of the window, at least 4) is undefined.
// <tag>_wstrain-{vol | exx,eyy,ezz,exy,exz,eyz | eq | G00 .. G22}-W-H-D.raw, and one line of statistics per pair.
// --window-principal LIST and --window-rotation LIST (each on its own or with any of the others; the LISTs of --principal and
// --rotation) compute those two from the window's gradient instead of central differences (f3d_window_strain's gradient, then
// f3d_principal_from_gradient / f3d_polar_from_gradient), with the radius and minimum count of --window-radius / --window-min-count:
// <tag>_wprincipal-{e1,e2,e3 | gmax | d1x,.. | d3x,..}-W-H-D.raw and <tag>_wrotation-{theta | rx,ry,rz | l1,l2,l3}-W-H-D.raw, and one
// line of statistics each per pair.
// --principal LIST (same conditions and the same source as --strain, with which it may be combined; LIST a comma-separated subset of
// val,shear,dir1,dir3) diagonalises the Green-Lagrange tensor of that displacement on the device (f3d_principal_strain) and writes
// the selected fields as <tag>_principal-{e1,e2,e3 | gmax | d1x,d1y,d1z | d3x,d3y,d3z}-W-H-D.raw, and one line of statistics per
// pair.
// --rotation LIST (same conditions and the same source once more; LIST a comma-separated subset of angle,vector,stretch) takes the
// rotation R of F = R U out of the local deformation gradient of that displacement on the device (f3d_polar_decomposition) and
// writes the selected fields as <tag>_rotation-{theta | rx,ry,rz | l1,l2,l3}-W-H-D.raw (the angle in radians, the rotation vector
// angle * axis, the principal stretches), and one line of statistics per pair.
// --inverse (same conditions and the same source once more) inverts that displacement on the device (f3d_invert_displacement, 32
// steps, tolerance 1e-3): <tag>_inverse-{u,v,w,err}-W-H-D.raw is the displacement on the LATER frame's grid that leads back to the
// earlier one (NaN where the point comes from outside the volume) and the round-trip residual of it, and one line of statistics per
// pair.
// --match LIST (resident driver, pairs in order; LIST a comma-separated subset of warped,zncc,rmsd) says where the flow is to be
// believed: frame k+1 is carried onto frame k's grid through the PAIR's flow (f3d_carry_field; also under --cumulative, since frame 0
// is not kept) and compared with frame k over (2R+1)^3 windows on the device (f3d_local_correlation; --match-radius R, 1 .. 4,
// default 3).  <tag>_match-{warped,zncc,rmsd}-W-H-D.raw with the flow's tag, and one line of statistics per pair.
// --detrend MODEL (same conditions and the same source as --strain) fits a translation, a rigid motion or an affine map to that
// displacement on the device (f3d_motion_sums, f3d_motion_solve) and takes it out (f3d_remove_motion): the drift, settling and tilt
// of the sample between the scans.  <tag>_detrended-{u,v,w}-W-H-D.raw is what remains, and one line per pair gives the motion.
// --detrend-min-zncc T fits only where the zncc of --match (which must then select zncc) is at least T; not with --cumulative, whose
// displacement lives on frame 0's grid and the zncc on the pair's.
// --validate MODE (same conditions and the same source as --strain) runs the normalised median test on that displacement on the device
// (f3d_validate_displacement: every vector against the median of its up to 26 neighbours --validate-step voxels away, default 1, in
// units of their median residual plus --validate-eps, default 0.1) and sets what exceeds --validate-threshold (default 2; tested with
// at least --validate-min-neighbours neighbours, default 9) to NaN (mark) or to the neighbour median (replace).  --validate-min-zncc Z
// also rejects the voxels whose zncc of --match is below Z (conditions of --detrend-min-zncc); --validate-fill N runs up to N further
// passes that give undefined voxels the median of their defined neighbours.  <tag>_validated-{r,u,v,w}-W-H-D.raw and one line per pair.
// --use-validated makes --strain, --principal, --rotation and --detrend take the validated displacement in place of the raw one; the
// validated field is then computed before them, and after the match.
// --labels FILE --label-motion MODEL (same conditions and the same source as --detrend, --use-validated included) fits MODEL to the
// voxels of every body of a segmentation on the device (f3d_label_motion_sums, f3d_motion_solve_labels) and takes each body's fit out of
// its voxels (f3d_remove_label_motion).  FILE is raw little-endian int32 of W x H x D on frame 0's grid: 0 background, 1 .. max the
// bodies; it is uploaded once.  With more than two frames it needs --cumulative or --total: only the displacement from frame 0 lives on that grid.
// A body with fewer than --label-min-voxels voxels (default 27) is not fitted.  <tag>_labelres-{u,v,w}-W-H-D.raw is what remains (NaN
// where there is no fit), <tag>_labelmotion.csv has one row per label, and one line per pair sums it up.
// --labels FILE --contacts (same conditions and the same source as --label-motion, with or without it) finds the contacts between the
// bodies of the segmentation on the device (f3d_label_contacts) and their kinematics on the host (f3d_contact_kinematics):
// <tag>_contacts.csv has one row per pair of touching bodies -- lo, hi, status (the F3D_CONTACT_* bits), the faces per axis, the area,
// the normal from lo to hi, the mean face centre, the opening and the slip of the displacement across the contact, and the same two from
// the fits of --label-motion when that is given too (nan otherwise) -- and one line per pair sums it up.  A contact with fewer than
// --contact-min-faces faces (default 4) is marked small and left out of that line's opening, closing and slip.
// --segment LO:HI makes the labels on the device instead of reading them (f3d_label_components): the voxels of the raw frame 0 with
// LO <= value <= HI, in the units of the frame as it is read (either side may be left empty for an open bound), joined over their faces
// into bodies while the first pair is resident; a body of fewer than --segment-min-voxels voxels (default 27) gets no label.  It takes
// the place of --labels FILE for --label-motion and --contacts, and may stand alone.  <tag>_labels.raw (tag of the first pair) is the
// label volume in the format --labels reads, <tag>_bodies.csv has one row per body (label, voxels), and one line sums it up.
// --segment-split R (or --segment-split-d2 N, the exact form: N = ceil(R^2)) takes touching bodies apart (f3d_split_components): the
// cores are the foreground voxels at least R voxels deep below the surface, and every foreground voxel goes to the nearest core of its
// connected body.  Same files; the line that sums up gains what the split found.  Only with --segment.
// Either side of --segment LO:HI may be a token instead of a number: otsu is the cut of two classes, otsu1 and otsu2 the lower and the
// upper cut of three (f3d_histogram of frame 0 on the device, f3d_otsu and f3d_histogram_edge on the host).  On the LO side a token
// stands for the float32 edge e of the cut bin, so the foreground is s >= e; on the HI side for the largest float below e, so it is
// s < e: otsu1:otsu2 is exactly the middle phase, and :otsu and otsu: partition the voxels inside the range.  --segment-bins B (1 ..
// 4096, default 256) and --segment-range A:B (default: the finite minimum and maximum of frame 0) lay the bins; one line says what was
// chosen and the run goes on exactly as if the numbers had been given.  --histogram, alone or with --segment, writes
// <tag>_histogram.csv (bin, lower edge with %.9g, count) and prints one line.
// (--labels FILE | --segment ...) --label-shape writes the shape table of the bodies (f3d_label_shape_sums on the device,
// f3d_label_shape_solve on the host), once, right after the labels are on the device: <tag>_shapes.csv (tag of the first pair) has one
// row per label -- label, status, voxels, the bounding box, the voxels on the two box faces of each axis, centroid, diameter of the ball
// of the same volume, the three semi-axes and their directions, staircase faces, the Cauchy-Crofton surface, sphericity and the Euler
// number -- and one line sums it up.  It needs no displacement; every other output is the same with and without it.
// (--labels FILE | --segment ...) --label-stats LIST [--label-stats-bins B] [--label-stats-paint] gives the statistics of fields per
// body (f3d_label_field_sums on the device, f3d_label_field_solve on the host).  LIST is a comma-separated subset of grey (the raw
// frame 0 of the first pair; done once, when the labels and that frame are on the device), vol, eq (--strain must select the name), gmax
// (--principal shear), angle (--rotation angle), zncc, rmsd (--match), wvol, weq (--window-strain); a field of a pair is read in its
// container right after it was computed, under the conditions and from the source of --label-motion.  The shift of the quantisation and,
// with B bins (0 .. 256, default 64), their range are taken from the field's finite range under the labels.  <tag>_labelstats.csv has
// one row per (field, label): field, label, status, n, min, max, mean, std, q05, median, q95, below, above; one line is printed per
// field and pair; with --label-stats-paint <tag>_labelmean-<name>-W-H-D.raw is the mean of each ok label painted into its voxels
// (f3d_paint_labels), NaN elsewhere.  Every other output is the same with and without it.
// --segment ... --track [--track-min-fraction F] follows the bodies from frame to frame.  While pair k is resident the RAW frame k+1 is
// segmented into a second label volume with what --segment settled for frame 0 -- the thresholds as numbers, --segment-min-voxels and the
// split; an Otsu cut is the number it came to on frame 0 and is not taken again per frame.  The overlap of frame 0's bodies with these
// through the pair's flow or, with --cumulative, the displacement from frame 0 (the validated one under --use-validated) is counted on
// the device (f3d_label_overlap), solved on the host (f3d_overlap_solve: a share of at least F, default 0.1, counts) and the later
// frame's bodies are renumbered on the device (f3d_relabel_labels).  <tag>_tracks.csv has a row per body of frame 0 (side a) and then
// per body of frame k+1 (side b); <tag>_tracked-labels.raw is frame k+1's bodies under frame 0's numbers, new bodies after them; one
// line sums it up.  With more than two frames it needs --cumulative; every other output is the same with and without it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "f3d_host.h"
#include "hip_utils.h"
#include "optical_flow.h"
#include "optical_flow_p.h"
#include "synth.h"

static void Usage()
{
  std::printf("usage: flow3d --dims W H D (--frames f0.raw f1.raw [f2.raw ...] [--f32] | --synthetic) [--out prefix]\n"
              "              [--levels N] [--scale s] [--outer N] [--inner N] [--alpha a] [--eps-smooth e]\n"
              "              [--eps-data e] [--median r] [--sigma s] [--vtk] [--stats] [--silent] [--partial [--full] [--budget-mb N]]\n"
              "              [--concurrent N] [--cumulative] [--initial-flow U V W] [--warm-start | --total]\n"
              "              [--block-match [--block-match-step S] [--block-match-window W] [--block-match-search R | RX:RY:RZ]\n"
              "               [--block-match-min-zncc T] [--block-match-only]]\n"
              "              [--subset-match [--subset-step S] [--subset-window W] [--subset-model translation|affine]\n"
              "               [--subset-iterations N] [--subset-tolerance T] [--subset-min-zncc Z] [--subset-start flow|block-match|zero]]\n"
              "              [--strain vol,e,eq] [--principal val,shear,dir1,dir3]\n"
              "              [--rotation angle,vector,stretch] [--inverse] [--match warped,zncc,rmsd [--match-radius R]]\n"
              "              [--window-strain vol,e,eq,grad [--window-radius R] [--window-min-count K]]\n"
              "              [--window-principal val,shear,dir1,dir3] [--window-rotation angle,vector,stretch]\n"
              "              [--detrend translation|rigid|affine [--detrend-min-zncc T]]\n"
              "              [--validate mark|replace [--validate-step S] [--validate-threshold T] [--validate-eps E]\n"
              "               [--validate-min-neighbours K] [--validate-fill N] [--validate-min-zncc Z] [--use-validated]]\n"
              "              [--labels FILE --label-motion translation|rigid|affine [--label-min-voxels K]]\n"
              "              [--labels FILE --contacts [--contact-min-faces K]]\n"
              "              [(--labels FILE | --segment ...) --label-shape]\n"
              "              [(--labels FILE | --segment ...) --label-stats grey,vol,eq,gmax,angle,zncc,rmsd,wvol,weq\n"
              "               [--label-stats-bins B] [--label-stats-paint]]  (a name needs the option that computes it: --strain vol / eq,\n"
              "               --principal shear, --rotation angle, --match zncc / rmsd, --window-strain vol / eq)\n"
              "              [--segment LO:HI [--segment-min-voxels K]]\n"
              "              [--segment-split R | --segment-split-d2 N]\n"
              "              [--segment with otsu, or otsu1 / otsu2, in place of LO or HI] [--segment-bins B] [--segment-range A:B]\n"
              "              [--histogram]\n"
              "              [--segment ... --track [--track-min-fraction F]]  (frame k+1 is cut at the numbers --segment settled\n"
              "               for frame 0; an Otsu cut is not taken again per frame)\n");
}

int main(int argc, char** argv)
{
  size_t width = 0, height = 0, depth = 0;
  std::vector<std::string> files;
  std::string prefix = "flow3d";
  bool f32_input = false, synthetic = false, write_vtk = false, silent_mode = false, print_stats = false;
  bool use_partial_gpu = false, partial_full = false, cumulative = false;
  bool total = false, warm_start = false, initial_given = false;  // --total, --warm-start, --initial-flow U V W
  std::vector<std::string> initial_files;
  bool block_match = false, block_match_only = false, block_match_sub_given = false;  // --block-match and its options
  OpticalFlowE::BlockMatchParams block_match_params;
  bool subset_match = false, subset_sub_given = false;  // --subset-match and its options
  OpticalFlowE::SubsetMatchParams subset_params;
  subset_params.start = OpticalFlowE::kSubsetFlow;
  size_t concurrent = 1;
  unsigned strain_fields = 0;     // --strain: F3D_STRAIN_* groups
  unsigned wstrain_fields = 0;    // --window-strain: F3D_STRAIN_* groups and F3D_WSTRAIN_G
  unsigned window_radius = 2;     // --window-radius
  unsigned window_min_count = 0;  // --window-min-count; 0: a quarter of the window, at least 4
  bool window_sub_given = false;
  unsigned principal_fields = 0;  // --principal: F3D_PRINCIPAL_* groups
  unsigned wprincipal_fields = 0; // --window-principal: F3D_PRINCIPAL_* groups
  unsigned wpolar_fields = 0;     // --window-rotation: F3D_POLAR_* groups
  unsigned polar_fields = 0;      // --rotation: F3D_POLAR_* groups
  bool inverse = false;           // --inverse
  unsigned match_fields = 0;      // --match: OpticalFlowE::kMatch* bits
  unsigned match_radius = 3;      // --match-radius
  bool match_radius_given = false;
  const float match_threshold = 0.8f;
  int detrend_model = -1;         // --detrend: F3D_MOTION_*
  float detrend_min_zncc = std::nanf("");  // --detrend-min-zncc; NaN: no mask
  bool detrend_min_given = false;
  unsigned validate_mode = 0;     // --validate: F3D_VALIDATE_MARK / F3D_VALIDATE_REPLACE
  unsigned validate_step = 1, validate_min_neighbours = 9, validate_fill = 0;
  float validate_threshold = 2.0f, validate_eps = 0.1f;
  float validate_min_zncc = std::nanf("");  // --validate-min-zncc; NaN: no mask
  bool validate_min_given = false, validate_sub_given = false, use_validated = false;
  std::string labels_file;        // --labels
  int label_model = -1;           // --label-motion: F3D_MOTION_*
  unsigned long long label_min_voxels = 27;
  bool label_min_given = false;
  bool contacts = false;          // --contacts
  bool label_shape = false;       // --label-shape
  std::vector<std::string> label_stats;  // --label-stats: the names in the order given
  size_t label_stats_bins = 64;   // --label-stats-bins
  bool label_stats_bins_given = false, label_stats_paint = false;
  unsigned long long contact_min_faces = 4;
  bool contact_min_given = false;
  bool segment = false;           // --segment LO:HI
  float segment_lo = -INFINITY, segment_hi = INFINITY;
  unsigned long long segment_min_voxels = 27;
  bool segment_min_given = false;
  int segment_token[2] = {0, 0};   // what stands for LO and for HI: 0 a number, 1 otsu, 2 otsu1, 3 otsu2
  size_t segment_bins = 256;       // --segment-bins B
  bool segment_bins_given = false;
  float segment_range[2] = {0.f, 0.f};  // --segment-range A:B
  bool segment_range_given = false;
  bool histogram = false;          // --histogram
  bool track = false;              // --track
  double track_min_fraction = 0.1; // --track-min-fraction F
  bool track_min_given = false;
  int segment_split_given = 0;            // --segment-split R and --segment-split-d2 N, counted
  unsigned long long segment_core_d2 = 0;  // 0: no split
  const unsigned inverse_iterations = 32;
  const float inverse_tolerance = 1e-3f;

  // defaults of src/main.cpp:77-85
  size_t warp_levels_count = 40;
  float warp_scale_factor = 0.95f;
  size_t outer_iterations_count = 40;
  size_t inner_iterations_count = 5;
  float equation_alpha = 7.5f;
  float equation_smoothness = 0.001f;
  float equation_data = 0.001f;
  size_t median_radius = 5;
  float gaussian_sigma = 2.0f;

  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto need = [&](int n) {
      if (i + n >= argc) {
        Usage();
        std::exit(64);
      }
    };
    if (a == "--dims") { need(3); width = std::strtoull(argv[++i], nullptr, 10); height = std::strtoull(argv[++i], nullptr, 10); depth = std::strtoull(argv[++i], nullptr, 10); }
    else if (a == "--frames") {
      need(2);
      while (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) files.push_back(argv[++i]);
    }
    else if (a == "--stats") print_stats = true;
    else if (a == "--out") { need(1); prefix = argv[++i]; }
    else if (a == "--levels") { need(1); warp_levels_count = std::strtoull(argv[++i], nullptr, 10); }
    else if (a == "--scale") { need(1); warp_scale_factor = std::strtof(argv[++i], nullptr); }
    else if (a == "--outer") { need(1); outer_iterations_count = std::strtoull(argv[++i], nullptr, 10); }
    else if (a == "--inner") { need(1); inner_iterations_count = std::strtoull(argv[++i], nullptr, 10); }
    else if (a == "--alpha") { need(1); equation_alpha = std::strtof(argv[++i], nullptr); }
    else if (a == "--eps-smooth") { need(1); equation_smoothness = std::strtof(argv[++i], nullptr); }
    else if (a == "--eps-data") { need(1); equation_data = std::strtof(argv[++i], nullptr); }
    else if (a == "--median") { need(1); median_radius = std::strtoull(argv[++i], nullptr, 10); }
    else if (a == "--sigma") { need(1); gaussian_sigma = std::strtof(argv[++i], nullptr); }
    else if (a == "--f32") f32_input = true;
    else if (a == "--synthetic") synthetic = true;
    else if (a == "--vtk") write_vtk = true;
    else if (a == "--silent") silent_mode = true;
    else if (a == "--partial") use_partial_gpu = true;
    else if (a == "--full") partial_full = true;
    else if (a == "--budget-mb") { need(1); setenv("F3D_P_BUDGET_MB", argv[++i], 1); }
    else if (a == "--concurrent") { need(1); concurrent = std::strtoull(argv[++i], nullptr, 10); }
    else if (a == "--cumulative") cumulative = true;
    else if (a == "--total") total = true;
    else if (a == "--warm-start") warm_start = true;
    else if (a == "--initial-flow") {
      initial_given = true;
      while (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) initial_files.push_back(argv[++i]);
    }
    else if (a == "--block-match") block_match = true;
    else if (a == "--block-match-only") block_match_only = block_match_sub_given = true;
    else if (a == "--block-match-step" || a == "--block-match-window") {
      need(1);
      char* rest = nullptr;
      const long n = std::strtol(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || n < 1 || n > (a == "--block-match-step" ? 1 << 20 : F3D_BLOCK_MATCH_MAX_WINDOW)) { Usage(); return 64; }
      (a == "--block-match-step" ? block_match_params.step : block_match_params.window) = static_cast<int>(n);
      block_match_sub_given = true;
    }
    else if (a == "--block-match-search") {
      need(1);
      // R or RX:RY:RZ
      const std::string list = argv[++i];
      int count = 0;
      size_t at = 0;
      while (count < 3) {
        const size_t end = list.find(':', at);
        const std::string item = list.substr(at, end == std::string::npos ? std::string::npos : end - at);
        char* rest = nullptr;
        const long n = std::strtol(item.c_str(), &rest, 10);
        if (item.empty() || *rest || n < 0 || n > F3D_BLOCK_MATCH_MAX_REACH) { Usage(); return 64; }
        block_match_params.radius[count++] = static_cast<int>(n);
        if (end == std::string::npos) break;
        at = end + 1;
        if (count == 3) { Usage(); return 64; }
      }
      if (count == 1) block_match_params.radius[1] = block_match_params.radius[2] = block_match_params.radius[0];
      else if (count != 3) { Usage(); return 64; }
      block_match_sub_given = true;
    }
    else if (a == "--block-match-min-zncc") {
      need(1);
      char* rest = nullptr;
      block_match_params.min_zncc = std::strtod(argv[++i], &rest);
      if (rest == argv[i] || *rest || std::isnan(block_match_params.min_zncc)) { Usage(); return 64; }
      block_match_sub_given = true;
    }
    else if (a == "--subset-match") subset_match = true;
    else if (a == "--subset-step" || a == "--subset-window" || a == "--subset-iterations") {
      need(1);
      char* rest = nullptr;
      const long n = std::strtol(argv[++i], &rest, 10);
      const long most = a == "--subset-step" ? 1 << 20 : (a == "--subset-window" ? F3D_SUBSET_MATCH_MAX_WINDOW : F3D_SUBSET_MATCH_MAX_ITERATIONS);
      if (rest == argv[i] || *rest || n < 1 || n > most) { Usage(); return 64; }
      (a == "--subset-step" ? subset_params.step : (a == "--subset-window" ? subset_params.window : subset_params.max_iterations)) =
          static_cast<int>(n);
      subset_sub_given = true;
    }
    else if (a == "--subset-tolerance" || a == "--subset-min-zncc") {
      need(1);
      char* rest = nullptr;
      const double v = std::strtod(argv[++i], &rest);
      if (rest == argv[i] || *rest || std::isnan(v) || (a == "--subset-tolerance" && !(v > 0.0))) { Usage(); return 64; }
      (a == "--subset-tolerance" ? subset_params.tolerance : subset_params.min_zncc) = v;
      subset_sub_given = true;
    }
    else if (a == "--subset-model") {
      need(1);
      const std::string v = argv[++i];
      if (v == "translation") subset_params.model = F3D_SUBSET_TRANSLATION;
      else if (v == "affine") subset_params.model = F3D_SUBSET_AFFINE;
      else { Usage(); return 64; }
      subset_sub_given = true;
    }
    else if (a == "--subset-start") {
      need(1);
      const std::string v = argv[++i];
      if (v == "flow") subset_params.start = OpticalFlowE::kSubsetFlow;
      else if (v == "block-match") subset_params.start = OpticalFlowE::kSubsetNodes;
      else if (v == "zero") subset_params.start = OpticalFlowE::kSubsetZero;
      else { Usage(); return 64; }
      subset_sub_given = true;
    }
    else if (a == "--inverse") inverse = true;
    else if (a == "--strain") {
      need(1);
      const std::string list = argv[++i];
      size_t at = 0;
      while (true) {
        const size_t end = list.find(',', at);
        const std::string item = list.substr(at, end == std::string::npos ? std::string::npos : end - at);
        if (item == "vol") strain_fields |= F3D_STRAIN_VOL;
        else if (item == "e") strain_fields |= F3D_STRAIN_E;
        else if (item == "eq") strain_fields |= F3D_STRAIN_EQ;
        else { Usage(); return 64; }
        if (end == std::string::npos) break;
        at = end + 1;
      }
    }
    else if (a == "--window-strain") {
      need(1);
      const std::string list = argv[++i];
      size_t at = 0;
      while (true) {
        const size_t end = list.find(',', at);
        const std::string item = list.substr(at, end == std::string::npos ? std::string::npos : end - at);
        if (item == "vol") wstrain_fields |= F3D_STRAIN_VOL;
        else if (item == "e") wstrain_fields |= F3D_STRAIN_E;
        else if (item == "eq") wstrain_fields |= F3D_STRAIN_EQ;
        else if (item == "grad") wstrain_fields |= F3D_WSTRAIN_G;
        else { Usage(); return 64; }
        if (end == std::string::npos) break;
        at = end + 1;
      }
    }
    else if (a == "--window-radius" || a == "--window-min-count") {
      need(1);
      char* rest = nullptr;
      const unsigned long n = std::strtoul(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || argv[i][0] == '-') { Usage(); return 64; }
      if (a == "--window-radius") {
        if (n < 1 || n > 3) { Usage(); return 64; }
        window_radius = static_cast<unsigned>(n);
      } else {
        if (n < 1 || n > 343) { Usage(); return 64; }
        window_min_count = static_cast<unsigned>(n);
      }
      window_sub_given = true;
    }
    else if (a == "--window-principal") {
      need(1);
      const std::string list = argv[++i];
      size_t at = 0;
      while (true) {
        const size_t end = list.find(',', at);
        const std::string item = list.substr(at, end == std::string::npos ? std::string::npos : end - at);
        if (item == "val") wprincipal_fields |= F3D_PRINCIPAL_VALUES;
        else if (item == "shear") wprincipal_fields |= F3D_PRINCIPAL_SHEAR;
        else if (item == "dir1") wprincipal_fields |= F3D_PRINCIPAL_DIR1;
        else if (item == "dir3") wprincipal_fields |= F3D_PRINCIPAL_DIR3;
        else { Usage(); return 64; }
        if (end == std::string::npos) break;
        at = end + 1;
      }
    }
    else if (a == "--window-rotation") {
      need(1);
      const std::string list = argv[++i];
      size_t at = 0;
      while (true) {
        const size_t end = list.find(',', at);
        const std::string item = list.substr(at, end == std::string::npos ? std::string::npos : end - at);
        if (item == "angle") wpolar_fields |= F3D_POLAR_ANGLE;
        else if (item == "vector") wpolar_fields |= F3D_POLAR_VECTOR;
        else if (item == "stretch") wpolar_fields |= F3D_POLAR_STRETCH;
        else { Usage(); return 64; }
        if (end == std::string::npos) break;
        at = end + 1;
      }
    }
    else if (a == "--principal") {
      need(1);
      const std::string list = argv[++i];
      size_t at = 0;
      while (true) {
        const size_t end = list.find(',', at);
        const std::string item = list.substr(at, end == std::string::npos ? std::string::npos : end - at);
        if (item == "val") principal_fields |= F3D_PRINCIPAL_VALUES;
        else if (item == "shear") principal_fields |= F3D_PRINCIPAL_SHEAR;
        else if (item == "dir1") principal_fields |= F3D_PRINCIPAL_DIR1;
        else if (item == "dir3") principal_fields |= F3D_PRINCIPAL_DIR3;
        else { Usage(); return 64; }
        if (end == std::string::npos) break;
        at = end + 1;
      }
    }
    else if (a == "--rotation") {
      need(1);
      const std::string list = argv[++i];
      size_t at = 0;
      while (true) {
        const size_t end = list.find(',', at);
        const std::string item = list.substr(at, end == std::string::npos ? std::string::npos : end - at);
        if (item == "angle") polar_fields |= F3D_POLAR_ANGLE;
        else if (item == "vector") polar_fields |= F3D_POLAR_VECTOR;
        else if (item == "stretch") polar_fields |= F3D_POLAR_STRETCH;
        else { Usage(); return 64; }
        if (end == std::string::npos) break;
        at = end + 1;
      }
    }
    else if (a == "--match") {
      need(1);
      const std::string list = argv[++i];
      size_t at = 0;
      while (true) {
        const size_t end = list.find(',', at);
        const std::string item = list.substr(at, end == std::string::npos ? std::string::npos : end - at);
        if (item == "warped") match_fields |= OpticalFlowE::kMatchWarped;
        else if (item == "zncc") match_fields |= OpticalFlowE::kMatchZncc;
        else if (item == "rmsd") match_fields |= OpticalFlowE::kMatchRmsd;
        else { Usage(); return 64; }
        if (end == std::string::npos) break;
        at = end + 1;
      }
    }
    else if (a == "--match-radius") {
      need(1);
      char* rest = nullptr;
      const unsigned long r = std::strtoul(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || r < 1 || r > 4) { Usage(); return 64; }
      match_radius = static_cast<unsigned>(r);
      match_radius_given = true;
    }
    else if (a == "--detrend") {
      need(1);
      const std::string model = argv[++i];
      if (model == "translation") detrend_model = F3D_MOTION_TRANSLATION;
      else if (model == "rigid") detrend_model = F3D_MOTION_RIGID;
      else if (model == "affine") detrend_model = F3D_MOTION_AFFINE;
      else { Usage(); return 64; }
    }
    else if (a == "--detrend-min-zncc") {
      need(1);
      char* rest = nullptr;
      detrend_min_zncc = std::strtof(argv[++i], &rest);
      if (rest == argv[i] || *rest || std::isnan(detrend_min_zncc)) { Usage(); return 64; }
      detrend_min_given = true;
    }
    else if (a == "--validate") {
      need(1);
      const std::string mode = argv[++i];
      if (mode == "mark") validate_mode = F3D_VALIDATE_MARK;
      else if (mode == "replace") validate_mode = F3D_VALIDATE_REPLACE;
      else { Usage(); return 64; }
    }
    else if (a == "--validate-step" || a == "--validate-min-neighbours" || a == "--validate-fill") {
      need(1);
      char* rest = nullptr;
      const unsigned long n = std::strtoul(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || argv[i][0] == '-') { Usage(); return 64; }
      if (a == "--validate-step") {
        if (n < 1 || n > 16) { Usage(); return 64; }
        validate_step = static_cast<unsigned>(n);
      } else if (a == "--validate-min-neighbours") {
        if (n < 1 || n > 26) { Usage(); return 64; }
        validate_min_neighbours = static_cast<unsigned>(n);
      } else {
        if (n > 1000) { Usage(); return 64; }
        validate_fill = static_cast<unsigned>(n);
      }
      validate_sub_given = true;
    }
    else if (a == "--validate-threshold" || a == "--validate-eps" || a == "--validate-min-zncc") {
      need(1);
      char* rest = nullptr;
      const float x = std::strtof(argv[++i], &rest);
      if (rest == argv[i] || *rest || std::isnan(x)) { Usage(); return 64; }
      if (a == "--validate-threshold") {
        if (x < 0.f) { Usage(); return 64; }
        validate_threshold = x;
      } else if (a == "--validate-eps") {
        if (!(x > 0.f) || std::isinf(x)) { Usage(); return 64; }
        validate_eps = x;
      } else {
        validate_min_zncc = x;
        validate_min_given = true;
      }
      validate_sub_given = true;
    }
    else if (a == "--use-validated") use_validated = true;
    else if (a == "--labels") {
      need(1);
      labels_file = argv[++i];
      if (labels_file.empty()) { Usage(); return 64; }
    }
    else if (a == "--label-motion") {
      need(1);
      const std::string model = argv[++i];
      if (model == "translation") label_model = F3D_MOTION_TRANSLATION;
      else if (model == "rigid") label_model = F3D_MOTION_RIGID;
      else if (model == "affine") label_model = F3D_MOTION_AFFINE;
      else { Usage(); return 64; }
    }
    else if (a == "--label-min-voxels") {
      need(1);
      char* rest = nullptr;
      label_min_voxels = std::strtoull(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || argv[i][0] == '-') { Usage(); return 64; }
      label_min_given = true;
    }
    else if (a == "--contacts") contacts = true;
    else if (a == "--label-shape") label_shape = true;
    else if (a == "--label-stats") {
      need(1);
      std::string list = argv[++i];
      size_t pos = 0;
      while (pos <= list.size()) {
        const size_t comma = std::min(list.find(',', pos), list.size());
        const std::string item = list.substr(pos, comma - pos);
        static const char* const known[9] = {"grey", "vol", "eq", "gmax", "angle", "zncc", "rmsd", "wvol", "weq"};
        const bool is_known = std::find_if(known, known + 9, [&](const char* n) { return item == n; }) != known + 9;
        if (!is_known || std::find(label_stats.begin(), label_stats.end(), item) != label_stats.end()) {
          std::printf("--label-stats %s: '%s' is not one of grey, vol, eq, gmax, angle, zncc, rmsd, wvol, weq, or is given twice\n",
                      list.c_str(), item.c_str());
          Usage();
          return 64;
        }
        label_stats.push_back(item);
        pos = comma + 1;
      }
    }
    else if (a == "--label-stats-bins") {
      need(1);
      char* rest = nullptr;
      const unsigned long long b = std::strtoull(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || argv[i][0] == '-' || b > 256) {
        std::printf("--label-stats-bins %s: B must be 0 .. 256\n", argv[i]);
        Usage();
        return 64;
      }
      label_stats_bins = static_cast<size_t>(b);
      label_stats_bins_given = true;
    }
    else if (a == "--label-stats-paint") label_stats_paint = true;
    else if (a == "--track") track = true;
    else if (a == "--track-min-fraction") {
      need(1);
      char* rest = nullptr;
      track_min_fraction = std::strtod(argv[++i], &rest);
      if (rest == argv[i] || *rest || !(track_min_fraction > 0.0 && track_min_fraction <= 1.0)) {
        std::printf("--track-min-fraction %s: F must be in (0, 1]\n", argv[i]);
        Usage();
        return 64;
      }
      track_min_given = true;
    }
    else if (a == "--segment") {
      need(1);
      // LO:HI, either side empty for an open bound; anything else, a NaN or LO > HI is malformed
      const std::string range = argv[++i];
      const size_t colon = range.find(':');
      if (colon == std::string::npos || range.find(':', colon + 1) != std::string::npos) { Usage(); return 64; }
      const std::string side[2] = {range.substr(0, colon), range.substr(colon + 1)};
      float bound[2] = {-INFINITY, INFINITY};
      for (int k = 0; k < 2; ++k) {
        segment_token[k] = 0;
        if (side[k].empty()) continue;
        // a token stands for a cut of frame 0's histogram; the bound stays open until the frame is there
        if (side[k] == "otsu" || side[k] == "otsu1" || side[k] == "otsu2") {
          segment_token[k] = side[k] == "otsu" ? 1 : side[k] == "otsu1" ? 2 : 3;
          continue;
        }
        char* rest = nullptr;
        bound[k] = std::strtof(side[k].c_str(), &rest);
        if (rest == side[k].c_str() || *rest || bound[k] != bound[k]) { Usage(); return 64; }
      }
      if (segment_token[0] && segment_token[1]) {
        if ((segment_token[0] == 1) != (segment_token[1] == 1)) {
          std::printf("--segment %s: otsu is the cut of two classes, otsu1 and otsu2 are the cuts of three: they cannot be mixed\n", range.c_str());
          Usage();
          return 64;
        }
        if (segment_token[0] >= segment_token[1]) {  // HI stands for the largest value below its cut
          std::printf("--segment %s: LO is above HI\n", range.c_str());
          Usage();
          return 64;
        }
      }
      if (bound[0] > bound[1]) {
        std::printf("--segment %s: LO is above HI\n", range.c_str());
        Usage();
        return 64;
      }
      segment = true;
      segment_lo = bound[0];
      segment_hi = bound[1];
    }
    else if (a == "--segment-bins") {
      need(1);
      char* rest = nullptr;
      const unsigned long long b = std::strtoull(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || argv[i][0] == '-' || b < 1 || b > 4096) { Usage(); return 64; }
      segment_bins = static_cast<size_t>(b);
      segment_bins_given = true;
    }
    else if (a == "--segment-range") {
      need(1);
      // A:B, both finite numbers with A < B
      const std::string range = argv[++i];
      const size_t colon = range.find(':');
      if (colon == std::string::npos || range.find(':', colon + 1) != std::string::npos) { Usage(); return 64; }
      const std::string side[2] = {range.substr(0, colon), range.substr(colon + 1)};
      for (int k = 0; k < 2; ++k) {
        char* rest = nullptr;
        segment_range[k] = std::strtof(side[k].c_str(), &rest);
        if (side[k].empty() || rest == side[k].c_str() || *rest || !std::isfinite(segment_range[k])) { Usage(); return 64; }
      }
      if (!(segment_range[0] < segment_range[1])) {
        std::printf("--segment-range %s: A must be below B\n", range.c_str());
        Usage();
        return 64;
      }
      segment_range_given = true;
    }
    else if (a == "--histogram") histogram = true;
    else if (a == "--segment-min-voxels") {
      need(1);
      char* rest = nullptr;
      segment_min_voxels = std::strtoull(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || argv[i][0] == '-' || segment_min_voxels == 0) { Usage(); return 64; }
      segment_min_given = true;
    }
    else if (a == "--segment-split") {
      need(1);
      char* rest = nullptr;
      const double radius = std::strtod(argv[++i], &rest);
      if (rest == argv[i] || *rest || !std::isfinite(radius) || !(radius > 0) || radius > 65536.0) { Usage(); return 64; }
      segment_core_d2 = static_cast<unsigned long long>(std::ceil(radius * radius));
      ++segment_split_given;
    }
    else if (a == "--segment-split-d2") {
      need(1);
      char* rest = nullptr;
      segment_core_d2 = std::strtoull(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || argv[i][0] == '-' || segment_core_d2 == 0) { Usage(); return 64; }
      ++segment_split_given;
    }
    else if (a == "--contact-min-faces") {
      need(1);
      char* rest = nullptr;
      contact_min_faces = std::strtoull(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest || argv[i][0] == '-') { Usage(); return 64; }
      contact_min_given = true;
    }
    else { Usage(); return 64; }
  }
  if (width == 0 || height == 0 || depth == 0 || (!synthetic && files.size() < 2)) {
    Usage();
    return 64;
  }
  if (cumulative && (use_partial_gpu || concurrent > 1)) {
    std::printf("--cumulative needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    return 64;
  }
  // the solves that start from a displacement: all refusals before any device is touched
  if (total && (cumulative || warm_start)) {
    std::printf(cumulative ? "--total solves frame 0 -> frame k+1 directly and --cumulative composes it from the pairs: choose one\n"
                           : "--total starts every pair from the one before already; --warm-start belongs to consecutive pairs\n");
    Usage();
    return 64;
  }
  if ((total || warm_start || initial_given) && (use_partial_gpu || concurrent > 1)) {
    std::printf("%s needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                total ? "--total" : (warm_start ? "--warm-start" : "--initial-flow"), use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (initial_given) {
    if (initial_files.size() != 3) {
      std::printf("--initial-flow takes three files, the u, v and w of the displacement pair 0 starts from\n");
      Usage();
      return 64;
    }
    for (const std::string& path : initial_files) {
      std::FILE* f = std::fopen(path.c_str(), "rb");
      const bool good = f && std::fseek(f, 0, SEEK_END) == 0 && static_cast<size_t>(std::ftell(f)) == width * height * depth * sizeof(float);
      if (f) std::fclose(f);
      if (!good) {
        std::printf("--initial-flow %s: not a file of %zu x %zu x %zu float32 values (%zu bytes)\n", path.c_str(), width, height, depth,
                    width * height * depth * sizeof(float));
        Usage();
        return 64;
      }
    }
  }
  // --block-match: the guess comes from the frames themselves; all refusals before any device is touched
  if (block_match_sub_given && !block_match) {
    std::printf("--block-match-step, -window, -search, -min-zncc and -only need --block-match\n");
    Usage();
    return 64;
  }
  if (block_match) {
    const size_t pairs_given = synthetic ? 1 : (files.empty() ? 0 : files.size() - 1);
    const char* why = nullptr;
    if (initial_given) why = "--block-match makes the guess --initial-flow would read: choose one";
    else if (use_partial_gpu || concurrent > 1) why = "--block-match needs the resident driver solving the pairs in order: it cannot be combined with --partial or --concurrent N > 1";
    else if ((total || warm_start) && pairs_given > 1) why = "--block-match on the pairs after the first is not available under --warm-start or --total, which start them from the pair before";
    else if (block_match_only && pairs_given > 1) why = "--block-match-only takes one pair";
    std::string layout_error;
    f3d_block_match_grid laid;
    if (!why && f3d_block_match_layout(width, height, depth, block_match_params.step, block_match_params.window, block_match_params.radius[0],
                                       block_match_params.radius[1], block_match_params.radius[2], &laid)) {
      layout_error = std::string("--block-match: ") + f3d_host_last_error();
      why = layout_error.c_str();
    }
    if (why) {
      std::printf("%s\n", why);
      Usage();
      return 64;
    }
  }
  // --subset-match: all refusals before any device is touched
  if (subset_sub_given && !subset_match) {
    std::printf("--subset-step, -window, -model, -iterations, -tolerance, -min-zncc and -start need --subset-match\n");
    Usage();
    return 64;
  }
  if (subset_match) {
    const char* why = nullptr;
    if (use_partial_gpu || concurrent > 1) why = "--subset-match needs the resident driver: it cannot be combined with --partial or --concurrent N > 1";
    else if (subset_params.start == OpticalFlowE::kSubsetNodes && (!block_match || block_match_only))
      why = "--subset-start block-match needs --block-match (without --block-match-only)";
    else if (block_match_only) why = "--subset-match runs after the pair's solve, which --block-match-only leaves out";
    std::string layout_error;
    f3d_subset_match_grid laid;
    if (!why && f3d_subset_match_layout(width, height, depth, subset_params.step, subset_params.window, &laid)) {
      layout_error = std::string("--subset-match: ") + f3d_host_last_error();
      why = layout_error.c_str();
    }
    if (why) {
      std::printf("%s\n", why);
      Usage();
      return 64;
    }
  }
  const bool from_frame_0 = cumulative || total;  // the displacement the derived fields are computed of starts at frame 0
  if (strain_fields && (use_partial_gpu || concurrent > 1)) {
    std::printf("--strain needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    return 64;
  }
  if (window_sub_given && !wstrain_fields && !wprincipal_fields && !wpolar_fields) {
    std::printf("--window-radius and --window-min-count need --window-strain, --window-principal or --window-rotation\n");
    Usage();
    return 64;
  }
  if ((wprincipal_fields || wpolar_fields) && (use_partial_gpu || concurrent > 1)) {
    std::printf("%s needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                wprincipal_fields ? "--window-principal" : "--window-rotation", use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (wstrain_fields && (use_partial_gpu || concurrent > 1)) {
    std::printf("--window-strain needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  {
    const unsigned window = (2 * window_radius + 1) * (2 * window_radius + 1) * (2 * window_radius + 1);
    if (window_min_count > window) {
      std::printf("--window-min-count must be 1 .. %u at --window-radius %u\n", window, window_radius);
      Usage();
      return 64;
    }
    if (!window_min_count) window_min_count = std::max(4u, window / 4);
  }
  if (principal_fields && (use_partial_gpu || concurrent > 1)) {
    std::printf("--principal needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (polar_fields && (use_partial_gpu || concurrent > 1)) {
    std::printf("--rotation needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (inverse && (use_partial_gpu || concurrent > 1)) {
    std::printf("--inverse needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (match_radius_given && !match_fields) {
    std::printf("--match-radius needs --match\n");
    Usage();
    return 64;
  }
  if (match_fields && (use_partial_gpu || concurrent > 1)) {
    std::printf("--match needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (detrend_min_given && detrend_model < 0) {
    std::printf("--detrend-min-zncc needs --detrend\n");
    Usage();
    return 64;
  }
  if (detrend_model >= 0 && (use_partial_gpu || concurrent > 1)) {
    std::printf("--detrend needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (detrend_min_given && (cumulative || !(match_fields & OpticalFlowE::kMatchZncc))) {
    std::printf(cumulative ? "--detrend-min-zncc cannot be combined with --cumulative: the zncc of --match lives on the pair's grid\n"
                           : "--detrend-min-zncc needs --match with zncc in its list\n");
    Usage();
    return 64;
  }
  if ((validate_sub_given || use_validated) && !validate_mode) {
    std::printf(use_validated ? "--use-validated needs --validate\n" : "--validate-step, -threshold, -eps, -min-neighbours, -fill and "
                                                                       "-min-zncc need --validate\n");
    Usage();
    return 64;
  }
  if (validate_mode && (use_partial_gpu || concurrent > 1)) {
    std::printf("--validate needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (validate_min_given && (cumulative || !(match_fields & OpticalFlowE::kMatchZncc))) {
    std::printf(cumulative ? "--validate-min-zncc cannot be combined with --cumulative: the zncc of --match lives on the pair's grid\n"
                           : "--validate-min-zncc needs --match with zncc in its list\n");
    Usage();
    return 64;
  }
  if ((segment && !labels_file.empty()) || (segment_min_given && !segment)) {
    std::printf("--segment takes the place of --labels FILE: they cannot be combined, and --segment-min-voxels needs --segment\n");
    Usage();
    return 64;
  }
  if (segment_split_given > 1 || (segment_split_given && (!segment || !labels_file.empty()))) {
    std::printf("--segment-split R and --segment-split-d2 N are two forms of one option: give one, and only with --segment\n");
    Usage();
    return 64;
  }
  if ((segment_bins_given || segment_range_given) && !segment_token[0] && !segment_token[1] && !histogram) {
    std::printf("--segment-bins and --segment-range lay the bins of a histogram: they need otsu, otsu1 or otsu2 in --segment, or --histogram\n");
    Usage();
    return 64;
  }
  if ((track && !segment) || (track_min_given && !track)) {
    std::printf("--track follows the bodies --segment makes: it needs --segment, and --track-min-fraction needs --track\n");
    Usage();
    return 64;
  }
  if (track && (use_partial_gpu || concurrent > 1)) {
    std::printf("--track needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (track && !synthetic && files.size() > 2 && !from_frame_0) {
    std::printf("--track of more than two frames needs --cumulative or --total: the labels live on frame 0's grid, and only the displacement from "
                "frame 0 lives there too\n");
    Usage();
    return 64;
  }
  if (histogram && (use_partial_gpu || concurrent > 1)) {
    std::printf("--histogram needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (segment && (use_partial_gpu || concurrent > 1)) {
    std::printf("--segment needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if ((contacts && labels_file.empty() && !segment) || (contact_min_given && !contacts)) {
    std::printf("--contacts needs --labels FILE, and --contact-min-faces needs --contacts\n");
    Usage();
    return 64;
  }
  if (contacts && (use_partial_gpu || concurrent > 1)) {
    std::printf("--contacts needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (contacts && !synthetic && files.size() > 2 && !from_frame_0) {
    std::printf("--contacts of more than two frames needs --cumulative or --total: the labels live on frame 0's grid, and only the displacement "
                "from frame 0 lives there too\n");
    Usage();
    return 64;
  }
  if (label_shape && labels_file.empty() && !segment) {
    std::printf("--label-shape needs --labels FILE or --segment\n");
    Usage();
    return 64;
  }
  if (label_shape && (use_partial_gpu || concurrent > 1)) {
    std::printf("--label-shape needs the resident driver, which holds the labels: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if ((label_stats_bins_given || label_stats_paint) && label_stats.empty()) {
    std::printf("--label-stats-bins and --label-stats-paint need --label-stats\n");
    Usage();
    return 64;
  }
  if (!label_stats.empty() && labels_file.empty() && !segment) {
    std::printf("--label-stats needs --labels FILE or --segment\n");
    Usage();
    return 64;
  }
  if (!label_stats.empty() && (use_partial_gpu || concurrent > 1)) {
    std::printf("--label-stats needs the resident driver, which holds the labels and the fields: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  bool label_stats_of_pair = false;  // a name besides grey
  for (const std::string& name : label_stats) {
    const char* option = nullptr;
    if (name == "vol" && !(strain_fields & F3D_STRAIN_VOL)) option = "--strain vol";
    if (name == "eq" && !(strain_fields & F3D_STRAIN_EQ)) option = "--strain eq";
    if (name == "gmax" && !(principal_fields & F3D_PRINCIPAL_SHEAR)) option = "--principal shear";
    if (name == "angle" && !(polar_fields & F3D_POLAR_ANGLE)) option = "--rotation angle";
    if (name == "zncc" && !(match_fields & OpticalFlowE::kMatchZncc)) option = "--match zncc";
    if (name == "rmsd" && !(match_fields & OpticalFlowE::kMatchRmsd)) option = "--match rmsd";
    if (name == "wvol" && !(wstrain_fields & F3D_STRAIN_VOL)) option = "--window-strain vol";
    if (name == "weq" && !(wstrain_fields & F3D_STRAIN_EQ)) option = "--window-strain eq";
    if (option) {
      std::printf("--label-stats %s needs %s, which computes the field\n", name.c_str(), option);
      Usage();
      return 64;
    }
    if ((name == "zncc" || name == "rmsd") && cumulative) {
      std::printf("--label-stats %s cannot be combined with --cumulative: the fields of --match live on the pair's grid\n", name.c_str());
      Usage();
      return 64;
    }
    if (name != "grey") label_stats_of_pair = true;
  }
  if (label_stats_of_pair && !synthetic && files.size() > 2 && !from_frame_0) {
    std::printf("--label-stats of a field of more than two frames needs --cumulative or --total: the labels live on frame 0's grid, and only the "
                "displacement from frame 0 lives there too\n");
    Usage();
    return 64;
  }
  if ((!contacts && !segment && !label_shape && label_stats.empty() && labels_file.empty() != (label_model < 0)) || (label_min_given && label_model < 0)) {
    std::printf("--labels and --label-motion need each other, and --label-min-voxels needs both\n");
    Usage();
    return 64;
  }
  if (label_model >= 0 && (use_partial_gpu || concurrent > 1)) {
    std::printf("--label-motion needs the resident driver solving the pairs in order: it cannot be combined with %s\n",
                use_partial_gpu ? "--partial" : "--concurrent N > 1");
    Usage();
    return 64;
  }
  if (label_model >= 0 && !synthetic && files.size() > 2 && !from_frame_0) {
    std::printf("--label-motion of more than two frames needs --cumulative or --total: the labels live on frame 0's grid, and only the displacement "
                "from frame 0 lives there too\n");
    Usage();
    return 64;
  }
  // the segmentation is read before any device is touched: a file of another size or without a body is an argument error
  std::vector<int> label_volume;
  size_t n_labels = 0, n_bodies = 0;  // the largest label, and how many of 1 .. n_labels occur
  if ((label_model >= 0 || contacts || label_shape || !label_stats.empty()) && !segment) {
    const size_t count = width * height * depth;
    std::FILE* f = std::fopen(labels_file.c_str(), "rb");
    bool good = f != nullptr;
    if (good) {
      // the size first: nothing is allocated for a file that is not this volume
      good = std::fseek(f, 0, SEEK_END) == 0 && static_cast<size_t>(std::ftell(f)) == count * sizeof(int);
      if (good) {
        std::rewind(f);
        label_volume.resize(count);
        good = std::fread(label_volume.data(), sizeof(int), count, f) == count;
      }
      std::fclose(f);
    }
    if (!good) {
      std::printf("--labels %s: cannot read %zu x %zu x %zu int32 values (%zu bytes)\n", labels_file.c_str(), width, height, depth,
                  count * sizeof(int));
      Usage();
      return 64;
    }
    const int largest = *std::max_element(label_volume.begin(), label_volume.end());
    if (largest < 1 || largest > (1 << 22)) {
      std::printf("--labels %s: the largest label is %d; it must be 1 .. %d\n", labels_file.c_str(), largest, 1 << 22);
      Usage();
      return 64;
    }
    n_labels = static_cast<size_t>(largest);
    if (contacts) {
      std::vector<char> seen(n_labels + 1, 0);
      for (int l : label_volume)
        if (l >= 1) seen[static_cast<size_t>(l)] = 1;
      for (char c : seen) n_bodies += c;
    }
  }

  std::printf("//----------------------------------------------------------------------//\n");
  std::printf("//        3D optical flow, MI355X-native (HIP / CDNA4) implementation     //\n");
  std::printf("//----------------------------------------------------------------------//\n");

  if (!InitDeviceContextWithFirstAvailableDevice()) return 1;

  DataSize4 data_size = {width, height, depth, 0};
  OperationParameters params;
  params.PushValuePtr("warp_levels_count", &warp_levels_count);
  params.PushValuePtr("warp_scale_factor", &warp_scale_factor);
  params.PushValuePtr("outer_iterations_count", &outer_iterations_count);
  params.PushValuePtr("inner_iterations_count", &inner_iterations_count);
  params.PushValuePtr("equation_alpha", &equation_alpha);
  params.PushValuePtr("equation_smoothness", &equation_smoothness);
  params.PushValuePtr("equation_data", &equation_data);
  params.PushValuePtr("median_radius", &median_radius);
  params.PushValuePtr("gaussian_sigma", &gaussian_sigma);
  auto load = [&](Data3D& frame, const std::string& path) {
    return f32_input ? frame.ReadRAWFromFileF32(path.c_str(), width, height, depth)
                     : frame.ReadRAWFromFileU8(path.c_str(), width, height, depth);
  };
  Data3D frame_0, frame_1;
  Data3D flow_u(width, height, depth), flow_v(width, height, depth), flow_w(width, height, depth);
  const size_t pairs = synthetic ? 1 : files.size() - 1;
  if (synthetic) {
    if (!frame_0.Allocate(width, height, depth) || !frame_1.Allocate(width, height, depth)) return 2;
    f3d_synth::TranslatedGaussianPair(width, height, depth, frame_0.DataPtr(), frame_1.DataPtr());
  } else if (!load(frame_0, files[0])) {
    return 2;
  }
  const std::string suffix = "-" + std::to_string(width) + "-" + std::to_string(height) + "-" + std::to_string(depth) +
                             (use_partial_gpu ? "-partial.raw" : ".raw");

  if (use_partial_gpu) {
    OpticalFlowP optical_flow_p;
    if (!optical_flow_p.Initialize(data_size)) return 3;
    std::printf("Mode: Partial processing mode \n");
    optical_flow_p.silent = silent_mode;
    optical_flow_p.full_pipeline = partial_full;  // pre-blur and median as in the resident mode (the reference's piecemeal driver has neither)
    for (size_t k = 0; k < pairs; ++k) {
      if (!synthetic && !load(frame_1, files[k + 1])) return 2;
      optical_flow_p.ComputeFlow(frame_0, frame_1, flow_u, flow_v, flow_w, params);
      if (print_stats) {
        CudaOperationStatP stat_p;
        Stat3 stat = {0.f, 0.f, 0.f};
        OperationParameters op;
        op.PushValuePtr("flow_u", &flow_u);
        op.PushValuePtr("flow_v", &flow_v);
        op.PushValuePtr("flow_w", &flow_w);
        op.PushValuePtr("data_size", &data_size);
        op.PushValuePtr("stat", &stat);
        stat_p.silent = true;
        if (stat_p.Initialize()) stat_p.Execute(op);
        std::printf("Flow magnitude  min: %8.4f  max: %8.4f  avg: %8.4f\n", stat.min, stat.max, stat.avg);
      }
      const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
      flow_u.WriteRAWToFileF32((tag + "_flow-u" + suffix).c_str());
      flow_v.WriteRAWToFileF32((tag + "_flow-v" + suffix).c_str());
      flow_w.WriteRAWToFileF32((tag + "_flow-w" + suffix).c_str());
      if (write_vtk) Data3D::WriteFlowToFileVTK((tag + "_flow.vtk").c_str(), flow_u, flow_v, flow_w);
      std::printf("pair %zu of %zu: %.3f s, %zu solver residencies, %zu levels streamed, %zu levels on the device\n", k + 1, pairs,
                  optical_flow_p.LastDeviceSeconds(), optical_flow_p.LastSolvePasses(), optical_flow_p.LastStreamedLevels(),
                  optical_flow_p.LastResidentLevels());
      if (pairs > 1) frame_0.Swap(frame_1);
    }
    optical_flow_p.Destroy();
    f3d_host_shutdown();
    return 0;
  }

  if (concurrent > 1 && pairs > 1) {
    // N pairs at once: every worker thread binds a lane of its own and drives a driver of its own on it
    const size_t workers = std::min(concurrent, pairs);
    std::printf("Mode: Full GPU mode, %zu pairs at a time\n", workers);
    std::mutex print_mutex;
    std::atomic<int> failed{0};
    const auto t_start = std::chrono::steady_clock::now();
    auto work = [&](size_t me) {
      f3d_lane lane = nullptr;
      if (CheckDeviceError(f3d_lane_create(&lane)) || CheckDeviceError(f3d_lane_make_current(lane))) {
        failed = 3;
        return;
      }
      {
        OpticalFlowE flow;
        Data3D f0, f1, u(width, height, depth), v(width, height, depth), w(width, height, depth);
        bool ok;
        {
          std::lock_guard<std::mutex> lock(print_mutex);   // the set-up lines of one driver at a time
          ok = flow.Initialize(data_size);
        }
        flow.silent = true;
        // the bag holds pointers to main's variables, which nobody writes from here on: the workers share it read-only
        for (size_t k = me; ok && k < pairs && !failed; k += workers) {
          if (!load(f0, files[k]) || !load(f1, files[k + 1])) {
            failed = 2;
            break;
          }
          flow.ComputeFlow(f0, f1, u, v, w, params);
          const std::string tag = prefix + "_" + std::to_string(k);
          u.WriteRAWToFileF32((tag + "_flow-u" + suffix).c_str());
          v.WriteRAWToFileF32((tag + "_flow-v" + suffix).c_str());
          w.WriteRAWToFileF32((tag + "_flow-w" + suffix).c_str());
          if (write_vtk) Data3D::WriteFlowToFileVTK((tag + "_flow.vtk").c_str(), u, v, w);
          std::lock_guard<std::mutex> lock(print_mutex);
          std::printf("pair %zu of %zu done by worker %zu\n", k + 1, pairs, me);
        }
        if (!ok) failed = 3;
        flow.Destroy();
      }
      f3d_lane_make_current(nullptr);
      f3d_lane_destroy(lane);
    };
    std::vector<std::thread> threads;
    for (size_t t = 0; t < workers; ++t) threads.emplace_back(work, t);
    for (std::thread& t : threads) t.join();
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    std::printf("%zu pairs in %.3f s: %.2f pairs per second with %zu at a time\n", pairs, secs, pairs / secs, workers);
    f3d_host_shutdown();
    return failed;
  }

  OpticalFlowE optical_flow_e;
  if (!optical_flow_e.Initialize(data_size)) {
    std::printf("The resident driver needs 15 containers of the volume on the device; for larger volumes run with --partial\n"
                "(host-resident volumes streamed through the GPU, no pre-blur and no median like the reference's piecemeal driver).\n");
    return 3;
  }
  if (!optical_flow_e.AllocateResidentFrames()) return 3;
  std::printf("Mode: Full GPU mode \n");
  if ((label_model >= 0 || contacts || label_shape || !label_stats.empty()) && !segment) {
    if (!optical_flow_e.UploadLabels(label_volume.data())) return 3;
    std::vector<int>().swap(label_volume);
  }
  optical_flow_e.silent = silent_mode;
  optical_flow_e.collect_level_statistics = print_stats;

  // --label-shape: the shape table of the `bodies` labels on the device into <tag>_shapes.csv and one line; 0 or the exit status
  auto write_shapes = [&](size_t bodies) -> int {
    if (bodies > (static_cast<size_t>(1) << 22)) {
      std::printf("Error: --label-shape takes at most %d bodies, not %zu: raise --segment-min-voxels so that the small ones get no label\n",
                  1 << 22, bodies);
      return 3;
    }
    std::vector<f3d_label_shape> shapes(bodies);
    if (bodies && !optical_flow_e.ComputeLabelShapes(bodies, shapes.data(), nullptr)) {
      std::printf("Error: %s\n", optical_flow_e.DerivedError(OpticalFlowE::kLabelMotion).c_str());
      return 3;
    }
    const std::string tag = pairs > 1 ? prefix + "_0" : prefix;
    std::FILE* csv = std::fopen((tag + "_shapes.csv").c_str(), "w");
    size_t empty = 0, touching = 0, holed = 0;
    std::vector<double> diameters, sphericities;
    if (csv) {
      std::fprintf(csv, "label,status,voxels,x_lo,y_lo,z_lo,x_hi,y_hi,z_hi,border_x,border_y,border_z,centroid_x,centroid_y,centroid_z,"
                        "diameter,semi_axis_1,semi_axis_2,semi_axis_3,axis_1_x,axis_1_y,axis_1_z,axis_2_x,axis_2_y,axis_2_z,axis_3_x,"
                        "axis_3_y,axis_3_z,faces,surface,sphericity,euler\n");
      for (size_t l = 0; l < bodies; ++l) {
        const f3d_label_shape& s = shapes[l];
        std::fprintf(csv, "%zu,%d,%llu,%lld,%lld,%lld,%lld,%lld,%lld,%llu,%llu,%llu", l + 1, s.status, s.voxels, s.box_lo[0], s.box_lo[1],
                     s.box_lo[2], s.box_hi[0], s.box_hi[1], s.box_hi[2], s.border[0], s.border[1], s.border[2]);
        std::fprintf(csv, ",%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g", s.centroid[0], s.centroid[1], s.centroid[2], s.diameter, s.semi_axes[0],
                     s.semi_axes[1], s.semi_axes[2]);
        for (int i = 0; i < 9; ++i) std::fprintf(csv, ",%.9g", s.axes[i]);
        std::fprintf(csv, ",%llu,%.9g,%.9g,%lld\n", s.faces, s.surface, s.sphericity, s.euler);
        if (s.status != F3D_LABEL_OK) {
          ++empty;
          continue;
        }
        if (s.border[0] + s.border[1] + s.border[2]) ++touching;
        if (s.euler != 1) ++holed;
        diameters.push_back(s.diameter);
        sphericities.push_back(s.sphericity);
      }
    }
    const bool csv_error = csv && std::ferror(csv) != 0;
    if (!csv || std::fclose(csv) != 0 || csv_error) {
      std::printf("Error: cannot write %s_shapes.csv\n", tag.c_str());
      return 2;
    }
    // the upper median of the bodies that have a voxel; nan without one
    auto median = [](std::vector<double>& v) {
      if (v.empty()) return std::nan("");
      std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
      return v[v.size() / 2];
    };
    std::printf("shapes frame 0: %zu bodies, %zu empty, %zu touch the border, median diameter %.6g, median sphericity %.6g, %zu with Euler "
                "number != 1\n", bodies, empty, touching, median(diameters), median(sphericities), holed);
    return 0;
  };
  if (label_shape && !segment)
    if (const int status = write_shapes(n_labels)) return status;

  // --label-stats: the statistics of one named field over the `stats_labels` labels on the device, as rows of the pair's table
  // (`stats_rows`, written by flush_stats), one line, and with --label-stats-paint the painted means; 0 or the exit status
  size_t stats_labels = n_labels;  // the bodies of --segment once it has run
  std::string stats_rows;
  auto stats_of = [&](const std::string& name, size_t k, bool whole_line) -> int {
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    const auto failed = [&]() {
      std::printf("Error: %s\n", optical_flow_e.DerivedError(OpticalFlowE::kLabelMotion).c_str());
      return 3;
    };
    if (stats_labels == 0 || stats_labels > (static_cast<size_t>(1) << 22)) {
      std::printf("Error: --label-stats takes 1 .. %d bodies, not %zu; --segment-min-voxels decides which get a label\n", 1 << 22, stats_labels);
      return 3;
    }
    const DevicePtr field = optical_flow_e.NamedField(name.c_str());
    if (!field) {
      std::printf("Error: --label-stats %s: the field is not on the device\n", name.c_str());
      return 3;
    }
    float range[2] = {0.f, 0.f};
    f3d_range_info found = {};
    if (!optical_flow_e.LabelFieldRange(field, &range[0], &range[1], &found)) return failed();
    const int shift = f3d_label_field_shift(range[0], range[1], found.finite);
    // a constant field has no range for bins, and neither has one whose width or scale overflows float32 (f3d_histogram's rule)
    const float span = range[1] - range[0];
    const bool has_range = found.finite != 0 && range[0] < range[1] && std::isfinite(span) && label_stats_bins != 0 &&
                           std::isfinite(static_cast<float>(label_stats_bins) / span);
    const size_t bins = has_range ? label_stats_bins : 0;
    std::vector<f3d_label_field_stat> stats(stats_labels);
    std::vector<unsigned> counts(stats_labels * bins);
    f3d_label_field_info info = {};
    f3d_label_field_summary sum = {};
    if (!optical_flow_e.ComputeLabelField(field, stats_labels, shift, bins ? range : nullptr, bins, 1, stats.data(),
                                          bins ? counts.data() : nullptr, &info, &sum))
      return failed();
    char row[512];
    for (size_t l = 0; l < stats_labels; ++l) {
      const f3d_label_field_stat& s = stats[l];
      std::snprintf(row, sizeof(row), "%s,%zu,%s,%llu,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%llu,%llu\n", name.c_str(), l + 1,
                    s.status == F3D_LABEL_OK ? "ok" : s.status == F3D_LABEL_EMPTY ? "empty" : "small", s.n, s.min, s.max, s.mean, s.std,
                    s.q05, s.median, s.q95, s.below, s.above);
      stats_rows += row;
    }
    if (whole_line)
      std::printf("label stats %s frame %zu -> frame %zu: ", name.c_str(), from_frame_0 ? size_t(0) : k, k + 1);
    else
      std::printf("label stats %s frame 0: ", name.c_str());
    std::printf("%llu ok, %llu empty, %llu small of %zu labels, mean %.9g; shift %d, %zu bins over [%.9g, %.9g]; %llu voxels used, %llu "
                "nan, %llu out of range, %llu foreign\n", sum.ok, sum.empty, sum.small, stats_labels, sum.mean, shift, bins,
                static_cast<double>(range[0]), static_cast<double>(range[1]), info.used, info.nan, info.out_of_range, info.foreign);
    if (label_stats_paint) {
      std::vector<float> means(stats_labels);
      for (size_t l = 0; l < stats_labels; ++l)
        means[l] = stats[l].status == F3D_LABEL_OK ? static_cast<float>(stats[l].mean) : std::nanf("");
      Data3D painted;
      if (!painted.Allocate(width, height, depth)) return 2;
      if (!optical_flow_e.PaintLabels(means.data(), stats_labels, &painted)) return failed();
      painted.WriteRAWToFileF32((tag + "_labelmean-" + name + suffix).c_str());
    }
    return 0;
  };
  auto flush_stats = [&](size_t k) -> int {
    if (stats_rows.empty()) return 0;
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    std::FILE* csv = std::fopen((tag + "_labelstats.csv").c_str(), "w");
    if (csv) {
      std::fprintf(csv, "field,label,status,n,min,max,mean,std,q05,median,q95,below,above\n");
      std::fwrite(stats_rows.data(), 1, stats_rows.size(), csv);
    }
    stats_rows.clear();
    const bool csv_error = csv && std::ferror(csv) != 0;
    if (!csv || std::fclose(csv) != 0 || csv_error) {
      std::printf("Error: cannot write %s_labelstats.csv\n", tag.c_str());
      return 2;
    }
    return 0;
  };
  const bool stats_grey = std::find(label_stats.begin(), label_stats.end(), "grey") != label_stats.end();
  // grey: once, when the labels and the raw frame 0 of the first pair are both on the device; its rows lead the first pair's table
  auto stats_of_frame_0 = [&]() -> int {
    if (!stats_grey) return 0;
    if (const int status = stats_of("grey", 0, false)) return status;
    return label_stats_of_pair ? 0 : flush_stats(0);
  };
  // the fields of pair k, right after they were computed
  auto stats_of_pair = [&](size_t k) -> int {
    if (!label_stats_of_pair) return 0;
    for (const std::string& name : label_stats)
      if (name != "grey")
        if (const int status = stats_of(name, k, true)) return status;
    return flush_stats(k);
  };

  auto report = [&]() {
    Stat3 stat = {0.f, 0.f, 0.f};
    if (optical_flow_e.ResultStatistics(stat))
      std::printf("Flow magnitude  min: %8.4f  max: %8.4f  avg: %8.4f\n", stat.min, stat.max, stat.avg);
    if (silent_mode)  // otherwise the driver has printed each level as it went
      for (const OpticalFlowE::LevelStatistics& st : optical_flow_e.LevelStats())
        std::printf("level %2d (%4zu x%4zu x%4zu)  residual before the solve: rms %.5f  mean |.| %.5f  max %.4f;  flow after it: "
                    "min %.4f  max %.4f  avg %.4f\n", st.level, st.size.width, st.size.height, st.size.depth, st.before.rms,
                    st.before.mean_abs, st.before.max_abs, st.flow.min, st.flow.max, st.flow.avg);
    OpticalFlowE::Residual reg, unreg;
    if (optical_flow_e.FinalResidual(reg, unreg))
      std::printf("Registration residual (frame_1 warped by the flow vs frame_0)  rms: %.5f  mean |.|: %.5f  max: %.4f   "
                  "(unregistered  rms: %.5f  mean |.|: %.5f  max: %.4f)\n", reg.rms, reg.mean_abs, reg.max_abs, unreg.rms,
                  unreg.mean_abs, unreg.max_abs);
  };
  auto write_pair = [&](size_t k, Data3D& u, Data3D& v, Data3D& w) {
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    u.WriteRAWToFileF32((tag + "_flow-u" + suffix).c_str());
    v.WriteRAWToFileF32((tag + "_flow-v" + suffix).c_str());
    w.WriteRAWToFileF32((tag + "_flow-w" + suffix).c_str());
    if (write_vtk) Data3D::WriteFlowToFileVTK((tag + "_flow.vtk").c_str(), u, v, w);
  };
  // --cumulative: the displacement frame 0 -> frame k+1 and how many points have left the volume (NaN)
  Data3D disp[3];
  if (cumulative)
    for (Data3D& d : disp)
      if (!d.Allocate(width, height, depth)) return 2;
  auto write_disp = [&](size_t k) {
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    disp[0].WriteRAWToFileF32((tag + "_disp-u" + suffix).c_str());
    disp[1].WriteRAWToFileF32((tag + "_disp-v" + suffix).c_str());
    disp[2].WriteRAWToFileF32((tag + "_disp-w" + suffix).c_str());
    if (write_vtk) Data3D::WriteFlowToFileVTK((tag + "_disp.vtk").c_str(), disp[0], disp[1], disp[2]);
    const float* u = disp[0].DataPtr();
    const size_t n = width * height * depth;
    size_t lost = 0;
    for (size_t i = 0; i < n; ++i) lost += std::isnan(u[i]) ? 1 : 0;
    std::printf("displacement frame 0 -> frame %zu: %zu of %zu voxels have left the volume\n", k + 1, lost, n);
  };
  // --strain, --principal, --rotation, --inverse: the derived fields of pair k (of its flow, or with --cumulative of the displacement
  // frame 0 -> frame k+1) and the statistics the device computed with them; --match: always of the pair's flow and the pair's frames.
  // One descriptor per feature; `order` below is the order in which they run on the library stream and go down on the `down` queue.
  struct DerivedField {
    const char* option;  // without the dashes; the files are <tag>_<option>-<name><suffix>
    OpticalFlowE::Derived which;
    unsigned fields;     // the selection; 0 when the option was not given
    const char* const* names;
    bool of_pair;        // computed of the pair's flow also under --cumulative
    std::function<bool(const OpticalFlowE::Displacement&)> compute;
    std::function<void(size_t)> print;  // the statistics line of pair k
    Data3D host[OpticalFlowE::kMaxDerivedFields];
    Data3D* out[OpticalFlowE::kMaxDerivedFields] = {};
    // sequence mode: the kernel of pair k has run (`done`); its fields have gone down, so pair k+1 may rewrite them (`down`)
    f3d_event done = nullptr, down = nullptr;
  };
  static const char* const strain_names[8] = {"vol", "exx", "eyy", "ezz", "exy", "exz", "eyz", "eq"};
  static const char* const wstrain_names[17] = {"vol", "exx", "eyy", "ezz", "exy", "exz", "eyz", "eq", "G00",
                                               "G01", "G02", "G10", "G11", "G12", "G20", "G21", "G22"};
  static const char* const principal_names[10] = {"e1", "e2", "e3", "gmax", "d1x", "d1y", "d1z", "d3x", "d3y", "d3z"};
  static const char* const polar_names[7] = {"theta", "rx", "ry", "rz", "l1", "l2", "l3"};
  static const char* const inverse_names[4] = {"u", "v", "w", "err"};
  static const char* const match_names[3] = {"warped", "zncc", "rmsd"};
  static const char* const motion_names[3] = {"u", "v", "w"};
  static const char* const motion_models[3] = {"translation", "rigid", "affine"};
  static const char* const validated_names[4] = {"r", "u", "v", "w"};
  static const char* const labelres_names[4] = {"u", "v", "w", "labels"};
  static const char* const label_status[4] = {"ok", "empty", "small", "degenerate"};
  std::vector<f3d_motion_fit> label_fits(n_labels);
  std::vector<int> label_state(n_labels);
  std::vector<double> label_rms_after(n_labels);
  f3d_label_info label_info = {};
  bool label_table_failed = false;  // a <tag>_labelmotion.csv that could not be written: the run ends with 2 like an unreadable frame
  const size_t voxels = width * height * depth;
  f3d_strain_stats strain_stats = {};
  f3d_window_strain_stats wstrain_stats = {};
  f3d_principal_stats principal_stats = {};
  f3d_polar_stats polar_stats = {};
  f3d_principal_stats wprincipal_stats = {};
  f3d_polar_stats wpolar_stats = {};
  f3d_inverse_stats inverse_stats = {};
  f3d_correlation_stats match_stats = {};
  f3d_motion_fit motion_fit = {};
  f3d_motion_residual motion_residual = {};
  f3d_validate_stats validate_stats = {};
  // --use-validated: what --strain, --window-strain, --window-principal, --window-rotation, --principal, --rotation and --detrend are
  // computed of
  auto validated_or = [&](const OpticalFlowE::Displacement& of) {
    if (!use_validated) return of;
    const DevicePtr d[3] = {optical_flow_e.DerivedContainer(OpticalFlowE::kValidated, 1),
                            optical_flow_e.DerivedContainer(OpticalFlowE::kValidated, 2),
                            optical_flow_e.DerivedContainer(OpticalFlowE::kValidated, 3)};
    return OpticalFlowE::Containers(d);
  };
  DerivedField derived[11] = {
      {"strain", OpticalFlowE::kStrain, strain_fields, strain_names, false,
       [&](const OpticalFlowE::Displacement& of) { return optical_flow_e.ComputeStrain(validated_or(of), strain_fields, &strain_stats); },
       [&](size_t k) {
         const f3d_strain_stats& st = strain_stats;
         const double mean = st.defined ? st.vol_sum / static_cast<double>(st.defined) : std::nan("");
         std::printf("strain frame %zu -> frame %zu: vol min/mean/max %.6g/%.6g/%.6g, eq max %.6g, %llu folded, %llu undefined of %zu "
                     "voxels\n", from_frame_0 ? size_t(0) : k, k + 1, st.vol_min, mean, st.vol_max, st.eq_max, st.folded,
                     static_cast<unsigned long long>(voxels) - st.defined, voxels);
       }},
      {"principal", OpticalFlowE::kPrincipal, principal_fields, principal_names, false,
       [&](const OpticalFlowE::Displacement& of) { return optical_flow_e.ComputePrincipal(validated_or(of), principal_fields, &principal_stats); },
       [&](size_t k) {
         const f3d_principal_stats& st = principal_stats;
         std::printf("principal frame %zu -> frame %zu: e1 max %.6g, e3 min %.6g, shear max %.6g, %llu undefined of %zu voxels\n",
                     from_frame_0 ? size_t(0) : k, k + 1, st.e1_max, st.e3_min, st.shear_max,
                     static_cast<unsigned long long>(voxels) - st.defined, voxels);
       }},
      {"inverse", OpticalFlowE::kInverse, inverse ? 1u : 0u, inverse_names, false,
       [&](const OpticalFlowE::Displacement& of) {
         return optical_flow_e.ComputeInverse(of, inverse_iterations, inverse_tolerance, &inverse_stats);
       },
       [&](size_t k) {
         const f3d_inverse_stats& st = inverse_stats;
         const double mean = st.defined ? static_cast<double>(st.steps_sum) / static_cast<double>(st.defined) : std::nan("");
         std::printf("inverse frame %zu -> frame %zu: err max %.6g, mean steps %.6g, %llu unconverged, %llu lost of %zu voxels\n", k + 1,
                     from_frame_0 ? size_t(0) : k, st.err_max, mean, st.unconverged, static_cast<unsigned long long>(voxels) - st.defined,
                     voxels);
       }},
      // the frames of the pair are the resident pair: in a sequence SelectResidentPair(k, k+1) holds until the next solve begins
      {"match", OpticalFlowE::kMatch, match_fields, match_names, true,
       [&](const OpticalFlowE::Displacement& of) {
         return optical_flow_e.ComputeMatch(of, 0, 0, match_fields, match_radius, match_threshold, &match_stats);
       },
       [&](size_t k) {
         const f3d_correlation_stats& st = match_stats;
         const double mean = st.defined ? st.zncc_sum / static_cast<double>(st.defined) : std::nan("");
         std::printf("match frame %zu -> frame %zu: zncc min/mean %.6g/%.6g, %llu below %.6g, rmsd max %.6g, %llu flat, %llu lost of %zu "
                     "voxels\n", k, k + 1, st.zncc_min, mean, st.below, match_threshold, st.rmsd_max,
                     static_cast<unsigned long long>(voxels) - st.defined - st.lost, st.lost, voxels);
       }},
      // after the match: with --detrend-min-zncc the zncc container of this pair is the mask
      {"detrended", OpticalFlowE::kMotion, detrend_model >= 0 ? 1u : 0u, motion_names, false,
       [&](const OpticalFlowE::Displacement& of) {
         const DevicePtr mask = detrend_min_given ? optical_flow_e.DerivedContainer(OpticalFlowE::kMatch, 1) : 0;
         return optical_flow_e.ComputeMotion(validated_or(of), detrend_model, mask, detrend_min_zncc, &motion_fit, &motion_residual);
       },
       [&](size_t k) {
         const f3d_motion_fit& f = motion_fit;
         const f3d_motion_residual& r = motion_residual;
         std::printf("motion frame %zu -> frame %zu (%s): t (%.6g, %.6g, %.6g), ", from_frame_0 ? size_t(0) : k, k + 1,
                     motion_models[detrend_model], f.t[0], f.t[1], f.t[2]);
         if (detrend_model == F3D_MOTION_RIGID) {
           // degrees appear in this line only: the fit itself carries the cosine and the axial vector
           const double sine = std::sqrt((f.axial[0] * f.axial[0] + f.axial[1] * f.axial[1]) + f.axial[2] * f.axial[2]);
           const double unit = sine > 0 ? 1.0 / sine : 0.0;
           std::printf("angle %.6g deg about (%.6g, %.6g, %.6g), ", std::atan2(sine, f.cos_angle) * (180.0 / 3.14159265358979323846),
                       f.axial[0] * unit, f.axial[1] * unit, f.axial[2] * unit);
         } else if (detrend_model == F3D_MOTION_AFFINE) {
           std::printf("M (%.6g, %.6g, %.6g; %.6g, %.6g, %.6g; %.6g, %.6g, %.6g), ", f.M[0], f.M[1], f.M[2], f.M[3], f.M[4], f.M[5],
                       f.M[6], f.M[7], f.M[8]);
         }
         const double after = r.present ? std::sqrt(r.sum_sq / static_cast<double>(r.present)) : std::nan("");
         std::printf("rms %.6g -> %.6g, max |res| %.6g, %llu of %zu voxels\n", f.rms_before, after, r.max_abs, f.n, voxels);
       }},
      // after the match for the same reason; with --use-validated before the fields that are computed of it (`order` below)
      {"validated", OpticalFlowE::kValidated, validate_mode ? F3D_VALIDATE_R | F3D_VALIDATE_D : 0u, validated_names, false,
       [&](const OpticalFlowE::Displacement& of) {
         const DevicePtr mask = validate_min_given ? optical_flow_e.DerivedContainer(OpticalFlowE::kMatch, 1) : 0;
         return optical_flow_e.ComputeValidated(of, mask, validate_min_zncc, validate_step, validate_eps, validate_threshold,
                                                validate_min_neighbours, validate_mode, validate_fill,
                                                F3D_VALIDATE_R | F3D_VALIDATE_D, &validate_stats);
       },
       [&](size_t k) {
         const f3d_validate_stats& st = validate_stats;
         std::printf("validate frame %zu -> frame %zu (%s, step %u): %llu tested, %llu outliers, %llu replaced, %llu undefined, r max %.6g "
                     "of %zu voxels\n", from_frame_0 ? size_t(0) : k, k + 1, validate_mode == F3D_VALIDATE_MARK ? "mark" : "replace",
                     validate_step, st.tested, st.outliers, st.replaced, st.undefined, st.r_max, voxels);
       }},
      // listed last so that the indices above stay; it runs after the principal strains (`order` below)
      {"rotation", OpticalFlowE::kPolar, polar_fields, polar_names, false,
       [&](const OpticalFlowE::Displacement& of) { return optical_flow_e.ComputePolar(validated_or(of), polar_fields, &polar_stats); },
       [&](size_t k) {
         const f3d_polar_stats& st = polar_stats;
         const double mean = st.defined ? st.theta_sum / static_cast<double>(st.defined) : std::nan("");
         std::printf("rotation frame %zu -> frame %zu: angle max %.6g rad, mean %.6g rad, stretch max %.6g, min %.6g, %llu folded, %llu "
                     "undefined of %zu voxels\n", from_frame_0 ? size_t(0) : k, k + 1, st.theta_max, mean, st.l1_max, st.l3_min, st.folded,
                     static_cast<unsigned long long>(voxels) - st.defined - st.folded, voxels);
       }},
      // the same source as --detrend; the table of the labels is written with the line
      {"labelres", OpticalFlowE::kLabelMotion, label_model >= 0 ? 1u : 0u, labelres_names, false,
       [&](const OpticalFlowE::Displacement& of) {
         return optical_flow_e.ComputeLabelMotion(validated_or(of), n_labels, label_model, label_min_voxels, label_fits.data(),
                                                  label_state.data(), label_rms_after.data(), &label_info);
       },
       [&](size_t k) {
         const double degrees = 180.0 / 3.14159265358979323846;
         const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
         std::FILE* csv = std::fopen((tag + "_labelmotion.csv").c_str(), "w");
         if (csv) {
           std::fprintf(csv, "label,status,n,cx,cy,cz,tx,ty,tz,%srms_before,rms_after\n",
                        label_model == F3D_MOTION_RIGID ? "angle_deg,ax,ay,az,"
                        : label_model == F3D_MOTION_AFFINE ? "m00,m01,m02,m10,m11,m12,m20,m21,m22," : "");
         } else {
           std::printf("Error: cannot write %s_labelmotion.csv\n", tag.c_str());
           label_table_failed = true;
         }
         size_t count[4] = {0, 0, 0, 0};
         std::vector<double> length;
         double max_angle = 0.0;
         for (size_t l = 0; l < n_labels; ++l) {
           const f3d_motion_fit& f = label_fits[l];
           const int state = label_state[l];
           ++count[state];
           const double sine = std::sqrt((f.axial[0] * f.axial[0] + f.axial[1] * f.axial[1]) + f.axial[2] * f.axial[2]);
           const double unit = sine > 0 ? 1.0 / sine : 0.0;
           const double angle = std::atan2(sine, f.cos_angle) * degrees;
           if (state == F3D_LABEL_OK) {
             length.push_back(std::sqrt((f.t[0] * f.t[0] + f.t[1] * f.t[1]) + f.t[2] * f.t[2]));
             if (label_model == F3D_MOTION_RIGID) max_angle = std::max(max_angle, angle);
           }
           if (!csv) continue;
           std::fprintf(csv, "%zu,%s,%llu,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,", l + 1, label_status[state], f.n, f.centre[0], f.centre[1],
                        f.centre[2], f.t[0], f.t[1], f.t[2]);
           if (label_model == F3D_MOTION_RIGID)
             std::fprintf(csv, "%.9g,%.9g,%.9g,%.9g,", state == F3D_LABEL_OK ? angle : 0.0, f.axial[0] * unit, f.axial[1] * unit,
                          f.axial[2] * unit);
           else if (label_model == F3D_MOTION_AFFINE)
             std::fprintf(csv, "%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,", f.M[0], f.M[1], f.M[2], f.M[3], f.M[4], f.M[5], f.M[6],
                          f.M[7], f.M[8]);
           std::fprintf(csv, "%.9g,%.9g\n", f.rms_before, label_rms_after[l]);
         }
         const bool write_error = csv && std::ferror(csv) != 0;
         if (csv && (std::fclose(csv) != 0 || write_error)) {
           std::printf("Error: cannot write %s_labelmotion.csv\n", tag.c_str());
           label_table_failed = true;
         }
         double median = std::nan("");
         if (!length.empty()) {
           std::sort(length.begin(), length.end());
           median = length.size() % 2 ? length[length.size() / 2] : 0.5 * (length[length.size() / 2 - 1] + length[length.size() / 2]);
         }
         std::printf("label motion frame %zu -> frame %zu (%s): %zu labels fitted, %zu empty, %zu small, %zu degenerate; median |t| %.6g, ",
                     from_frame_0 ? size_t(0) : k, k + 1, motion_models[label_model], count[0], count[1], count[2], count[3], median);
         if (label_model == F3D_MOTION_RIGID) std::printf("max angle %.6g deg, ", max_angle);
         std::printf("%llu foreign, %llu out of range voxels\n", label_info.foreign, label_info.out_of_range);
       }},
      // the same source as --strain, after which it runs (`order` below)
      {"wstrain", OpticalFlowE::kWindowStrain, wstrain_fields, wstrain_names, false,
       [&](const OpticalFlowE::Displacement& of) {
         return optical_flow_e.ComputeWindowStrain(validated_or(of), wstrain_fields, window_radius, window_min_count, &wstrain_stats);
       },
       [&](size_t k) {
         const f3d_window_strain_stats& st = wstrain_stats;
         const double mean = st.defined ? st.vol_sum / static_cast<double>(st.defined) : std::nan("");
         std::printf("window strain (r=%u) frame %zu -> frame %zu: vol min/mean/max %.6g/%.6g/%.6g, eq max %.6g, %llu folded, %llu thin, "
                     "%llu lost of %zu voxels\n", window_radius, from_frame_0 ? size_t(0) : k, k + 1, st.vol_min, mean, st.vol_max,
                     st.eq_max, st.folded, st.thin, st.lost, voxels);
       }},
      // the principal strains and the rotation of the window's gradient: after the window strain, the lines of --principal / --rotation
      {"wprincipal", OpticalFlowE::kWindowPrincipal, wprincipal_fields, principal_names, false,
       [&](const OpticalFlowE::Displacement& of) {
         return optical_flow_e.ComputeWindowPrincipal(validated_or(of), wprincipal_fields, window_radius, window_min_count,
                                                      &wprincipal_stats);
       },
       [&](size_t k) {
         const f3d_principal_stats& st = wprincipal_stats;
         std::printf("window principal (r=%u) frame %zu -> frame %zu: e1 max %.6g, e3 min %.6g, shear max %.6g, %llu undefined of %zu "
                     "voxels\n", window_radius, from_frame_0 ? size_t(0) : k, k + 1, st.e1_max, st.e3_min, st.shear_max,
                     static_cast<unsigned long long>(voxels) - st.defined, voxels);
       }},
      {"wrotation", OpticalFlowE::kWindowPolar, wpolar_fields, polar_names, false,
       [&](const OpticalFlowE::Displacement& of) {
         return optical_flow_e.ComputeWindowPolar(validated_or(of), wpolar_fields, window_radius, window_min_count, &wpolar_stats);
       },
       [&](size_t k) {
         const f3d_polar_stats& st = wpolar_stats;
         const double mean = st.defined ? st.theta_sum / static_cast<double>(st.defined) : std::nan("");
         std::printf("window rotation (r=%u) frame %zu -> frame %zu: angle max %.6g rad, mean %.6g rad, stretch max %.6g, min %.6g, %llu "
                     "folded, %llu undefined of %zu voxels\n", window_radius, from_frame_0 ? size_t(0) : k, k + 1, st.theta_max, mean,
                     st.l1_max, st.l3_min, st.folded, static_cast<unsigned long long>(voxels) - st.defined - st.folded, voxels);
       }}};
  // --contacts: no field of voxels, so no DerivedField: the table of pair k is computed after the derived fields of pair k (the fits of
  // --label-motion are then those of the same displacement) and written after their files
  std::vector<f3d_contact> contact_list;
  std::vector<f3d_contact_kin> contact_kin;
  f3d_contact_info contact_info = {};
  auto compute_contacts = [&](const OpticalFlowE::Displacement& of) {
    if (!optical_flow_e.ComputeContacts(validated_or(of), n_labels, &contact_list, &contact_info)) {
      std::printf("Error: %s\n", optical_flow_e.DerivedError(OpticalFlowE::kLabelMotion).c_str());
      return false;
    }
    contact_kin.resize(contact_list.size());
    if (contact_list.empty()) return true;  // bodies that do not touch (those of --segment never do): nothing to project, and no array to pass
    const size_t dims[3] = {width, height, depth};
    const bool fitted = label_model >= 0;
    return f3d_contact_kinematics(contact_list.data(), contact_list.size(), dims, fitted ? label_fits.data() : nullptr,
                                  fitted ? label_state.data() : nullptr, fitted ? n_labels : 0, contact_min_faces,
                                  contact_kin.data()) == 0;
  };
  auto write_contacts = [&](size_t k) {
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    std::FILE* csv = std::fopen((tag + "_contacts.csv").c_str(), "w");
    if (csv) std::fprintf(csv, "lo,hi,status,faces_x,faces_y,faces_z,area,nx,ny,nz,px,py,pz,jump_normal,jump_slip,fit_normal,fit_slip\n");
    size_t opening = 0, closing = 0;
    double largest_slip = 0.0;
    for (size_t i = 0; i < contact_list.size(); ++i) {
      const f3d_contact& c = contact_list[i];
      const f3d_contact_kin& q = contact_kin[i];
      if (!(q.status & F3D_CONTACT_SMALL)) {
        if (q.jump_normal > 0x1p-14) ++opening;
        if (q.jump_normal < -0x1p-14) ++closing;
        if (q.jump_slip > largest_slip) largest_slip = q.jump_slip;
      }
      if (csv)
        std::fprintf(csv, "%d,%d,%u,%llu,%llu,%llu,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g\n", c.lo, c.hi, q.status, c.faces[0],
                     c.faces[1], c.faces[2], q.area, q.normal[0], q.normal[1], q.normal[2], q.point[0], q.point[1], q.point[2],
                     q.jump_normal, q.jump_slip, q.fit_normal, q.fit_slip);
    }
    const bool write_error = csv && std::ferror(csv) != 0;
    if (!csv || std::fclose(csv) != 0 || write_error) {
      std::printf("Error: cannot write %s_contacts.csv\n", tag.c_str());
      label_table_failed = true;
    }
    std::printf("contacts frame %zu -> frame %zu: %zu contacts between %zu bodies, mean coordination %.6g, %zu opening, %zu closing "
                "beyond 2^-14, largest slip %.6g; %llu contact faces, %llu without a jump, %llu foreign\n", from_frame_0 ? size_t(0) : k,
                k + 1, contact_list.size(), n_bodies, n_bodies ? 2.0 * static_cast<double>(contact_list.size()) / static_cast<double>(n_bodies) : 0.0,
                opening, closing, largest_slip, contact_info.contact, contact_info.jump_absent, contact_info.foreign);
  };
  // the order in which the features run and their files and lines come out: as listed, with the window strain and the two fields of
  // the window's gradient after the strain and the rotation after the principal strains,
  // or with --use-validated the match (whose zncc may be the mask) and the validated field first
  DerivedField* order[11] = {&derived[0], &derived[8], &derived[9], &derived[10], &derived[1], &derived[6],
                             &derived[2], &derived[3], &derived[4],  &derived[5],  &derived[7]};
  if (use_validated) {
    DerivedField* const first[11] = {&derived[3], &derived[5], &derived[0], &derived[8], &derived[9], &derived[10],
                                     &derived[1], &derived[6], &derived[2], &derived[4], &derived[7]};
    for (int i = 0; i < 11; ++i) order[i] = first[i];
  }
  for (DerivedField& f : derived)
    for (int i = 0; i < OpticalFlowE::DerivedFieldCount(f.which); ++i)
      if (OpticalFlowE::DerivedSelected(f.which, i, f.fields)) {
        if (!f.host[i].Allocate(width, height, depth)) return 2;
        f.out[i] = &f.host[i];
      }
  auto write_derived = [&](DerivedField& f, size_t k) {
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    for (int i = 0; i < OpticalFlowE::DerivedFieldCount(f.which); ++i)
      if (f.out[i]) f.host[i].WriteRAWToFileF32((tag + "_" + f.option + "-" + f.names[i] + suffix).c_str());
    f.print(k);
  };

  // --track: no field of voxels either.  Pair k is resident, so its raw later frame is: the bodies of frame k+1 with the numbers
  // --segment settled, their overlap with frame 0's bodies through `of`, the solve, the new numbers, and the two files, all before
  // the next solve is enqueued (every call waits for the stream).  0: fine; otherwise the exit status.
  size_t track_n_a = 0;  // the bodies of frame 0 (segment_frame_0)
  auto track_pair = [&](size_t k, const OpticalFlowE::Displacement& of) {
    const auto failed = [&]() {
      std::printf("Error: %s\n", optical_flow_e.DerivedError(OpticalFlowE::kLabelMotion).c_str());
      return 3;
    };
    f3d_split_info later = {};
    if (!optical_flow_e.ComputeLabelsB(0, segment_lo, segment_hi, segment_core_d2, segment_min_voxels, nullptr, &later)) return failed();
    if (later.n_labels > (1ull << 22)) {
      std::printf("Error: --track found %llu bodies in frame %zu and takes at most %d: raise --segment-min-voxels (now %llu)\n",
                  later.n_labels, k + 1, 1 << 22, segment_min_voxels);
      return 3;
    }
    // a frame without a body still has an answer: every body of frame 0 vanished.  Body 1 then has no voxel and comes out empty.
    const size_t n_b = std::max<size_t>(1, static_cast<size_t>(later.n_labels));
    std::vector<f3d_overlap> rows;
    f3d_overlap_info counted = {};
    if (!optical_flow_e.ComputeOverlap(validated_or(of), track_n_a, n_b, &rows, &counted)) return failed();
    std::vector<f3d_track_a> a(track_n_a);
    std::vector<f3d_track_b> b(n_b);
    std::vector<int> map_b(n_b);
    f3d_track_summary sum = {};
    if (f3d_overlap_solve(rows.data(), rows.size(), track_n_a, n_b, track_min_fraction, a.data(), b.data(), map_b.data(), &sum)) {
      std::printf("Error: %s\n", f3d_host_last_error());
      return 3;
    }
    std::vector<int> volume(width * height * depth);
    if (!optical_flow_e.RelabelB(map_b.data(), n_b) || !optical_flow_e.DownloadLabelsB(volume.data())) return failed();
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    std::FILE* raw = std::fopen((tag + "_tracked-labels.raw").c_str(), "wb");
    const bool raw_good = raw && std::fwrite(volume.data(), sizeof(int), volume.size(), raw) == volume.size();
    if ((raw && std::fclose(raw) != 0) || !raw_good) {
      std::printf("Error: cannot write %s_tracked-labels.raw\n", tag.c_str());
      return 2;
    }
    std::FILE* csv = std::fopen((tag + "_tracks.csv").c_str(), "w");
    double iou_sum = 0.0;
    if (csv) {
      std::fprintf(csv, "side,label,status,voxels,lost,background,unreached,best,n_best,partners,fraction,shift_x,shift_y,shift_z,iou,new_label\n");
      for (size_t i = 0; i < a.size(); ++i) {
        const f3d_track_a& t = a[i];
        std::fprintf(csv, "a,%zu,%u,%llu,%llu,%llu,0,%d,%llu,%d,%.9g,%.9g,%.9g,%.9g,%.9g,%zu\n", i + 1, t.status, t.n, t.n_lost, t.n_background,
                     t.best_b, t.n_best, t.n_targets, t.fraction, t.shift[0], t.shift[1], t.shift[2], t.iou, i + 1);
      }
      for (size_t i = 0; i < b.size(); ++i) {
        const f3d_track_b& t = b[i];
        std::fprintf(csv, "b,%zu,%u,%llu,0,0,%llu,%d,%llu,%d,nan,nan,nan,nan,nan,%d\n", i + 1, t.status, t.m, t.n_unreached, t.best_a, t.n_best,
                     t.n_sources, map_b[i]);
      }
    }
    const bool csv_error = csv && std::ferror(csv) != 0;
    if (!csv || std::fclose(csv) != 0 || csv_error) {
      std::printf("Error: cannot write %s_tracks.csv\n", tag.c_str());
      return 2;
    }
    for (const f3d_track_a& t : a)
      if (t.status & F3D_TRACK_MATCHED) iou_sum += t.iou;
    std::printf("track frame %zu -> frame %zu: %llu of %zu bodies matched, %llu split, %llu merged, %llu vanished, %llu appeared, %llu left; "
                "mean IoU %.6g; lost %llu, foreign %llu\n", from_frame_0 ? size_t(0) : k, k + 1, sum.matched, track_n_a, sum.split, sum.merged,
                sum.vanished, sum.appeared, sum.left, sum.matched ? iou_sum / static_cast<double>(sum.matched) : std::nan(""),
                counted.lost_body + counted.lost_background, counted.foreign_a + counted.foreign_b);
    return 0;
  };

  // --segment: the labels of frame 0, made while the first pair is resident and before anything reads labels.  0: fine; otherwise
  // the exit status.
  auto segment_frame_0 = [&]() {
    const std::string tag_0 = pairs > 1 ? prefix + "_0" : prefix;
    if (histogram || segment_token[0] || segment_token[1]) {
      std::vector<unsigned long long> counts(segment_bins);
      f3d_histogram_info counted = {};
      float range_lo = 0.f, range_hi = 0.f;
      if (!optical_flow_e.ComputeHistogram(0, segment_range_given ? segment_range : nullptr, segment_bins, counts.data(), &counted, &range_lo,
                                           &range_hi)) {
        std::printf("Error: %s\n", optical_flow_e.DerivedError(OpticalFlowE::kLabelMotion).c_str());
        return 3;
      }
      const double a = static_cast<double>(range_lo), b = static_cast<double>(range_hi);
      if (histogram) {
        std::FILE* csv = std::fopen((tag_0 + "_histogram.csv").c_str(), "w");
        if (csv) {
          std::fprintf(csv, "bin,lower_edge,count\n");
          for (size_t k = 0; k < segment_bins; ++k) {
            float edge = 0.f;
            if (f3d_histogram_edge(range_lo, range_hi, segment_bins, k, &edge)) {
              std::printf("Error: %s\n", f3d_host_last_error());
              std::fclose(csv);
              return 3;
            }
            std::fprintf(csv, "%zu,%.9g,%llu\n", k, static_cast<double>(edge), counts[k]);
          }
        }
        const bool csv_error = csv && std::ferror(csv) != 0;
        if (!csv || std::fclose(csv) != 0 || csv_error) {
          std::printf("Error: cannot write %s_histogram.csv\n", tag_0.c_str());
          return 2;
        }
        std::printf("histogram frame 0: %zu bins of [%.9g, %.9g]: %llu voxels counted, %llu NaN, %llu outside the range\n", segment_bins, a, b,
                    counted.used, counted.nan, counted.below + counted.above);
      }
      if (segment_token[0] || segment_token[1]) {
        const int classes = (segment_token[0] == 1 || segment_token[1] == 1) ? 2 : 3;
        unsigned cuts[2] = {0, 0};
        f3d_otsu_info chosen = {};
        if (f3d_otsu(counts.data(), segment_bins, classes, cuts, &chosen)) {
          std::printf("Error: %s\n", f3d_host_last_error());
          return 3;
        }
        if (chosen.status != F3D_OTSU_OK) {
          std::printf("Error: --segment otsu: fewer than %d of the %zu bins of [%.9g, %.9g] are occupied (%llu voxels counted): there is no "
                      "cut of %d classes\n", classes, segment_bins, a, b, counted.used, classes);
          return 3;
        }
        float edges[2] = {0.f, 0.f};
        for (int j = 0; j < classes - 1; ++j)
          if (f3d_histogram_edge(range_lo, range_hi, segment_bins, cuts[j], &edges[j])) {
            std::printf("Error: %s\n", f3d_host_last_error());
            return 3;
          }
        if (classes == 2)
          std::printf("threshold frame 0: otsu, 2 classes over %zu bins of [%.9g, %.9g]: cut at bin %u = %.9g (%llu | %llu voxels), %llu NaN, "
                      "%llu outside the range\n", segment_bins, a, b, cuts[0], static_cast<double>(edges[0]), chosen.populations[0],
                      chosen.populations[1], counted.nan, counted.below + counted.above);
        else
          std::printf("threshold frame 0: otsu, 3 classes over %zu bins of [%.9g, %.9g]: cuts at bins %u, %u = %.9g, %.9g (%llu | %llu | %llu "
                      "voxels), %llu NaN, %llu outside the range\n", segment_bins, a, b, cuts[0], cuts[1], static_cast<double>(edges[0]),
                      static_cast<double>(edges[1]), chosen.populations[0], chosen.populations[1], chosen.populations[2], counted.nan,
                      counted.below + counted.above);
        // LO is the edge itself (s >= e), HI the largest float below it (s < e)
        if (segment_token[0]) segment_lo = edges[segment_token[0] == 3 ? 1 : 0];
        if (segment_token[1]) segment_hi = std::nextafterf(edges[segment_token[1] == 3 ? 1 : 0], -INFINITY);
        if (segment_lo > segment_hi) {
          std::printf("Error: --segment: with the cut the range is [%.9g, %.9g]: LO is above HI\n", static_cast<double>(segment_lo),
                      static_cast<double>(segment_hi));
          return 3;
        }
      }
      if (!segment) return 0;
    }
    std::vector<unsigned long long> sizes;
    f3d_component_info info = {};
    f3d_split_info split = {};
    const bool labelled = segment_core_d2 ? optical_flow_e.ComputeSplitLabels(0, segment_lo, segment_hi, segment_core_d2, segment_min_voxels, &sizes, &split)
                                          : optical_flow_e.ComputeLabels(0, segment_lo, segment_hi, segment_min_voxels, &sizes, &info);
    if (!labelled) {
      std::printf("Error: %s\n", optical_flow_e.DerivedError(OpticalFlowE::kLabelMotion).c_str());
      return 3;
    }
    if (segment_core_d2) {  // the first eight counters are those of the classes
      const f3d_component_info classes = {split.foreground, split.background, split.nan, split.n_components, split.n_labels,
                                          split.dropped_components, split.dropped_voxels, split.largest};
      info = classes;
    }
    std::printf("bodies frame 0: %llu bodies of %llu foreground voxels (largest %llu), %llu bodies of %llu voxels dropped below %llu, "
                "%llu background, %llu NaN\n", info.n_labels, info.foreground, info.largest, info.dropped_components, info.dropped_voxels,
                segment_min_voxels, info.background, info.nan);
    if (segment_core_d2)
      std::printf("split at d2 >= %llu: %llu components, %llu cores, %llu remainder bodies of %llu voxels\n", segment_core_d2,
                  split.connected_components, split.n_cores, split.remainder_bodies, split.remainder_voxels);
    const std::string tag = pairs > 1 ? prefix + "_0" : prefix;
    std::vector<int> volume(width * height * depth);
    if (!optical_flow_e.DownloadLabels(volume.data())) {
      std::printf("Error: %s\n", optical_flow_e.DerivedError(OpticalFlowE::kLabelMotion).c_str());
      return 3;
    }
    std::FILE* raw = std::fopen((tag + "_labels.raw").c_str(), "wb");
    const bool raw_good = raw && std::fwrite(volume.data(), sizeof(int), volume.size(), raw) == volume.size();
    if ((raw && std::fclose(raw) != 0) || !raw_good) {
      std::printf("Error: cannot write %s_labels.raw\n", tag.c_str());
      return 2;
    }
    std::FILE* csv = std::fopen((tag + "_bodies.csv").c_str(), "w");
    if (csv) {
      std::fprintf(csv, "label,voxels\n");
      for (size_t l = 0; l < sizes.size(); ++l) std::fprintf(csv, "%zu,%llu\n", l + 1, sizes[l]);
    }
    const bool csv_error = csv && std::ferror(csv) != 0;
    if (!csv || std::fclose(csv) != 0 || csv_error) {
      std::printf("Error: cannot write %s_bodies.csv\n", tag.c_str());
      return 2;
    }
    if (label_shape)
      if (const int status = write_shapes(static_cast<size_t>(info.n_labels))) return status;
    stats_labels = static_cast<size_t>(info.n_labels);
    if (track) {
      if (info.n_labels == 0 || info.n_labels > (1ull << 22)) {
        std::printf("Error: --segment found %llu bodies and --track takes 1 .. %d; --segment-min-voxels is %llu\n", info.n_labels, 1 << 22,
                    segment_min_voxels);
        return 3;
      }
      track_n_a = static_cast<size_t>(info.n_labels);
    }
    if (label_model >= 0 || contacts) {
      if (info.n_labels == 0 || info.n_labels > (1ull << 22)) {
        std::printf(info.n_labels ? "Error: --segment found %llu bodies and --label-motion and --contacts take at most %d: raise "
                                    "--segment-min-voxels (now %llu) so that the small ones get no label\n"
                                  : "Error: --segment found no body (%llu) for --label-motion or --contacts; the most is %d, "
                                    "--segment-min-voxels is %llu\n", info.n_labels, 1 << 22, segment_min_voxels);
        return 3;
      }
      n_labels = n_bodies = static_cast<size_t>(info.n_labels);
      label_fits.assign(n_labels, f3d_motion_fit());
      label_state.assign(n_labels, 0);
      label_rms_after.assign(n_labels, 0.0);
    }
    return 0;
  };

  // --initial-flow, --warm-start, --total: what a pair starts from, and the line that says what was found in it
  auto say_initial = [&](const f3d_initial_info& found) {
    std::printf("initial flow: %llu replaced, %llu leaving, max |.| %.6g\n", found.replaced, found.leaving, static_cast<double>(found.max_abs));
  };
  auto initial_from_files = [&]() {
    Data3D guess[3];
    for (int i = 0; i < 3; ++i)
      if (!guess[i].ReadRAWFromFileF32(initial_files[i].c_str(), width, height, depth)) return 2;
    f3d_initial_info found = {};
    if (!optical_flow_e.SetInitialFlow(guess[0], guess[1], guess[2], &found)) {
      std::printf("Error: %s\n", optical_flow_e.InitialFlowError().c_str());
      return 3;
    }
    say_initial(found);
    return 0;
  };

  // --block-match: the node table of the resident pair into <tag>_blockmatch.csv, one line about it, and (unless only the table is
  // wanted) the guess of the pair's solve from it
  auto initial_from_block_match = [&](size_t k) {
    f3d_block_match_summary sum = {};
    if (!optical_flow_e.BlockMatch(block_match_params, nullptr, nullptr, &sum)) {
      std::printf("Error: %s\n", optical_flow_e.InitialFlowError().c_str());
      return 3;
    }
    const std::vector<f3d_block_match_node>& rows = optical_flow_e.BlockMatchNodes();
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    std::FILE* csv = std::fopen((tag + "_blockmatch.csv").c_str(), "w");
    if (!csv) {
      std::printf("Error: cannot write %s_blockmatch.csv\n", tag.c_str());
      return 2;
    }
    static const char* const kStatus[] = {"ok", "flat", "none", "low", "edge"};
    std::fprintf(csv, "x,y,z,shift_x,shift_y,shift_z,offset_x,offset_y,offset_z,zncc,status,evaluated,outside,flat\n");
    std::vector<double> lengths;
    for (const f3d_block_match_node& r : rows) {
      std::fprintf(csv, "%d,%d,%d,%d,%d,%d,%.17g,%.17g,%.17g,%.17g,%s,%d,%d,%d\n", r.position[0], r.position[1], r.position[2], r.shift[0],
                   r.shift[1], r.shift[2], r.offset[0], r.offset[1], r.offset[2], r.zncc, kStatus[r.status], r.evaluated, r.outside, r.flat);
      if (r.status == F3D_BLOCK_NODE_OK || r.status == F3D_BLOCK_NODE_EDGE)
        lengths.push_back(std::sqrt(static_cast<double>(r.u) * r.u + static_cast<double>(r.v) * r.v + static_cast<double>(r.w) * r.w));
    }
    std::fclose(csv);
    // the upper median and the maximum of |shift + offset| over the nodes that have a vector; nan without one
    double median = std::nan(""), largest = std::nan("");
    if (!lengths.empty()) {
      std::nth_element(lengths.begin(), lengths.begin() + lengths.size() / 2, lengths.end());
      median = lengths[lengths.size() / 2];
      largest = *std::max_element(lengths.begin(), lengths.end());
    }
    std::printf("block match: %llu nodes, %llu ok, %llu low, %llu flat, %llu edge, %llu none, median shift %.4f, largest %.4f\n", sum.nodes, sum.ok,
                sum.low, sum.flat, sum.edge, sum.none, median, largest);
    if (block_match_only) return 0;
    f3d_initial_info found = {};
    if (!optical_flow_e.SetInitialFromNodes(nullptr, &found)) {
      std::printf("Error: %s\n", optical_flow_e.InitialFlowError().c_str());
      return 3;
    }
    say_initial(found);
    return 0;
  };

  // --subset-match: the node table of the resident pair, measured beside the flow the driver holds, into <tag>_subset.csv, and one
  // line about it
  auto subset_of_pair = [&](size_t k) {
    f3d_subset_match_summary sum = {};
    if (!optical_flow_e.SubsetMatch(subset_params, nullptr, &sum)) {
      std::printf("Error: %s\n", optical_flow_e.InitialFlowError().c_str());
      return 3;
    }
    const std::string tag = pairs > 1 ? prefix + "_" + std::to_string(k) : prefix;
    std::FILE* csv = std::fopen((tag + "_subset.csv").c_str(), "w");
    if (!csv) {
      std::printf("Error: cannot write %s_subset.csv\n", tag.c_str());
      return 2;
    }
    static const char* const kStatus[] = {"ok", "nan", "flat", "flat_target", "singular", "outside", "lost", "not_converged", "no_start", "low"};
    std::fprintf(csv, "x,y,z,status,iterations,zncc,u,v,w,ux,uy,uz,vx,vy,vz,wx,wy,wz,diff_u,diff_v,diff_w\n");
    for (const f3d_subset_match_node& r : optical_flow_e.SubsetMatchNodes()) {
      std::fprintf(csv, "%d,%d,%d,%s,%d,%.17g,%.9g,%.9g,%.9g", r.position[0], r.position[1], r.position[2], kStatus[r.status], r.iterations, r.zncc,
                   r.u, r.v, r.w);
      for (float g : r.grad) std::fprintf(csv, ",%.9g", g);
      std::fprintf(csv, ",%.9g,%.9g,%.9g\n", r.diff[0], r.diff[1], r.diff[2]);
    }
    std::fclose(csv);
    std::printf("subset match: %llu nodes", sum.nodes);
    for (int s = 0; s < F3D_SUBSET_NODE_STATUS_COUNT; ++s) std::printf(", %llu %s", sum.status[s], kStatus[s]);
    std::printf(", median zncc %.4f, |flow - subset| over %llu nodes: rms %.4f, median %.4f, p95 %.4f\n", sum.median_zncc, sum.compared, sum.rms,
                sum.median, sum.p95);
    return 0;
  };

  if (pairs == 1) {
    if (!synthetic && !load(frame_1, files[1])) return 2;
    optical_flow_e.UploadResidentFrames(frame_0, frame_1);
    if (initial_given)
      if (const int status = initial_from_files()) return status;
    if (block_match) {
      if (const int status = initial_from_block_match(0)) return status;
      if (block_match_only) {
        optical_flow_e.Destroy();
        f3d_host_shutdown();
        return 0;
      }
    }
    const bool from_guess = initial_given || block_match;
    // (a plain solve that cannot run goes on as it always did; one that was to start from the displacement says why and ends)
    if (!optical_flow_e.ComputeFlowResident(params, from_guess) && from_guess) return 3;
    if (print_stats) report();
    if (segment || histogram)
      if (const int status = segment_frame_0()) return status;
    if (const int status = stats_of_frame_0()) return status;
    optical_flow_e.DownloadFlow(flow_u, flow_v, flow_w);
    write_pair(0, flow_u, flow_v, flow_w);
    if (subset_match)
      if (const int status = subset_of_pair(0)) return status;
    if (cumulative) {
      if (!optical_flow_e.ResetTrajectory() || !optical_flow_e.ComposeTrajectory() ||
          !optical_flow_e.DownloadTrajectory(disp[0], disp[1], disp[2], nullptr))
        return 3;
      write_disp(0);
    }
    for (DerivedField* fp : order) {
      DerivedField& f = *fp;
      if (!f.fields) continue;
      if (!f.compute(cumulative && !f.of_pair ? OpticalFlowE::Trajectory() : OpticalFlowE::HeldFlow()) ||
          !optical_flow_e.DownloadDerived(f.which, f.out, f.fields))
        return 3;
      write_derived(f, 0);
    }
    if (const int status = stats_of_pair(0)) return status;
    if (contacts) {
      if (!compute_contacts(cumulative ? OpticalFlowE::Trajectory() : OpticalFlowE::HeldFlow())) return 3;
      write_contacts(0);
    }
    if (track)
      if (const int status = track_pair(0, cumulative ? OpticalFlowE::Trajectory() : OpticalFlowE::HeldFlow())) return status;
  } else {
    // Sequence: pair k solves on the device while the host reads frame k+2 and uploads it on one copy queue, and downloads and
    // writes the flow of pair k-1 on another -- from and to page-locked buffers (the reference's ALLOCATE_PINNED_MEMORY switch,
    // data3d.cpp:30,57-61), so the copies really run beside the kernels.  A frame crosses the link once although it serves two
    // pairs.  With --stats or without --silent the driver reads results back per level, which serialises the solve with the
    // host; the copies still overlap.
    if (!optical_flow_e.AllocateSequenceFrames()) return 3;
    const DataSize4& c = optical_flow_e.ContainerSize();
    Data3D host_frame[3], host_flow[2][3];
    std::vector<void*> pinned;
    // (volumes of 32 MiB and more only: smaller ones live in the allocator's shared heap, see OpticalFlowP::ComputeFlow)
    auto pin = [&](Data3D& v) {
      const size_t bytes = width * height * depth * sizeof(float);
      if (bytes >= (static_cast<size_t>(32) << 20) && f3d_host_register(v.DataPtr(), bytes) == 0) pinned.push_back(v.DataPtr());
    };
    for (Data3D& f : host_frame)
      if (!f.Allocate(width, height, depth)) return 2;
    for (auto& set : host_flow)
      for (Data3D& f : set)
        if (!f.Allocate(width, height, depth)) return 2;
    for (Data3D& f : host_frame) pin(f);
    for (auto& set : host_flow)
      for (Data3D& f : set) pin(f);
    if (cumulative)
      for (Data3D& d : disp) pin(d);
    for (DerivedField& f : derived)
      for (Data3D* d : f.out)
        if (d) pin(*d);
    f3d_queue up = nullptr, down = nullptr;
    f3d_event uploaded[3] = {nullptr, nullptr, nullptr};
    if (CheckDeviceError(f3d_queue_create(&up)) || CheckDeviceError(f3d_queue_create(&down))) return 3;
    for (f3d_event& e : uploaded)
      if (CheckDeviceError(f3d_event_create(&e))) return 3;
    // The slot of a frame.  Consecutive pairs: frame index mod 3.  --total: frame 0 keeps slot 0 for the whole sequence and frame
    // i >= 1 takes slot 1 + (i - 1) % 2, so that the upload of frame k+2 beside solve k (frames 0 and k+1) goes into the slot of frame k.
    auto slot_of = [&](size_t frame_index) {
      return static_cast<int>(total ? (frame_index == 0 ? 0 : 1 + (frame_index - 1) % 2) : frame_index % 3);
    };
    auto upload = [&](size_t frame_index) {  // file -> page-locked buffer -> device container
      const int slot = slot_of(frame_index);
      if (!load(host_frame[slot], files[frame_index])) return false;
      CheckDeviceError(f3d_copy_planes_h2d_on(up, optical_flow_e.SequenceFrame(slot), c.pitch, c.height, 0, host_frame[slot].DataPtr(),
                                              width, height, width, height, depth));
      CheckDeviceError(f3d_event_record_on(uploaded[slot], up));
      return true;
    };
    if (!upload(0) || !upload(1)) return 2;
    // --cumulative: displacement k is composed on the library stream after pair k and goes down on `down` beside the next solve.
    // Two device-side dependencies: the download of displacement k waits for compose k (`composed`), and compose k+1, which
    // rewrites the same containers in place, waits for that download to finish (`disp_down`).
    f3d_event composed = nullptr, disp_down = nullptr;
    if (cumulative) {
      if (CheckDeviceError(f3d_event_create(&composed)) || CheckDeviceError(f3d_event_create(&disp_down))) return 3;
      if (!optical_flow_e.ResetTrajectory()) return 3;
    }
    // --strain, --principal, --rotation, --inverse: the same pattern for each one's containers.  The kernel of pair k runs on the library
    // stream right after compose k (or after TakeResult); its statistics wait for that kernel only.  The fields go down on `down` beside
    // solve k+1 once the kernel is done (`done`), and the kernel of pair k+1, which rewrites the same containers, waits for that
    // download (`down`).
    // --match is the one reader of the frame containers after the solve: match k reads the frames of pair k, and the upload of frame k+3
    // on `up`, issued right after solve k+1 is enqueued, overwrites frame k's slot.  The host wait of EndComputeFlowResident and of
    // the statistics happens to order the two; the order is made explicit all the same: `up` waits for match k (`done`) before it
    // reuses the slot.
    DerivedField& match = derived[3];
    for (DerivedField& f : derived)
      if (f.fields)
        if (CheckDeviceError(f3d_event_create(&f.done)) || CheckDeviceError(f3d_event_create(&f.down))) return 3;
    DevicePtr taken[3] = {0, 0, 0};
    bool pending_output = false;
    const bool serial_sequence = std::getenv("F3D_SEQ_SERIAL") && std::atoi(std::getenv("F3D_SEQ_SERIAL")) != 0;
    // --total: everything pair k-1 enqueued on the library stream that may read frame k in its slot (the match, the second label volume
    // of --track) is behind `pair_read`; `up` waits for it before frame k+2 goes into that slot.  (The host waits of the statistics and
    // of the overlap happen to order the two already; the order is made explicit all the same, as for --match.)
    f3d_event pair_read = nullptr;
    if (total && CheckDeviceError(f3d_event_create(&pair_read))) return 3;
    for (size_t k = 0; k < pairs; ++k) {
      // pair k is frame k -> frame k+1, or with --total frame 0 -> frame k+1
      const size_t first = total ? 0 : k;
      // the solve of pair k waits (on the device) for the uploads of its two frames
      CheckDeviceError(f3d_queue_wait_event(nullptr, uploaded[slot_of(first)]));
      CheckDeviceError(f3d_queue_wait_event(nullptr, uploaded[slot_of(k + 1)]));
      optical_flow_e.SelectResidentPair(slot_of(first), slot_of(k + 1));
      // what the pair starts from: the files for pair 0; the flow of pair k-1 for a later pair of --warm-start (as it stands) and of
      // --total (frame 0 -> frame k).  `taken` still holds that flow: it goes back to the pool further down, beside this solve.
      bool from_initial = false;
      if (k == 0 && initial_given) {
        if (const int status = initial_from_files()) return status;
        from_initial = true;
      } else if (block_match) {
        if (const int status = initial_from_block_match(k)) return status;
        from_initial = true;
      } else if (k > 0 && (total || warm_start)) {
        f3d_initial_info found = {};
        if (!optical_flow_e.SetInitialFlow(OpticalFlowE::Containers(taken), &found)) {
          std::printf("Error: %s\n", optical_flow_e.InitialFlowError().c_str());
          return 3;
        }
        say_initial(found);
        from_initial = true;
      }
      if (!optical_flow_e.BeginComputeFlowResident(params, from_initial) && from_initial) return 3;  // the plain path goes on as before
      if (serial_sequence) optical_flow_e.EndComputeFlowResident();  // A/B timing: nothing runs beside the solve
      // beside it: frame k+2 into the container pair k-1 has released, and the previous pair's flow out to its files
      if (match.fields && k > 0) CheckDeviceError(f3d_queue_wait_event(up, match.done));  // match k-1 read the slot of frame k+2
      if (total && k > 0) CheckDeviceError(f3d_queue_wait_event(up, pair_read));          // so did whatever else pair k-1 ran on frame k
      if (k + 2 <= pairs && !upload(k + 2)) return 2;
      if (pending_output) {
        CheckDeviceError(f3d_queue_sync(down));
        optical_flow_e.GiveResultBack(taken);
        write_pair(k - 1, host_flow[(k - 1) & 1][0], host_flow[(k - 1) & 1][1], host_flow[(k - 1) & 1][2]);
        if (cumulative) write_disp(k - 1);
        for (DerivedField* f : order)
          if (f->fields) write_derived(*f, k - 1);
        if (contacts) write_contacts(k - 1);
        pending_output = false;
      }
      optical_flow_e.EndComputeFlowResident();
      // frame 0 is still in its container: frame 3 overwrites it only beside the solve of pair 1, and with --total nothing ever does
      if ((segment || histogram) && k == 0)
        if (const int status = segment_frame_0()) return status;
      if (k == 0)
        if (const int status = stats_of_frame_0()) return status;
      if (print_stats) report();
      std::printf("pair %zu of %zu: %.3f s on the device\n", k + 1, pairs, optical_flow_e.LastDeviceSeconds());
      // the driver still holds the flow and the pair's two frames stay in their slots: the upload beside this solve went elsewhere
      if (subset_match)
        if (const int status = subset_of_pair(k)) return status;
      if (!optical_flow_e.TakeResult(taken)) return 3;
      for (int i = 0; i < 3; ++i)
        CheckDeviceError(f3d_copy_planes_d2h_on(down, host_flow[k & 1][i].DataPtr(), width, height, width, height, depth, taken[i],
                                                c.pitch, c.height, 0));
      if (cumulative) {
        if (k > 0) CheckDeviceError(f3d_queue_wait_event(nullptr, disp_down));
        if (!optical_flow_e.ComposeTrajectory(taken)) return 3;
        CheckDeviceError(f3d_event_record(composed));
        CheckDeviceError(f3d_queue_wait_event(down, composed));
        for (int i = 0; i < 3; ++i)
          CheckDeviceError(f3d_copy_planes_d2h_on(down, disp[i].DataPtr(), width, height, width, height, depth,
                                                  optical_flow_e.TrajectoryContainer(i), c.pitch, c.height, 0));
        CheckDeviceError(f3d_event_record_on(disp_down, down));
      }
      for (DerivedField* fp : order) {
        DerivedField& f = *fp;
        if (!f.fields) continue;
        if (k > 0) CheckDeviceError(f3d_queue_wait_event(nullptr, f.down));
        if (!f.compute(cumulative && !f.of_pair ? OpticalFlowE::Trajectory() : OpticalFlowE::Containers(taken))) return 3;
        CheckDeviceError(f3d_event_record(f.done));
        CheckDeviceError(f3d_queue_wait_event(down, f.done));
        for (int i = 0; i < OpticalFlowE::DerivedFieldCount(f.which); ++i)
          if (f.out[i])
            CheckDeviceError(f3d_copy_planes_d2h_on(down, f.host[i].DataPtr(), width, height, width, height, depth,
                                                    optical_flow_e.DerivedContainer(f.which, i), c.pitch, c.height, 0));
        CheckDeviceError(f3d_event_record_on(f.down, down));
      }
      if (const int status = stats_of_pair(k)) return status;  // waits for the fields of pair k, which stay until pair k+1 rewrites them
      if (contacts && !compute_contacts(cumulative ? OpticalFlowE::Trajectory() : OpticalFlowE::Containers(taken))) return 3;
      // frame k+1 stays in its container until the upload of frame k+4, two solves from here; with --total until the upload of frame
      // k+3 beside the next solve, which waits for `pair_read`
      if (track)
        if (const int status = track_pair(k, cumulative ? OpticalFlowE::Trajectory() : OpticalFlowE::Containers(taken))) return status;
      if (total) CheckDeviceError(f3d_event_record(pair_read));
      pending_output = true;
    }
    if (pair_read) f3d_event_destroy(pair_read);
    CheckDeviceError(f3d_queue_sync(down));
    optical_flow_e.GiveResultBack(taken);
    write_pair(pairs - 1, host_flow[(pairs - 1) & 1][0], host_flow[(pairs - 1) & 1][1], host_flow[(pairs - 1) & 1][2]);
    if (cumulative) {
      write_disp(pairs - 1);
      f3d_event_destroy(composed);
      f3d_event_destroy(disp_down);
    }
    for (DerivedField* fp : order) {
      DerivedField& f = *fp;
      if (!f.fields) continue;
      write_derived(f, pairs - 1);
      f3d_event_destroy(f.done);
      f3d_event_destroy(f.down);
    }
    if (contacts) write_contacts(pairs - 1);
    CheckDeviceError(f3d_queue_sync(up));
    for (f3d_event e : uploaded) f3d_event_destroy(e);
    f3d_queue_destroy(up);
    f3d_queue_destroy(down);
    for (void* p : pinned) f3d_host_unregister(p);
  }

  optical_flow_e.Destroy();
  f3d_host_shutdown();
  return label_table_failed ? 2 : 0;
}
