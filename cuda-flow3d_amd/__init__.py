"""cuda-flow3d_amd -- Python binding of the MI355X-native 3-D optical-flow solver.

The product is native: libf3d_hip.so (hand-written gfx950 kernels behind the C ABI of include/f3d.h) and
libf3d_host.so (the C++ driver / operator classes that mirror the reference's src/optical_flow and
src/cuda_operations, C ABI in include/f3d_host.h).  This module only binds those two libraries with ctypes
and moves numpy volumes ([z, y, x], float32, x fastest like the reference's Data3D) across the boundary.
There is no Python or CPU implementation of any kernel here: if the libraries are missing, importing the
native handles raises -- build them with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C cuda-flow3d_amd`.
"""
import atexit
import collections
import contextlib
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBDIR = os.environ.get("F3D_LIBDIR") or os.path.join(_HERE, "lib")  # F3D_LIBDIR: A/B timing of two builds in one GPU call

DEFAULT_PARAMS = dict(
    warp_levels_count=40, warp_scale_factor=0.95, outer_iterations_count=40, inner_iterations_count=5,
    equation_alpha=7.5, equation_smoothness=0.001, equation_data=0.001, median_radius=5, gaussian_sigma=2.0,
)  # src/main.cpp:77-85


class F3dError(RuntimeError):
    pass


class Size4(C.Structure):  # DataSize4 / f3d_size4
    _fields_ = [("width", C.c_size_t), ("height", C.c_size_t), ("depth", C.c_size_t), ("pitch", C.c_size_t)]


class Slab(C.Structure):  # f3d_slab
    _fields_ = [("z_base", C.c_int), ("z_lo", C.c_int), ("z_hi", C.c_int)]


class LevelStat(C.Structure):  # f3d_level_stat
    _fields_ = [("level", C.c_int), ("width", C.c_size_t), ("height", C.c_size_t), ("depth", C.c_size_t),
                ("residual_rms", C.c_double), ("residual_mean_abs", C.c_double), ("residual_max_abs", C.c_float),
                ("flow_min", C.c_float), ("flow_max", C.c_float), ("flow_avg", C.c_float)]


class StrainStats(C.Structure):  # f3d_strain_stats
    _fields_ = [("defined", C.c_ulonglong), ("folded", C.c_ulonglong), ("vol_min", C.c_float), ("vol_max", C.c_float),
                ("eq_max", C.c_float), ("vol_sum", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class WindowStrainStats(C.Structure):  # f3d_window_strain_stats
    _fields_ = [("defined", C.c_ulonglong), ("folded", C.c_ulonglong), ("lost", C.c_ulonglong), ("thin", C.c_ulonglong),
                ("vol_min", C.c_float), ("vol_max", C.c_float), ("eq_max", C.c_float), ("vol_sum", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PrincipalStats(C.Structure):  # f3d_principal_stats
    _fields_ = [("defined", C.c_ulonglong), ("e1_max", C.c_float), ("e3_min", C.c_float), ("shear_max", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PolarStats(C.Structure):  # f3d_polar_stats
    _fields_ = [("defined", C.c_ulonglong), ("folded", C.c_ulonglong), ("theta_max", C.c_float), ("l1_max", C.c_float),
                ("l3_min", C.c_float), ("theta_sum", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class InverseStats(C.Structure):  # f3d_inverse_stats
    _fields_ = [("defined", C.c_ulonglong), ("unconverged", C.c_ulonglong), ("steps_sum", C.c_ulonglong), ("err_max", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class CorrelationStats(C.Structure):  # f3d_correlation_stats
    _fields_ = [("defined", C.c_ulonglong), ("lost", C.c_ulonglong), ("below", C.c_ulonglong), ("zncc_min", C.c_float),
                ("rmsd_max", C.c_float), ("zncc_sum", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class MotionSums(C.Structure):  # struct f3d_motion_sums
    _fields_ = [("n", C.c_ulonglong), ("Sx", C.c_double * 3), ("Sxx", C.c_double * 6), ("Sd", C.c_double * 3),
                ("Sxd", C.c_double * 9), ("Sdd", C.c_double * 3)]

    def as_dict(self):
        return {name: (getattr(self, name) if name == "n" else list(getattr(self, name))) for name, _ in self._fields_}


class MotionFit(C.Structure):  # f3d_motion_fit: d_fit(x) = t + M (x - centre)
    _fields_ = [("centre", C.c_double * 3), ("t", C.c_double * 3), ("M", C.c_double * 9), ("n", C.c_ulonglong),
                ("rms_before", C.c_double), ("cos_angle", C.c_double), ("axial", C.c_double * 3), ("model", C.c_int)]

    @property
    def matrix(self):
        """M as a 3 x 3 array: row = component u, v, w; column = coordinate x, y, z"""
        return np.array(list(self.M), np.float64).reshape(3, 3)

    def as_dict(self):
        return {"centre": list(self.centre), "t": list(self.t), "matrix": self.matrix.tolist(), "n": self.n,
                "rms_before": self.rms_before, "cos_angle": self.cos_angle, "axial": list(self.axial),
                "model": {v: k for k, v in MOTION_MODELS.items()}.get(self.model, self.model)}


class MotionResidual(C.Structure):  # f3d_motion_residual
    _fields_ = [("present", C.c_ulonglong), ("sum_sq", C.c_double), ("max_abs", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LabelInfo(C.Structure):  # f3d_label_info: every voxel of the volume in exactly one counter
    _fields_ = [("background", C.c_ulonglong), ("foreign", C.c_ulonglong), ("absent", C.c_ulonglong), ("out_of_range", C.c_ulonglong),
                ("used", C.c_ulonglong)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class Contact(C.Structure):  # struct f3d_contact: the exact sums of one unordered pair of labels
    _fields_ = [("lo", C.c_int), ("hi", C.c_int), ("faces", C.c_ulonglong * 3), ("area", C.c_longlong * 3), ("c2", C.c_longlong * 3),
                ("n_jump", C.c_ulonglong), ("J", C.c_longlong * 3)]


class ContactInfo(C.Structure):  # f3d_contact_info: every face of the volume in exactly one of the first five counters
    _fields_ = [("foreign", C.c_ulonglong), ("background", C.c_ulonglong), ("surface", C.c_ulonglong), ("interior", C.c_ulonglong),
                ("contact", C.c_ulonglong), ("jump_absent", C.c_ulonglong), ("lost", C.c_ulonglong), ("n_contacts", C.c_ulonglong),
                ("complete", C.c_int)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LabelShapeSums(C.Structure):  # struct f3d_label_shape_sums: the 36 exact sums of one label
    _fields_ = [("n", C.c_ulonglong), ("lo", C.c_longlong * 3), ("hi", C.c_longlong * 3), ("s1", C.c_ulonglong * 3),
                ("s2", C.c_ulonglong * 6), ("pairs", C.c_ulonglong * 13), ("squares", C.c_ulonglong * 3), ("cubes", C.c_ulonglong),
                ("border", C.c_ulonglong * 3)]


class LabelShapeInfo(C.Structure):  # f3d_label_shape_info: every voxel of the box in exactly one counter
    _fields_ = [("background", C.c_ulonglong), ("foreign", C.c_ulonglong), ("labelled", C.c_ulonglong)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LabelShape(C.Structure):  # f3d_label_shape
    _fields_ = [("status", C.c_int), ("voxels", C.c_ulonglong), ("box_lo", C.c_longlong * 3), ("box_hi", C.c_longlong * 3),
                ("border", C.c_ulonglong * 3), ("centroid", C.c_double * 3), ("diameter", C.c_double), ("semi_axes", C.c_double * 3),
                ("axes", C.c_double * 9), ("faces", C.c_ulonglong), ("surface", C.c_double), ("sphericity", C.c_double),
                ("euler", C.c_longlong)]


class LabelFieldSumsRow(C.Structure):  # struct f3d_label_field_sums: the eight exact words of one label
    _fields_ = [("n", C.c_ulonglong), ("min_key", C.c_ulonglong), ("max_key", C.c_ulonglong), ("iq", C.c_longlong),
                ("iqq_lo", C.c_ulonglong), ("iqq_hi", C.c_ulonglong), ("below", C.c_ulonglong), ("above", C.c_ulonglong)]


class LabelFieldInfo(C.Structure):  # f3d_label_field_info: every voxel of the box in exactly one counter, tried in this order
    _fields_ = [(k, C.c_ulonglong) for k in ("background", "foreign", "nan", "out_of_range", "used")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class LabelFieldStat(C.Structure):  # f3d_label_field_stat
    _fields_ = [("status", C.c_int), ("q05_bin", C.c_int), ("median_bin", C.c_int), ("q95_bin", C.c_int), ("n", C.c_ulonglong),
                ("below", C.c_ulonglong), ("above", C.c_ulonglong)] + \
               [(k, C.c_double) for k in ("min", "max", "mean", "variance", "std", "q05", "median", "q95")]


class LabelFieldSummary(C.Structure):  # f3d_label_field_summary
    _fields_ = [("ok", C.c_ulonglong), ("empty", C.c_ulonglong), ("small", C.c_ulonglong), ("mean", C.c_double)]


class Overlap(C.Structure):  # struct f3d_overlap: the exact sums of one pair (label of A, label of B)
    _fields_ = [("a", C.c_int), ("b", C.c_int), ("n", C.c_ulonglong), ("ca2", C.c_longlong * 3), ("cb2", C.c_longlong * 3)]


class OverlapInfo(C.Structure):  # f3d_overlap_info: every voxel of the volume in exactly one of the first six counters
    _fields_ = [(name, C.c_ulonglong) for name in ("foreign_a", "lost_background", "lost_body", "foreign_b", "background", "overlap",
                                                   "table_lost", "n_pairs")] + [("complete", C.c_int)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrackA(C.Structure):  # f3d_track_a
    _fields_ = [("n", C.c_ulonglong), ("n_lost", C.c_ulonglong), ("n_background", C.c_ulonglong), ("n_best", C.c_ulonglong),
                ("best_b", C.c_int), ("n_targets", C.c_int), ("fraction", C.c_double), ("shift", C.c_double * 3), ("iou", C.c_double),
                ("status", C.c_uint)]


class TrackB(C.Structure):  # f3d_track_b
    _fields_ = [("m", C.c_ulonglong), ("n_unreached", C.c_ulonglong), ("n_best", C.c_ulonglong), ("best_a", C.c_int),
                ("n_sources", C.c_int), ("status", C.c_uint)]


class TrackSummary(C.Structure):  # f3d_track_summary
    _fields_ = [(name, C.c_ulonglong) for name in ("matched", "split", "merged", "vanished", "appeared", "left", "n_ids")]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class ComponentInfo(C.Structure):  # f3d_component_info: every voxel of the box in exactly one of foreground and background
    _fields_ = [(name, C.c_ulonglong) for name in ("foreground", "background", "nan", "n_components", "n_labels", "dropped_components",
                                                   "dropped_voxels", "largest")]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class SplitInfo(C.Structure):  # f3d_split_info: f3d_component_info of the final classes, then what the split found on the way
    _fields_ = [(name, C.c_ulonglong) for name in ("foreground", "background", "nan", "n_components", "n_labels", "dropped_components",
                                                   "dropped_voxels", "largest", "connected_components", "core_voxels", "n_cores",
                                                   "remainder_bodies", "remainder_voxels")]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class HistogramInfo(C.Structure):  # f3d_histogram_info: every voxel of the volume in exactly one counter, tried in this order
    _fields_ = [(name, C.c_ulonglong) for name in ("masked", "nan", "below", "above", "used")]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class RangeInfo(C.Structure):  # f3d_range_info: every voxel of the volume in exactly one counter, tried in this order
    _fields_ = [(name, C.c_ulonglong) for name in ("masked", "nan", "infinite", "finite")]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class OtsuInfo(C.Structure):  # f3d_otsu_info
    _fields_ = [("status", C.c_int), ("populations", C.c_ulonglong * 3), ("objective", C.c_double)]


class NearestInfo(C.Structure):  # f3d_nearest_info
    _fields_ = [(name, C.c_ulonglong) for name in ("seeds", "d2_max", "unreached")]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class ContactKinematics(C.Structure):  # f3d_contact_kin
    _fields_ = [("point", C.c_double * 3), ("area", C.c_double), ("normal", C.c_double * 3), ("jump_normal", C.c_double),
                ("jump_slip", C.c_double), ("fit_normal", C.c_double), ("fit_slip", C.c_double), ("status", C.c_uint)]


class ValidateStats(C.Structure):  # f3d_validate_stats
    _fields_ = [("present", C.c_ulonglong), ("tested", C.c_ulonglong), ("outliers", C.c_ulonglong), ("replaced", C.c_ulonglong),
                ("undefined", C.c_ulonglong), ("r_max", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class InitialInfo(C.Structure):  # f3d_initial_info: what f3d_initial_flow found in a displacement a solve is to start from
    _fields_ = [("voxels", C.c_ulonglong), ("replaced", C.c_ulonglong), ("leaving", C.c_ulonglong), ("max_abs", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BlockMatchGrid(C.Structure):  # f3d_block_match_grid (include/f3d_block_match.h)
    _fields_ = [("ox", C.c_int), ("oy", C.c_int), ("oz", C.c_int), ("step", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("window", C.c_int), ("rx", C.c_int), ("ry", C.c_int), ("rz", C.c_int)]


class BlockMatchInfo(C.Structure):  # f3d_block_match_info
    _fields_ = [("nodes", C.c_ulonglong), ("ok", C.c_ulonglong), ("flat_nodes", C.c_ulonglong), ("none_nodes", C.c_ulonglong),
                ("evaluated", C.c_ulonglong), ("outside", C.c_ulonglong), ("flat", C.c_ulonglong), ("nan", C.c_ulonglong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BlockMatchSummary(C.Structure):  # f3d_block_match_summary
    _fields_ = [("nodes", C.c_ulonglong), ("ok", C.c_ulonglong), ("flat", C.c_ulonglong), ("none", C.c_ulonglong),
                ("low", C.c_ulonglong), ("edge", C.c_ulonglong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# f3d_block_match_record as 32 int32 per node, and f3d_block_match_node as a numpy record
BLOCK_MATCH_RECORD_WORDS = 32
BLOCK_MATCH_NODE = np.dtype([("position", np.int32, 3), ("shift", np.int32, 3), ("status", np.int32), ("evaluated", np.int32),
                             ("outside", np.int32), ("flat", np.int32), ("zncc", np.float64), ("offset", np.float64, 3),
                             ("u", np.float32), ("v", np.float32), ("w", np.float32), ("reserved", np.int32)])
BLOCK_NODE_STATUS = ("ok", "flat", "none", "low", "edge")


class SubsetGrid(C.Structure):  # f3d_subset_match_grid (include/f3d_subset_match.h)
    _fields_ = [("ox", C.c_int), ("oy", C.c_int), ("oz", C.c_int), ("step", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("window", C.c_int)]


class SubsetInfo(C.Structure):  # f3d_subset_match_info
    _fields_ = [("nodes", C.c_ulonglong), ("status", C.c_ulonglong * 9), ("iterations", C.c_ulonglong), ("nan", C.c_ulonglong)]

    def as_dict(self):
        return dict(nodes=self.nodes, status=list(self.status), iterations=self.iterations, nan=self.nan)


class SubsetSummary(C.Structure):  # f3d_subset_match_summary (include/f3d_host.h)
    _fields_ = [("nodes", C.c_ulonglong), ("status", C.c_ulonglong * 10), ("compared", C.c_ulonglong), ("median_zncc", C.c_double),
                ("rms", C.c_double), ("median", C.c_double), ("p95", C.c_double)]

    def as_dict(self):
        return dict(nodes=self.nodes, status=list(self.status), compared=self.compared, median_zncc=self.median_zncc, rms=self.rms,
                    median=self.median, p95=self.p95)


# f3d_subset_match_record and f3d_subset_match_node as numpy records
SUBSET_RECORD = np.dtype([("p", np.float64, 12), ("zncc", np.float64), ("step", np.float64), ("df", np.float64), ("dg", np.float64),
                          ("status", np.int32), ("iterations", np.int32), ("nan", np.int32), ("reserved", np.int32)])
SUBSET_NODE = np.dtype([("position", np.int32, 3), ("status", np.int32), ("iterations", np.int32), ("reserved", np.int32),
                        ("zncc", np.float64), ("u", np.float32), ("v", np.float32), ("w", np.float32), ("grad", np.float32, 9),
                        ("diff", np.float32, 3), ("reserved2", np.int32)])
SUBSET_STATUS = ("ok", "nan", "flat", "flat_target", "singular", "outside", "lost", "not_converged", "no_start", "low")
SUBSET_MODELS = {"translation": 0, "affine": 1}


class FlowParams(C.Structure):  # f3d_flow_params
    _fields_ = [
        ("warp_levels_count", C.c_size_t), ("warp_scale_factor", C.c_float),
        ("outer_iterations_count", C.c_size_t), ("inner_iterations_count", C.c_size_t),
        ("equation_alpha", C.c_float), ("equation_smoothness", C.c_float), ("equation_data", C.c_float),
        ("median_radius", C.c_size_t), ("gaussian_sigma", C.c_float),
    ]


_hip = None
_host = None
_fp = C.POINTER(C.c_float)
_dp = C.c_uint64
_dpp = C.POINTER(C.c_uint64)
_sz = C.c_size_t
_slabp = C.POINTER(Slab)


def _load(name):
    path = os.path.join(_LIBDIR, name)
    if not os.path.exists(path):
        raise F3dError(f"{path} is missing: the HIP extension has not been built (make -C {_HERE}); "
                       "there is no fallback path")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def hip():
    """Handle of libf3d_hip.so with argument types declared (include/f3d.h)."""
    global _hip
    if _hip is not None:
        return _hip
    L = _load("libf3d_hip.so")
    L.f3d_last_error.restype = C.c_char_p
    sig = {
        "f3d_init": [C.c_int], "f3d_shutdown": [], "f3d_is_initialized": [], "f3d_device_count": [C.POINTER(C.c_int)],
        "f3d_crash_maps_enable": [C.c_char_p],
        "f3d_lane_create": [C.POINTER(C.c_void_p)], "f3d_lane_make_current": [C.c_void_p], "f3d_lane_is_private": [], "f3d_lane_get_current": [C.POINTER(C.c_void_p)],
        "f3d_lane_destroy": [C.c_void_p],
        "f3d_selftest_weights": [C.c_uint, C.c_uint, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                 C.POINTER(C.c_uint)],
        "f3d_device_name": [C.c_char_p, _sz], "f3d_mem_info": [C.POINTER(_sz), C.POINTER(_sz)],
        "f3d_lds_per_workgroup": [C.POINTER(C.c_int)],
        "f3d_alloc_pitched": [C.POINTER(_dp), C.POINTER(_sz), _sz, _sz], "f3d_free": [_dp],
        "f3d_memset2d": [_dp, _sz, C.c_int, _sz, _sz],
        "f3d_copy3d_h2d": [_dp, _sz, _sz, _sz, _fp, _sz, _sz, _sz],
        "f3d_copy3d_d2h": [_fp, _sz, _sz, _sz, _dp, _sz, _sz, _sz],
        "f3d_copy_planes_h2d": [_dp, _sz, _sz, _sz, _fp, _sz, _sz, _sz, _sz, _sz],
        "f3d_copy_planes_d2h": [_fp, _sz, _sz, _sz, _sz, _sz, _dp, _sz, _sz, _sz],
        "f3d_queue_create": [C.POINTER(C.c_void_p)], "f3d_queue_destroy": [C.c_void_p], "f3d_queue_sync": [C.c_void_p],
        "f3d_event_record_on": [C.c_void_p, C.c_void_p], "f3d_queue_wait_event": [C.c_void_p, C.c_void_p],
        "f3d_copy_planes_h2d_on": [C.c_void_p, _dp, _sz, _sz, _sz, _fp, _sz, _sz, _sz, _sz, _sz],
        "f3d_copy_planes_d2h_on": [C.c_void_p, _fp, _sz, _sz, _sz, _sz, _sz, _dp, _sz, _sz, _sz],
        "f3d_copy_rect_d2d": [_dp, _sz, _sz, _sz, _dp, _sz, _sz, _sz, _sz, _sz, _sz],
        "f3d_host_register": [C.c_void_p, _sz], "f3d_host_unregister": [C.c_void_p],
        "f3d_host_is_pinned": [C.c_void_p, C.POINTER(C.c_int)],
        "f3d_copy_d2d": [_dp, _dp, _sz], "f3d_set_container": [C.POINTER(Size4)], "f3d_get_container": [C.POINTER(Size4)],
        "f3d_event_create": [C.POINTER(C.c_void_p)], "f3d_event_record": [C.c_void_p],
        "f3d_event_sync": [C.c_void_p], "f3d_event_elapsed_ms": [_fp, C.c_void_p, C.c_void_p],
        "f3d_event_destroy": [C.c_void_p], "f3d_stream_sync": [],
        "f3d_phi_ksi": [_dp] * 8 + [_sz] * 3 + [C.c_float] * 5 + [_dp, _dp, _slabp],
        "f3d_phi_ksi_zones": [_dp] * 8 + [_sz] * 3 + [C.c_float] * 5 + [_dp, _dp, _slabp, _slabp],
        "f3d_solve_sweep": [_dp] * 10 + [_sz] * 3 + [C.c_float] * 4 + [_dp] * 3 + [_slabp],
        "f3d_solve_sweep2": [_dp] * 10 + [_sz] * 3 + [C.c_float] * 4 + [_dp] * 3 + [_slabp],
        "f3d_solve_sweep_phi_ksi": [_dp] * 10 + [_sz] * 3 + [C.c_float] * 6 + [_dp] * 5 + [_slabp],
        "f3d_solve_sweep_phi_ksi_edges": [_dp] * 10 + [_sz] * 3 + [C.c_float] * 6 + [_dp] * 5 + [_slabp, C.c_int, C.c_int],
        "f3d_frame_derivatives": [_dp, _dp, _sz, _sz, _sz, C.c_float, C.c_float, C.c_float, _dp, _dp, _dp, _dp, _slabp],
        "f3d_solve_sweep_phi_ksi_edges_fd": [_dp] * 12 + [_sz] * 3 + [C.c_float] * 6 + [_dp] * 5 + [_slabp, C.c_int, C.c_int],
        "f3d_solve_sweep2_fd": [_dp] * 12 + [_sz] * 3 + [C.c_float] * 4 + [_dp] * 3 + [_slabp],
        "f3d_fused_launches_march_along_y": [_sz, _sz, _sz],
        "f3d_solve_sweep3": [_dp] * 10 + [_sz] * 3 + [C.c_float] * 4 + [_dp] * 3 + [_slabp],
        "f3d_solve_sweep2_phi_ksi": [_dp] * 10 + [_sz] * 3 + [C.c_float] * 6 + [_dp] * 5 + [_slabp],
        "f3d_solve_sweep_phi_ksi_fd": [_dp] * 12 + [_sz] * 3 + [C.c_float] * 6 + [_dp] * 5 + [_slabp],
        "f3d_warp": [_dp] * 5 + [_sz] * 3 + [C.c_float] * 3 + [_dp, _slabp],
        "f3d_resample_x": [_dp, _dp, _sz, _sz, _sz, _sz, _slabp],
        "f3d_resample_y": [_dp, _dp, _sz, _sz, _sz, _sz, _slabp],
        "f3d_resample_z": [_dp, _dp, _sz, _sz, _sz, _sz, _slabp, _slabp],
        "f3d_add": [_dp, _dp, _sz, _sz, _sz, _slabp],
        "f3d_median": [_dp, _sz, _sz, _sz, _sz, _dp, _slabp],
        # up to three volumes of one box per launch (arrays of device pointers)
        "f3d_resample_x_n": [_dpp, _dpp, _sz, _sz, _sz, _sz, _sz, _slabp],
        "f3d_resample_y_n": [_dpp, _dpp, _sz, _sz, _sz, _sz, _sz, _slabp],
        "f3d_resample_z_n": [_dpp, _dpp, _sz, _sz, _sz, _sz, _sz, _slabp, _slabp],
        "f3d_add_n": [_dpp, _dpp, _sz, _sz, _sz, _sz, _slabp],
        "f3d_median_n": [_dpp, _sz, _sz, _sz, _sz, _sz, _dpp, _slabp],
        "f3d_clear_box_n": [_dpp, _sz, _sz, _sz, _sz, _slabp],
        "f3d_set_conv_taps": [_fp, _sz],
        "f3d_conv_rows": [_dp, _dp, _sz, _sz, _sz, _sz, _slabp],
        "f3d_conv_cols": [_dp, _dp, _sz, _sz, _sz, _sz, _slabp],
        "f3d_conv_slices": [_dp, _dp, _sz, _sz, _sz, _sz, _slabp],
        "f3d_conv_rows_cols": [_dp, _dp, _sz, _sz, _sz, _sz, _slabp],
        "f3d_range_push": [C.c_char_p], "f3d_range_pop": [],
        "f3d_prof_enable": [C.c_int], "f3d_prof_reset": [], "f3d_prof_select": [C.c_uint],
        "f3d_prof_read": [C.c_int, _sz, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)],
        "f3d_abs_max": [_dp, _sz, _sz, _sz, _slabp, _fp],
        "f3d_comm_unique_id": [C.c_void_p], "f3d_comm_init": [C.c_void_p, C.c_int, C.c_int], "f3d_comm_destroy": [],
        "f3d_comm_rank": [C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "f3d_comm_info": [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_ulonglong)] * 2,
        "f3d_pack_planes": [_dp, C.c_int, C.c_int, _sz, _sz, _dp, _sz],
        "f3d_unpack_planes": [_dp, C.c_int, C.c_int, _sz, _sz, _dp, _sz],
        "f3d_copy_planes": [_dp, C.c_int, _dp, C.c_int, C.c_int, _sz, _sz],
        "f3d_copy_plane_segments": [C.POINTER(_dp), C.POINTER(C.c_int), C.POINTER(_dp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, _sz, _sz],
        "f3d_pack_segments": [C.POINTER(_dp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_sz), C.c_int, _sz, _sz, _dp],
        "f3d_unpack_segments": [C.POINTER(_dp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_sz), C.c_int, _sz, _sz, _dp],
        "f3d_comm_sendrecv": [_dp, C.POINTER(_sz), C.POINTER(_sz), _dp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(C.c_int), C.c_int],
        "f3d_flow_stats": [_dp, _dp, _dp, _sz, _sz, _sz, _slabp, _fp, _fp, C.POINTER(C.c_double)],
        "f3d_residual_stats": [_dp, _dp, _sz, _sz, _sz, _slabp, C.POINTER(C.c_double), C.POINTER(C.c_double), _fp],
        "f3d_comm_sendrecv_begin": [_dp, C.POINTER(_sz), C.POINTER(_sz), _dp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(C.c_int), C.c_int],
        "f3d_comm_sendrecv_end": [],
        "f3d_comm_allreduce_max_f32": [_fp],
        "f3d_comm_timing": [C.c_int],
        "f3d_comm_mark": [C.c_int, C.c_int],
        "f3d_comm_timing_read": [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_ulonglong)],
    }
    for name, args in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            # an older build named by F3D_LIBDIR (A/B timing of two libraries in one GPU call) may lack the newest entry points;
            # the library of the package itself must export every one of them
            if os.environ.get("F3D_LIBDIR"):
                continue
            raise
        fn.argtypes = args
        fn.restype = C.c_int
    _hip = L
    if hasattr(L, "f3d_crash_maps_enable"):
        _arm_crash_maps(L)
    return L


def _arm_crash_maps(L):
    """F3D_CRASH_MAPS=<file> (or any run under a rocprofiler tool): a fatal signal leaves /proc/self/maps in <file> before the
    usual handlers run, so the anonymous frames of a native stack trace can be put into libraries (include/f3d.h,
    f3d_crash_maps_enable; the one crash on record happened under `rocprofv3 --pmc` and could only be resolved after the fact)."""
    path = os.environ.get("F3D_CRASH_MAPS")
    if not path:
        blob = " ".join(os.environ.get(k, "") for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB"))
        if "rocprof" not in blob:
            return
        base = os.environ.get("F3D_OUT") or os.getcwd()
        path = os.path.join(base, f"f3d_crash_maps.{os.getpid()}.txt")
    L.f3d_crash_maps_enable(path.encode())


def host():
    """Handle of libf3d_host.so with argument types declared (include/f3d_host.h)."""
    global _host
    if _host is not None:
        return _host
    hip()
    L = _load("libf3d_host.so")
    pp = C.POINTER(FlowParams)
    sig = {
        "f3d_flow_create": [C.POINTER(C.c_void_p)], "f3d_flow_initialize": [C.c_void_p, _sz, _sz, _sz],
        "f3d_flow_compute": [C.c_void_p, _fp, _fp, pp, C.c_int, _fp, _fp, _fp],
        "f3d_flow_upload": [C.c_void_p, _fp, _fp],
        "f3d_flow_compute_resident": [C.c_void_p, pp, C.c_int, _fp],
        "f3d_flow_download": [C.c_void_p, _fp, _fp, _fp],
        "f3d_flow_container": [C.c_void_p, C.POINTER(Size4)], "f3d_flow_destroy": [C.c_void_p],
        "f3d_flow_set_level_stats": [C.c_void_p, C.c_int], "f3d_flow_level_stat_count": [C.c_void_p, C.POINTER(_sz)],
        "f3d_flow_level_stat": [C.c_void_p, _sz, C.POINTER(LevelStat)],
        "f3d_flow_final_residual": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "f3d_flow_trajectory_begin": [C.c_void_p], "f3d_flow_trajectory_append": [C.c_void_p],
        "f3d_flow_trajectory_download": [C.c_void_p, _fp, _fp, _fp, C.POINTER(C.c_ulonglong)],
        "f3d_flow_trajectory_end": [C.c_void_p],
        "f3d_flow_initial_upload": [C.c_void_p, _fp, _fp, _fp, C.POINTER(InitialInfo)],
        "f3d_flow_initial_take": [C.c_void_p, C.c_int, C.POINTER(InitialInfo)],
        "f3d_flow_initial_download": [C.c_void_p, _fp, _fp, _fp], "f3d_flow_initial_end": [C.c_void_p],
        "f3d_flow_compute_resident_from_initial": [C.c_void_p, pp, C.c_int, _fp],
        "f3d_flow_compute_from_initial": [C.c_void_p, _fp, _fp, pp, C.c_int, _fp, _fp, _fp],
        "f3d_block_match_layout": [_sz, _sz, _sz] + [C.c_int] * 5 + [C.POINTER(BlockMatchGrid)],
        "f3d_flow_block_match": [C.c_void_p] + [C.c_int] * 5 + [_sz, _fp, C.c_void_p, C.c_double, C.POINTER(BlockMatchGrid),
                                 C.POINTER(BlockMatchInfo), C.POINTER(BlockMatchSummary)],
        "f3d_flow_block_match_rows": [C.c_void_p, _sz, C.c_void_p, C.c_void_p],
        "f3d_flow_initial_from_nodes": [C.c_void_p, C.POINTER(ValidateStats), C.POINTER(InitialInfo)],
        "f3d_block_match_solve": [C.c_void_p, C.POINTER(BlockMatchGrid), C.c_void_p, C.c_double, C.c_void_p,
                                  C.POINTER(BlockMatchSummary)],
        "f3d_subset_match_layout": [_sz, _sz, _sz, C.c_int, C.c_int, C.POINTER(SubsetGrid)],
        "f3d_flow_subset_match": [C.c_void_p] + [C.c_int] * 5 + [C.c_double] * 3 + [C.POINTER(SubsetGrid), C.POINTER(SubsetInfo),
                                                                                   C.POINTER(SubsetSummary)],
        "f3d_flow_subset_match_rows": [C.c_void_p, _sz, C.c_void_p, C.c_void_p],
        "f3d_subset_match_table": [C.c_void_p, C.POINTER(SubsetGrid), C.c_double, C.POINTER(_fp), C.c_void_p, C.POINTER(SubsetSummary)],
        "f3d_flow_strain_compute": [C.c_void_p, C.c_int, C.c_uint, C.POINTER(_fp), C.POINTER(StrainStats)],
        "f3d_flow_strain_end": [C.c_void_p],
        "f3d_flow_window_strain_compute": [C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.POINTER(_fp),
                                           C.POINTER(WindowStrainStats)],
        "f3d_flow_window_strain_end": [C.c_void_p],
        "f3d_flow_principal_compute": [C.c_void_p, C.c_int, C.c_uint, C.POINTER(_fp), C.POINTER(PrincipalStats)],
        "f3d_flow_principal_end": [C.c_void_p],
        "f3d_flow_polar_compute": [C.c_void_p, C.c_int, C.c_uint, C.POINTER(_fp), C.POINTER(PolarStats)],
        "f3d_flow_polar_end": [C.c_void_p],
        "f3d_flow_window_principal_compute": [C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.POINTER(_fp),
                                              C.POINTER(PrincipalStats)],
        "f3d_flow_window_principal_end": [C.c_void_p],
        "f3d_flow_window_polar_compute": [C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.POINTER(_fp), C.POINTER(PolarStats)],
        "f3d_flow_window_polar_end": [C.c_void_p],
        "f3d_flow_inverse_compute": [C.c_void_p, C.c_int, C.c_uint, C.c_float, C.POINTER(_fp), C.POINTER(InverseStats)],
        "f3d_flow_inverse_end": [C.c_void_p],
        "f3d_flow_match_compute": [C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_float, C.POINTER(_fp), C.POINTER(CorrelationStats)],
        "f3d_flow_match_end": [C.c_void_p],
        "f3d_motion_solve": [C.POINTER(MotionSums), C.c_int, C.POINTER(MotionFit)],
        "f3d_motion_solve_labels": [C.POINTER(MotionSums), _sz, C.c_int, C.c_ulonglong, C.POINTER(C.c_double), C.POINTER(MotionFit),
                                    C.POINTER(C.c_int)],
        "f3d_flow_motion_compute": [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(_fp), C.POINTER(MotionFit),
                                    C.POINTER(MotionResidual)],
        "f3d_flow_motion_end": [C.c_void_p],
        "f3d_flow_label_motion_compute": [C.c_void_p, C.c_int, C.POINTER(C.c_int), _sz, C.c_int, C.c_ulonglong, C.POINTER(_fp),
                                          C.POINTER(MotionFit), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(LabelInfo)],
        "f3d_flow_label_motion_end": [C.c_void_p],
        "f3d_contact_kinematics": [C.POINTER(Contact), _sz, C.POINTER(_sz), C.POINTER(MotionFit), C.POINTER(C.c_int), _sz, C.c_ulonglong,
                                   C.POINTER(ContactKinematics)],
        "f3d_flow_contacts_compute": [C.c_void_p, C.c_int, C.POINTER(C.c_int), _sz, C.POINTER(C.POINTER(Contact)), C.POINTER(_sz),
                                      C.POINTER(ContactInfo)],
        "f3d_flow_contacts_end": [C.c_void_p],
        "f3d_label_shape_solve": [C.POINTER(LabelShapeSums), _sz, C.POINTER(LabelShape)],
        "f3d_flow_label_shapes_compute": [C.c_void_p, C.POINTER(C.c_int), _sz, C.POINTER(LabelShape), C.POINTER(LabelShapeInfo)],
        "f3d_flow_labels_compute": [C.c_void_p, _dp, C.c_float, C.c_float, C.c_ulonglong, C.POINTER(C.POINTER(C.c_ulonglong)), C.POINTER(_sz),
                                    C.POINTER(ComponentInfo)],
        "f3d_flow_labels_split": [C.c_void_p, _dp, C.c_float, C.c_float, C.c_ulonglong, C.c_ulonglong, C.POINTER(C.POINTER(C.c_ulonglong)),
                                  C.POINTER(_sz), C.POINTER(SplitInfo)],
        "f3d_flow_labels_end": [C.c_void_p], "f3d_flow_labels_download": [C.c_void_p, C.POINTER(C.c_int)],
        "f3d_overlap_solve": [C.POINTER(Overlap), _sz, _sz, _sz, C.c_double, C.POINTER(TrackA), C.POINTER(TrackB), C.POINTER(C.c_int),
                              C.POINTER(TrackSummary)],
        "f3d_flow_labels_b_upload": [C.c_void_p, C.POINTER(C.c_int)],
        "f3d_flow_labels_b_segment": [C.c_void_p, _dp, C.c_float, C.c_float, C.c_ulonglong, C.c_ulonglong,
                                      C.POINTER(C.POINTER(C.c_ulonglong)), C.POINTER(_sz), C.POINTER(SplitInfo)],
        "f3d_flow_overlap_compute": [C.c_void_p, C.c_int, _sz, _sz, C.POINTER(C.POINTER(Overlap)), C.POINTER(_sz), C.POINTER(OverlapInfo)],
        "f3d_flow_overlap_end": [C.c_void_p],
        "f3d_flow_labels_b_relabel": [C.c_void_p, C.POINTER(C.c_int), _sz],
        "f3d_flow_labels_b_download": [C.c_void_p, C.POINTER(C.c_int)],
        "f3d_label_field_solve": [C.POINTER(LabelFieldSumsRow), C.POINTER(C.c_uint), _sz, C.c_int, C.c_float, C.c_float, _sz, C.c_ulonglong,
                                  C.POINTER(LabelFieldStat), C.POINTER(LabelFieldSummary)],
        "f3d_label_field_shift": [C.c_float, C.c_float, C.c_ulonglong],
        "f3d_flow_label_field_compute": [C.c_void_p, _dp, _sz, C.c_int, _fp, _sz, C.c_ulonglong, C.POINTER(LabelFieldStat),
                                         C.POINTER(C.c_uint), C.POINTER(LabelFieldInfo), C.POINTER(LabelFieldSummary)],
        "f3d_flow_label_field_range": [C.c_void_p, _dp, _fp, _fp, C.POINTER(RangeInfo)],
        "f3d_flow_field_container": [C.c_void_p, C.c_char_p, C.POINTER(_dp)],
        "f3d_flow_labels_paint": [C.c_void_p, _fp, _sz, _fp],
        "f3d_histogram_edge": [C.c_float, C.c_float, _sz, _sz, _fp],
        "f3d_otsu": [C.POINTER(C.c_ulonglong), _sz, C.c_int, C.POINTER(C.c_uint), C.POINTER(OtsuInfo)],
        "f3d_histogram_rank": [C.POINTER(C.c_ulonglong), _sz, C.c_ulonglong, C.POINTER(C.c_uint)],
        "f3d_flow_histogram": [C.c_void_p, _dp, _fp, _sz, C.POINTER(C.c_ulonglong), C.POINTER(HistogramInfo), _fp, _fp],
        "f3d_flow_validate_compute": [C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_float, C.c_uint, C.c_uint, C.c_uint, C.c_float,
                                      C.POINTER(_fp), C.POINTER(ValidateStats)],
        "f3d_flow_validate_end": [C.c_void_p],
        "f3d_op_create": [C.POINTER(C.c_void_p), C.c_char_p], "f3d_op_initialize": [C.c_void_p, C.POINTER(Size4)],
        "f3d_op_execute": [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), _sz],
        "f3d_op_execute_batch": [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(_sz), _sz],
        "f3d_op_set_slab": [C.c_void_p, _slabp], "f3d_op_destroy": [C.c_void_p],
        "f3d_level_geometry": [_sz, _sz, _sz, C.c_float, C.c_int, C.POINTER(Size4), _fp, _fp, _fp],
        "f3d_gaussian_taps": [C.c_float, _fp, _sz, C.POINTER(_sz)],
        "f3d_raw_read_u8": [C.c_char_p, _sz, _sz, _sz, _fp], "f3d_raw_read_f32": [C.c_char_p, _sz, _sz, _sz, _fp],
        "f3d_raw_write_u8": [C.c_char_p, _fp, _sz, _sz, _sz], "f3d_raw_write_f32": [C.c_char_p, _fp, _sz, _sz, _sz],
        "f3d_vtk_write_flow": [C.c_char_p, _fp, _fp, _fp, _sz, _sz, _sz],
        "f3d_synth_pair": [_sz, _sz, _sz, _fp, _fp],
        "f3d_synth_planes": [_sz, _sz, _sz, _sz, _sz, _fp, _fp, _fp],
        "f3d_slabflow_create": [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int],
        "f3d_slabflow_initialize": [C.c_void_p, _sz, _sz, _sz],
        "f3d_slabflow_compute": [C.c_void_p, _fp, _fp, pp, _fp, _fp, _fp],
        "f3d_slabflow_upload": [C.c_void_p, _fp, _fp],
        "f3d_slabflow_compute_resident": [C.c_void_p, pp, _fp],
        "f3d_slabflow_download": [C.c_void_p, _fp, _fp, _fp],
        "f3d_slabflow_overlapped_iterations": [C.c_void_p, C.POINTER(_sz)],
        "f3d_slabflow_batched_exchanges": [C.c_void_p, C.POINTER(_sz)],
        "f3d_slabflow_gathered_warps": [C.c_void_p, C.POINTER(_sz)],
        "f3d_slabflow_stage_exchanges": [C.c_void_p, C.POINTER(_sz)],
        "f3d_slabflow_set_exchange_per_stage": [C.c_void_p, C.c_int],
        "f3d_slabflow_destroy": [C.c_void_p],
        "f3d_plan_owned": [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "f3d_plan_exchange": [C.c_int] * 5 + [C.POINTER(C.c_int)] * 5 + [C.c_int],
        "f3d_plan_resample_source": [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2,
        "f3d_volume_wrap": [C.POINTER(C.c_void_p), _fp, _sz, _sz, _sz], "f3d_volume_destroy": [C.c_void_p],
        "f3d_op_solve_p_last": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_sz), C.POINTER(C.c_int)],
        "f3d_op_solve_p_fused_weights": [C.c_void_p, C.POINTER(C.c_int)],
        "f3d_plan_solve_piecemeal": [_sz, _sz, _sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 5,
        "f3d_plan_sweeps": [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2 + [C.c_int],
        "f3d_plan_sweeps_weights_first": [C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.c_int],
        "f3d_pair8_plan": [C.c_int] * 7 + [C.POINTER(C.c_longlong)],
        "f3d_solver_chunk_limit": [C.c_ulonglong, C.c_int],
        "f3d_pair8_decode": [C.c_int] * 4 + [C.POINTER(C.c_longlong)] + [C.c_int] * 5 + [C.POINTER(C.c_int)] * 2,
        "f3d_pair8_plan_wide": [C.c_int] * 7 + [C.POINTER(C.c_longlong)],
        "f3d_pair8_decode_wide": [C.c_int] * 4 + [C.POINTER(C.c_longlong)] + [C.c_int] * 5 + [C.POINTER(C.c_int)] * 2,
        "f3d_pflow_create": [C.POINTER(C.c_void_p)], "f3d_pflow_initialize": [C.c_void_p, _sz, _sz, _sz],
        "f3d_pflow_compute": [C.c_void_p, _fp, _fp, _sz, _sz, _sz, pp, C.c_int, _fp, _fp, _fp, _fp],
        "f3d_pflow_stats": [C.c_void_p, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)], "f3d_pflow_destroy": [C.c_void_p],
        "f3d_pflow_set_resident": [C.c_void_p, C.c_int], "f3d_pflow_set_full_pipeline": [C.c_void_p, C.c_int], "f3d_pflow_originals_on_device": [C.c_void_p, C.POINTER(C.c_int)],
        "f3d_pflow_operator_seconds": [C.c_void_p, C.POINTER(C.c_double)],
        "f3d_pflow_levels_registered_inside": [C.c_void_p, C.POINTER(_sz)],
        "f3d_pflow_levels_with_constants_on_device": [C.c_void_p, C.POINTER(_sz)],
        "f3d_host_shutdown": [],
    }
    for name, args in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if os.environ.get("F3D_LIBDIR"):   # an older build under A/B timing (see hip())
                continue
            raise
        fn.argtypes = args
        fn.restype = C.c_int
    L.f3d_flow_default_params.argtypes = [pp]
    L.f3d_flow_default_params.restype = None
    L.f3d_op_name.argtypes = [C.c_void_p]
    L.f3d_op_name.restype = C.c_char_p
    L.f3d_max_warp_level.argtypes = [_sz, _sz, _sz, C.c_float]
    L.f3d_max_warp_level.restype = _sz
    L.f3d_volume_object.argtypes = [C.c_void_p]
    L.f3d_volume_object.restype = C.c_void_p
    L.f3d_volume_data.argtypes = [C.c_void_p]
    L.f3d_volume_data.restype = C.c_void_p
    L.f3d_piecemeal_budget_bytes.argtypes = []
    L.f3d_piecemeal_budget_bytes.restype = _sz
    if hasattr(L, "f3d_host_last_error"):
        L.f3d_host_last_error.argtypes = []
        L.f3d_host_last_error.restype = C.c_char_p
    _host = L
    return L


def shutdown():
    """Orderly end of device use: host volumes that are still page-locked are released, then f3d_host_shutdown() drops the
    out-of-core arena, the copy queues, the RCCL communicator, the timing events and the library stream.  Registered with
    atexit on import, so it runs while the interpreter, numpy's heap and the HIP runtime are all still alive -- nothing is
    left to the order in which the process unloads libraries.  Idempotent."""
    HostVolume.release_all()
    if _host is not None:
        _host.f3d_host_shutdown()
    elif _hip is not None and _hip.f3d_is_initialized():
        _hip.f3d_comm_destroy()
        _hip.f3d_shutdown()


atexit.register(shutdown)


def check(status, what="f3d call"):
    if status != 0:
        msg = hip().f3d_last_error()
        raise F3dError(f"{what} failed: {msg.decode() if msg else 'status %d' % status}")


def _host_check(status, what):
    """check() for the calls that can fail in the host library itself (f3d_host_last_error describes those)"""
    if status != 0:
        msg = host().f3d_host_last_error()
        raise F3dError(f"{what} failed: {msg.decode() if msg else 'status %d' % status}")


def _entry(name, argtypes, what):
    """An entry point of the device library that is declared on first use: it is not in hip()'s table, so that a library without it
    (an older build, the host-memory stand-in of the tests) still loads; using it there raises."""
    try:
        fn = getattr(hip(), name)
    except AttributeError:
        raise F3dError(f"{os.path.join(_LIBDIR, 'libf3d_hip.so')} has no {name}: this device library cannot {what}") from None
    fn.argtypes = argtypes
    fn.restype = C.c_int
    return fn


def solve_sweep_add_entry():
    """f3d_solve_sweep_add (include/f3d.h): the last sweep of a level that stores flow + increments; arguments of f3d_solve_sweep"""
    return _entry("f3d_solve_sweep_add", [_dp] * 10 + [_sz] * 3 + [C.c_float] * 4 + [_dp] * 3 + [_slabp],
                  "add the increments to the flow inside the last sweep")


def solve_phi_ksi_sweep_fd_entry():
    """f3d_solve_phi_ksi_sweep_fd (include/f3d.h): phi / ksi of an outer iteration and its first sweep in one launch"""
    return _entry("f3d_solve_phi_ksi_sweep_fd", [_dp] * 10 + [_sz] * 3 + [C.c_float] * 6 + [_dp] * 5 + [_slabp],
                  "compute the weights in front of a sweep")


def solve_sweep2_add_fd_entry():
    """f3d_solve_sweep2_add_fd (include/f3d.h): two sweeps that store flow + increments; arguments of f3d_solve_sweep2_fd"""
    return _entry("f3d_solve_sweep2_add_fd", [_dp] * 12 + [_sz] * 3 + [C.c_float] * 4 + [_dp] * 3 + [_slabp],
                  "add the increments to the flow inside the last two sweeps")


def _compose_entry():
    return _entry("f3d_compose_flow", [_dp] * 6 + [_sz] * 3 + [C.POINTER(C.c_ulonglong)], "compose flows into a trajectory")


def _initial_entry():
    return _entry("f3d_initial_flow", [_dp] * 6 + [_sz] * 3 + [C.POINTER(InitialInfo)], "prepare a displacement to start a solve from")


def _strain_entry():
    return _entry("f3d_flow_strain", [_dp] * 3 + [_dpp, C.c_uint] + [_sz] * 3 + [C.POINTER(StrainStats)], "compute strain fields")


def _window_strain_entry():
    return _entry("f3d_window_strain", [_dp] * 3 + [_dpp, C.c_uint, C.c_uint, C.c_uint] + [_sz] * 3 + [C.POINTER(WindowStrainStats)],
                  "compute strain fields over a window")


def _principal_entry():
    return _entry("f3d_principal_strain", [_dp] * 3 + [_dpp, C.c_uint] + [_sz] * 3 + [C.POINTER(PrincipalStats)],
                  "compute principal strains")


def _polar_entry():
    return _entry("f3d_polar_decomposition", [_dp] * 3 + [_dpp, C.c_uint] + [_sz] * 3 + [C.POINTER(PolarStats)],
                  "compute local rotations and stretches")


def _principal_from_gradient_entry():
    return _entry("f3d_principal_from_gradient", [_dpp, _dpp, C.c_uint] + [_sz] * 3 + [C.POINTER(PrincipalStats)],
                  "compute principal strains of a stored gradient")


def _polar_from_gradient_entry():
    return _entry("f3d_polar_from_gradient", [_dpp, _dpp, C.c_uint] + [_sz] * 3 + [C.POINTER(PolarStats)],
                  "compute local rotations and stretches of a stored gradient")


def _inverse_entry():
    return _entry("f3d_invert_displacement", [_dp] * 7 + [_sz] * 3 + [C.c_uint, C.c_float, C.POINTER(InverseStats)],
                  "invert displacements")


def _carry_entry():
    return _entry("f3d_carry_field", [_dp] * 5 + [_sz] * 3 + [C.c_uint, C.POINTER(C.c_ulonglong)],
                  "carry fields through a displacement")


def _correlation_entry():
    return _entry("f3d_local_correlation", [_dp] * 2 + [_dpp, C.c_uint, C.c_uint, C.c_float] + [_sz] * 3 + [C.POINTER(CorrelationStats)],
                  "compute the local correlation of two volumes")


def _motion_entry():
    """(f3d_motion_sums, f3d_remove_motion)"""
    what = "fit or remove the motion of a displacement"
    return (_entry("f3d_motion_sums", [_dp] * 4 + [C.c_float] + [_sz] * 3 + [C.POINTER(MotionSums)], what),
            _entry("f3d_remove_motion", [_dp] * 6 + [C.POINTER(MotionFit)] + [_sz] * 3 + [C.POINTER(MotionResidual)], what))


_LABEL_MOTION_WHAT = "fit or remove the motion of the labels of a segmentation"


def _label_sums_entry():
    return _entry("f3d_label_motion_sums", [_dp] * 4 + [_sz, _dp, C.c_float] + [_sz] * 3 + [C.POINTER(MotionSums), C.POINTER(LabelInfo)],
                  _LABEL_MOTION_WHAT)


def _label_remove_entry():
    return _entry("f3d_remove_label_motion", [_dp] * 4 + [_sz, C.POINTER(MotionFit), C.POINTER(C.c_int)] + [_dp] * 3 + [_sz] * 3 +
                  [C.POINTER(MotionResidual)], _LABEL_MOTION_WHAT)


def _label_motion_entry():
    """(f3d_label_motion_sums, f3d_remove_label_motion)"""
    return _label_sums_entry(), _label_remove_entry()


def _contacts_entry():
    return _entry("f3d_label_contacts", [_dp] * 4 + [_sz] * 5 + [C.POINTER(Contact), C.POINTER(ContactInfo)],
                  "find the contacts between the labels of a segmentation")


def _label_shape_entry():
    return _entry("f3d_label_shape_sums", [_dp] + [_sz] * 4 + [C.POINTER(LabelShapeSums), C.POINTER(LabelShapeInfo)],
                  "sum the shapes of the labels of a segmentation")


def _label_field_entry():
    return _entry("f3d_label_field_sums", [_dp, _dp, _sz, C.c_int, C.c_float, C.c_float] + [_sz] * 4 +
                  [C.POINTER(LabelFieldSumsRow), C.POINTER(C.c_uint), C.POINTER(LabelFieldInfo)],
                  "sum a field over the labels of a segmentation")


def _paint_entry():
    return _entry("f3d_paint_labels", [_dp, _sz, _fp, _dp] + [_sz] * 3, "paint a value per label into a volume")


def _overlap_entry():
    return _entry("f3d_label_overlap", [_dp, _sz, _dp, _sz] + [_dp] * 3 + [_sz] * 4 + [C.POINTER(Overlap), C.POINTER(OverlapInfo)],
                  "find the overlap of two label volumes")


def _relabel_entry():
    return _entry("f3d_relabel_labels", [_dp, _sz, C.POINTER(C.c_int), _dp] + [_sz] * 3 + [C.POINTER(C.c_ulonglong)],
                  "give the bodies of a label volume new numbers")


def _components_entry():
    return _entry("f3d_label_components", [_dp, C.c_float, C.c_float, C.c_ulonglong, _dp] + [_sz] * 3 +
                  [C.POINTER(C.c_ulonglong), _sz, C.POINTER(ComponentInfo)], "label the connected bodies of a thresholded volume")


def _histogram_entry():
    return _entry("f3d_histogram", [_dp, _dp, C.c_float, C.c_float] + [_sz] * 4 + [C.POINTER(C.c_ulonglong), C.POINTER(HistogramInfo)],
                  "count the grey values of a volume")


def _value_range_entry():
    return _entry("f3d_value_range", [_dp, _dp] + [_sz] * 3 + [_fp, _fp, C.POINTER(RangeInfo)],
                  "find the finite minimum and maximum of a volume")


def _nearest_entry():
    return _entry("f3d_nearest_seed", [_dp, C.c_uint, C.c_uint] + [_dp] * 3 + [_sz] * 3 + [C.POINTER(NearestInfo)],
                  "compute the exact distance and nearest-seed transform")


def _split_entry():
    return _entry("f3d_split_components", [_dp, C.c_float, C.c_float, C.c_ulonglong, C.c_ulonglong, _dp] + [_sz] * 3 +
                  [C.POINTER(C.c_ulonglong), _sz, C.POINTER(SplitInfo)], "take the touching bodies of a thresholded volume apart")


def _validate_entry():
    return _entry("f3d_validate_displacement", [_dp] * 4 + [C.c_float, C.c_uint, C.c_float, C.c_float, C.c_uint, C.c_uint, _dpp, C.c_uint] +
                  [_sz] * 3 + [C.POINTER(ValidateStats)], "validate a displacement")


def _mask(fields, groups, what):
    """the F3D_* bits of an iterable of group names (the keys of `groups`) or of a comma-separated string of them"""
    if isinstance(fields, str):
        fields = fields.split(",")
    mask = 0
    for f in fields:
        if f not in groups:
            raise ValueError(f"unknown {what} group {f!r} (one of {', '.join(groups)})")
        mask |= groups[f]
    if not mask:
        raise ValueError(f"no {what} group selected")
    return mask


def _source(source):
    """F3D_STRAIN_OF_FLOW / F3D_STRAIN_OF_TRAJECTORY of the `source` argument of OpticalFlow.strain, .principal and .inverse"""
    src = {"flow": 0, "trajectory": 1}.get(source)
    if src is None:
        raise ValueError(f"source must be 'flow' or 'trajectory', not {source!r}")
    return src


@contextlib.contextmanager
def _on_device(volumes, mismatch):
    """Volumes from anywhere in device containers of their own: yields (box, pointers, (w, h, d)) with `volumes` (numpy [z, y, x], made
    contiguous float32; ValueError(mismatch) unless all are 3-D of one shape) uploaded into a fresh Containers of their size.  The
    caller allocates its outputs, calls box.set_current() and the entry point, and downloads; on the way out the container
    geometry of whoever set one before (a driver on this lane) is put back and everything is freed."""
    vols = [np.ascontiguousarray(a, dtype=np.float32) for a in volumes]
    if any(a.ndim != 3 or a.shape != vols[0].shape for a in vols):
        raise ValueError(mismatch)
    d, h, w = vols[0].shape
    box = Containers(w, h, d)
    previous = Size4()
    check(hip().f3d_get_container(C.byref(previous)), "f3d_get_container")
    try:
        yield box, [box.new(a) for a in vols], (w, h, d)
    finally:
        if previous.pitch:
            hip().f3d_set_container(C.byref(previous))
        box.free()


def compose_flow(acc, inc):
    """One trajectory step on the device (include/f3d.h, f3d_compose_flow) for flows from anywhere: acc = (u, v, w) displacement of
    every voxel of frame 0 so far, inc = (u, v, w) flow of the next pair (numpy [z, y, x] float32, voxel units).  Returns
    (u, v, w, lost): acc + inc sampled trilinearly at x + acc, NaN where the point has left the volume, and the number of voxels
    whose u is NaN.  The inputs are not modified."""
    fn = _compose_entry()
    acc, inc = list(acc), list(inc)
    mismatch = "acc and inc must be three [z, y, x] volumes of one shape each"
    if len(acc) != 3 or len(inc) != 3:
        raise ValueError(mismatch)
    with _on_device(acc + inc, mismatch) as (box, p, dims):
        box.set_current()
        lost = C.c_ulonglong()
        check(fn(*p, *dims, C.byref(lost)), "f3d_compose_flow")
        return tuple(box.download(a, dims) for a in p[:3]) + (int(lost.value),)


def initial_flow(u, v, w):
    """A displacement made fit to start a solve from (include/f3d.h, f3d_initial_flow) for volumes from anywhere (numpy [z, y, x]
    float32, voxel units).  Returns ((u, v, w), info): the three components where all three are finite and +0 in all three where
    one is not, and an InitialInfo with the voxels, the replaced voxels, the finite voxels whose end point leaves the volume, and
    the largest |component| over the finite voxels.  The inputs are not modified."""
    fn = _initial_entry()
    mismatch = "u, v and w must be three [z, y, x] volumes of one shape"
    with _on_device([u, v, w], mismatch) as (box, p, dims):
        box.set_current()
        info = InitialInfo()
        check(fn(*p, *p, *dims, C.byref(info)), "f3d_initial_flow")
        return tuple(box.download(a, dims) for a in p), info


def _block_match_entry():
    return _entry("f3d_block_match", [_dp, _dp, C.c_float, C.c_float, _sz, _sz, _sz, _sz, C.POINTER(BlockMatchGrid), C.c_void_p, C.c_void_p,
                                      C.POINTER(BlockMatchInfo)], "match blocks of two frames")


def _expand_nodes_entry():
    return _entry("f3d_expand_nodes", [_fp, _fp, _fp] + [C.c_int] * 7 + [_dp] * 3 + [_sz] * 3, "expand node vectors to a dense field")


def block_match_grid(dims, step=16, window=8, search=8, origin=None, counts=None):
    """The node grid of block_match over a (w, h, d) volume as a BlockMatchGrid: nodes `step` apart whose (2 window + 1)^3 windows lie
    inside the volume, as many as fit and centred, unless origin = (ox, oy, oz) and / or counts = (nx, ny, nz) say otherwise.
    search: one radius or (rx, ry, rz).  ValueError when a window leaves the volume."""
    radii = (int(search),) * 3 if np.isscalar(search) else tuple(int(r) for r in search)
    step, window = int(step), int(window)
    if len(radii) != 3 or step < 1 or window < 1:
        raise ValueError("search must be one radius or three, step and window at least 1")
    first, count = [], []
    for axis, n in enumerate(dims):
        room = int(n) - 1 - 2 * window
        if room < 0:
            raise ValueError(f"a window of radius {window} leaves the volume along {'xyz'[axis]} ({n} voxels)")
        o = window + (room % step) // 2 if origin is None else int(origin[axis])
        c = (int(n) - 1 - window - o) // step + 1 if counts is None else int(counts[axis])
        if o < window or c < 1 or o + (c - 1) * step + window > int(n) - 1:
            raise ValueError(f"a window of radius {window} leaves the volume along {'xyz'[axis]}: origin {o}, {c} nodes, step {step}")
        first.append(o)
        count.append(c)
    return BlockMatchGrid(*first, step, *count, window, *radii)


class BlockMatchNodes:
    """The node table of block_match: `rows`, one BLOCK_MATCH_NODE record per node (x fastest); `records`, the [nodes, 32] int32 records
    of f3d_block_match they were solved from; `info` and `summary`, the dicts of f3d_block_match_info and f3d_block_match_summary;
    `grid` (BlockMatchGrid), `centre`.  origin, step, counts and u, v, w as [nz, ny, nx] arrays feed expand_nodes."""

    def __init__(self, rows, records, info, summary, grid, centre):
        self.rows, self.records, self.info, self.summary, self.grid, self.centre = rows, records, info, summary, grid, centre
        self.origin, self.step, self.counts = (grid.ox, grid.oy, grid.oz), grid.step, (grid.nx, grid.ny, grid.nz)

    def __len__(self):
        return len(self.rows)

    def _component(self, name):
        return np.ascontiguousarray(self.rows[name].reshape(self.counts[::-1]))

    u = property(lambda self: self._component("u"))
    v = property(lambda self: self._component("v"))
    w = property(lambda self: self._component("w"))

    def as_table(self):
        return [dict(x=int(r["position"][0]), y=int(r["position"][1]), z=int(r["position"][2]), shift=tuple(int(s) for s in r["shift"]),
                     offset=tuple(float(o) for o in r["offset"]), zncc=float(r["zncc"]), status=BLOCK_NODE_STATUS[int(r["status"])],
                     evaluated=int(r["evaluated"]), outside=int(r["outside"]), flat=int(r["flat"])) for r in self.rows]


def _centre_array(centre, nodes):
    if centre is None:
        return None
    centre = np.ascontiguousarray(centre, dtype=np.int32)
    if centre.size != 3 * nodes:
        raise ValueError(f"centre must hold one (x, y, z) triple per node, {nodes} of them")
    return centre.reshape(nodes, 3)


def solve_block_match(records, grid, centre=None, min_zncc=0.5):
    """f3d_block_match_solve (include/f3d_host.h) of [nodes, 32] int32 records: -> (rows as BLOCK_MATCH_NODE records, summary dict).
    Host code, no device needed."""
    nodes = grid.nx * grid.ny * grid.nz
    records = np.ascontiguousarray(records, dtype=np.int32)
    if records.shape != (nodes, BLOCK_MATCH_RECORD_WORDS):
        raise ValueError(f"records must be [{nodes}, {BLOCK_MATCH_RECORD_WORDS}] int32")
    centre = _centre_array(centre, nodes)
    rows, summary = np.zeros(nodes, BLOCK_MATCH_NODE), BlockMatchSummary()
    _host_check(host().f3d_block_match_solve(records.ctypes.data, C.byref(grid), None if centre is None else centre.ctypes.data,
                                             float(min_zncc), rows.ctypes.data, C.byref(summary)), "f3d_block_match_solve")
    return rows, summary.as_dict()


def block_match(a, b, step=16, window=8, search=8, bins=256, range=None, centre=None, min_zncc=0.5, origin=None, counts=None):
    """Coarse block matching on the device (include/f3d_block_match.h, f3d_block_match, then f3d_block_match_solve): on a grid of nodes
    `step` voxels apart, the integer shift within `search` (one radius or (rx, ry, rz)) of `centre` (one int triple per node, default
    zero) that maximises the zero-normalised cross-correlation of the (2 window + 1)^3 window of `a` against `b`, refined to a sub-voxel
    peak.  Grey values are quantised to `bins` codes over range = (lo, hi), the finite minimum and maximum of `a` when None.  a, b:
    numpy [z, y, x] float32 of one shape.  Returns a BlockMatchNodes; nodes whose ZNCC is below min_zncc, or that found nothing, have
    NaN vectors (validate_displacement on the node grid repairs them, expand_nodes makes the field dense)."""
    fn = _block_match_entry()
    find = _value_range_entry() if range is None else None
    bounds = None if range is None else _bin_range(range)
    with _on_device([a, b], "a and b must be two [z, y, x] volumes of one shape") as (box, p, dims):
        grid = block_match_grid(dims, step, window, search, origin, counts)
        nodes = grid.nx * grid.ny * grid.nz
        centre = _centre_array(centre, nodes)
        box.set_current()
        if bounds is None:
            lo, hi, found = C.c_float(), C.c_float(), RangeInfo()
            check(find(p[0], 0, *dims, C.byref(lo), C.byref(hi), C.byref(found)), "f3d_value_range")
            if found.finite == 0 or not lo.value < hi.value:
                raise ValueError("frame 0 has no two finite values: there is no range to lay the codes over")
            bounds = (lo.value, hi.value)
        records, info = np.zeros((nodes, BLOCK_MATCH_RECORD_WORDS), np.int32), BlockMatchInfo()
        check(fn(p[0], p[1], bounds[0], bounds[1], int(bins), *dims, C.byref(grid), None if centre is None else centre.ctypes.data,
                 records.ctypes.data, C.byref(info)), "f3d_block_match")
    rows, summary = solve_block_match(records, grid, centre, min_zncc)
    return BlockMatchNodes(rows, records, info.as_dict(), summary, grid, centre)


def expand_nodes(u, v, w, origin, step, dims):
    """Node vectors to a dense field on the device (include/f3d_block_match.h, f3d_expand_nodes): u, v, w numpy [nz, ny, nx] float32,
    node (i, j, k) at origin + step * (i, j, k); dims = (w, h, d) of the field.  Trilinear between the nodes, held constant outside
    their hull, NaN wherever a NaN node takes part.  Returns three [d, h, w] float32 volumes."""
    fn = _expand_nodes_entry()
    held = [_f32(c) for c in (u, v, w)]
    if any(a.ndim != 3 or a.shape != held[0][0].shape for a, _ in held):
        raise ValueError("u, v and w must be three [nz, ny, nx] arrays of one shape")
    nz, ny, nx = held[0][0].shape
    w_, h_, d_ = (int(n) for n in dims)
    previous = Size4()
    check(hip().f3d_get_container(C.byref(previous)), "f3d_get_container")
    box = Containers(w_, h_, d_)
    try:
        outs = [box.alloc() for _ in range(3)]
        box.set_current()
        check(fn(held[0][1], held[1][1], held[2][1], int(origin[0]), int(origin[1]), int(origin[2]), int(step), nx, ny, nz, *outs,
                 w_, h_, d_), "f3d_expand_nodes")
        return tuple(box.download(o, (w_, h_, d_)) for o in outs)
    finally:
        if previous.pitch:
            hip().f3d_set_container(C.byref(previous))
        box.free()


def block_match_initial(a, b, validate=True, **kw):
    """The dense guess of a pair for compute(initial=...): block_match(a, b, **kw), the node vectors through validate_displacement in
    replace mode with its defaults (the node grid is a small volume: outliers and the NaN nodes get their neighbours' median), then
    expand_nodes over the volume.  Returns ((u, v, w), nodes).  Voxels a NaN node still reaches are NaN; set_initial starts them from
    zero and counts them."""
    nodes = block_match(a, b, **kw)
    u, v, w = nodes.u, nodes.v, nodes.w
    if validate:
        d = validate_displacement(u, v, w, mode="replace", fields=("d",))
        u, v, w = d["u"], d["v"], d["w"]
    shape = np.asarray(a).shape
    return expand_nodes(u, v, w, nodes.origin, nodes.step, shape[::-1]), nodes


def _subset_match_entry():
    return _entry("f3d_subset_match", [_dp, _dp, _sz, _sz, _sz, C.POINTER(SubsetGrid), C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                       C.c_void_p, C.POINTER(SubsetInfo)], "correlate subsets of two frames")


def subset_grid(dims, step=16, window=8, origin=None, counts=None):
    """The node grid of subset_match over a (w, h, d) volume as a SubsetGrid: nodes `step` apart whose (2 window + 1)^3 windows and one
    voxel round them (the central differences) lie inside the volume, as many as fit and centred (f3d_subset_match_layout lays the
    same), unless origin = (ox, oy, oz) and / or counts = (nx, ny, nz) say otherwise.  ValueError when a window leaves the volume."""
    step, window = int(step), int(window)
    if step < 1 or not 1 <= window <= 8:
        raise ValueError("step must be at least 1 and window 1 .. 8")
    reach = window + 1
    first, count = [], []
    for axis, n in enumerate(dims):
        room = int(n) - 1 - 2 * reach
        if room < 0:
            raise ValueError(f"a window of radius {window} and a voxel round it leave the volume along {'xyz'[axis]} ({n} voxels)")
        o = reach + (room % step) // 2 if origin is None else int(origin[axis])
        c = (int(n) - 1 - reach - o) // step + 1 if counts is None else int(counts[axis])
        if o < reach or c < 1 or o + (c - 1) * step + reach > int(n) - 1:
            raise ValueError(f"a window of radius {window} leaves the volume along {'xyz'[axis]}: origin {o}, {c} nodes, step {step}")
        first.append(o)
        count.append(c)
    return SubsetGrid(*first, step, *count, window)


class SubsetNodes:
    """The node table of subset_match: `rows`, one SUBSET_NODE record per node (x fastest); `records`, the SUBSET_RECORD records of
    f3d_subset_match they were made from; `info` and `summary`, the dicts of f3d_subset_match_info and f3d_subset_match_summary; `grid`
    (SubsetGrid).  u, v, w, zncc, status, iterations are [nz, ny, nx] arrays; `grad` is the nine gradients (ux, uy, uz, vx, ..., wz) as
    [nz, ny, nx] float32 arrays, the list principal_from_gradient and polar_from_gradient take; diff the three of compare - subset."""

    def __init__(self, rows, records, info, summary, grid):
        self.rows, self.records, self.info, self.summary, self.grid = rows, records, info, summary, grid
        self.origin, self.step, self.counts = (grid.ox, grid.oy, grid.oz), grid.step, (grid.nx, grid.ny, grid.nz)

    def __len__(self):
        return len(self.rows)

    def _component(self, name):
        return np.ascontiguousarray(self.rows[name].reshape(self.counts[::-1]))

    u = property(lambda self: self._component("u"))
    v = property(lambda self: self._component("v"))
    w = property(lambda self: self._component("w"))
    zncc = property(lambda self: self._component("zncc"))
    status = property(lambda self: self._component("status"))
    iterations = property(lambda self: self._component("iterations"))
    grad = property(lambda self: [np.ascontiguousarray(self.rows["grad"][:, k].reshape(self.counts[::-1])) for k in range(9)])
    diff = property(lambda self: [np.ascontiguousarray(self.rows["diff"][:, k].reshape(self.counts[::-1])) for k in range(3)])

    def as_table(self):
        return [dict(x=int(r["position"][0]), y=int(r["position"][1]), z=int(r["position"][2]), status=SUBSET_STATUS[int(r["status"])],
                     iterations=int(r["iterations"]), zncc=float(r["zncc"]), u=float(r["u"]), v=float(r["v"]), w=float(r["w"]),
                     grad=tuple(float(g) for g in r["grad"]), diff=tuple(float(d) for d in r["diff"])) for r in self.rows]


def subset_table(records, grid, min_zncc=0.8, compare=None):
    """f3d_subset_match_table (include/f3d_host.h) of SUBSET_RECORD records: -> (rows as SUBSET_NODE records, summary dict).  compare:
    three arrays of one float32 per node, a displacement to hold the subsets against.  Host code, no device needed."""
    nodes = grid.nx * grid.ny * grid.nz
    records = np.ascontiguousarray(records, dtype=SUBSET_RECORD)
    if records.shape != (nodes,):
        raise ValueError(f"records must be {nodes} SUBSET_RECORD records")
    held = None
    if compare is not None:
        held = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in compare]
        if len(held) != 3 or any(c.size != nodes for c in held):
            raise ValueError(f"compare must be three arrays of {nodes} node values")
    pointers = None if held is None else (_fp * 3)(*[c.ctypes.data_as(_fp) for c in held])
    rows, summary = np.zeros(nodes, SUBSET_NODE), SubsetSummary()
    _host_check(host().f3d_subset_match_table(records.ctypes.data, C.byref(grid), float(min_zncc), pointers, rows.ctypes.data,
                                              C.byref(summary)), "f3d_subset_match_table")
    return rows, summary.as_dict()


def _subset_start(start, nodes):
    """start of subset_match as [nodes, 12] binary64 or None: 12 values per node, or three node arrays (u, v, w: gradients zero)"""
    if start is None:
        return None
    # three node arrays are three entries of `nodes` values each; a [3, 12] list for three nodes has 12 values per entry
    if isinstance(start, (tuple, list)) and len(start) == 3 and all(np.size(c) == nodes for c in start):
        full = np.zeros((nodes, 12), np.float64)
        for k, c in enumerate(start):
            c = np.asarray(c, dtype=np.float64).reshape(-1)
            if c.size != nodes:
                raise ValueError(f"start must hold one value per node, {nodes} of them, in each of u, v, w")
            full[:, 4 * k] = c
        return full
    start = np.ascontiguousarray(start, dtype=np.float64)
    if start.size != 12 * nodes:
        raise ValueError(f"start must hold 12 parameters per node, {nodes} nodes, or be three node arrays (u, v, w)")
    return start.reshape(nodes, 12)


def subset_match(a, b, grid=None, start=None, model="affine", max_iterations=20, tolerance=1e-3, reach=None, min_zncc=0.8, compare=None):
    """Subset correlation (local DVC) on the device (include/f3d_subset_match.h, f3d_subset_match, then f3d_subset_match_table): at
    every node of `grid` (a SubsetGrid, subset_grid(dims) when None) the displacement and, for model "affine", the displacement
    gradient that carry the (2 window + 1)^3 subset of `a` onto `b`, by inverse-compositional Gauss-Newton on the zero-normalised sum
    of squared differences with cubic interpolation of b, in binary64.  start: [nodes, 12] parameters (u, ux, uy, uz, v, ...), or three
    node arrays (u, v, w), or None for zero; a node with a NaN start is left out.  A node stops when its step is below `tolerance`
    (ok), after max_iterations, or when it has moved more than `reach` (the window radius when None) from its start.  a, b: numpy
    [z, y, x] float32 of one shape.  Returns a SubsetNodes: nodes that did not end ok with zncc >= min_zncc have NaN vectors; compare =
    (u, v, w) node arrays gives the difference to them and its rms, median and 95 % quantile in the summary."""
    fn = _subset_match_entry()
    if model not in SUBSET_MODELS:
        raise ValueError(f"model must be one of {sorted(SUBSET_MODELS)}")
    with _on_device([a, b], "a and b must be two [z, y, x] volumes of one shape") as (box, p, dims):
        if grid is None:
            grid = subset_grid(dims)
        nodes = grid.nx * grid.ny * grid.nz
        start = _subset_start(start, nodes)
        box.set_current()
        records, info = np.zeros(nodes, SUBSET_RECORD), SubsetInfo()
        check(fn(p[0], p[1], *dims, C.byref(grid), SUBSET_MODELS[model], None if start is None else start.ctypes.data, int(max_iterations),
                 float(tolerance), float(grid.window if reach is None else reach), records.ctypes.data, C.byref(info)), "f3d_subset_match")
    rows, summary = subset_table(records, grid, min_zncc, compare)
    return SubsetNodes(rows, records, info.as_dict(), summary, grid)


# the eight outputs of f3d_flow_strain in ABI order, and the F3D_STRAIN_* group of each
STRAIN_NAMES = ("vol", "exx", "eyy", "ezz", "exy", "exz", "eyz", "eq")
STRAIN_GROUPS = {"vol": 1, "e": 2, "eq": 4}
_STRAIN_GROUP_OF = (1, 2, 2, 2, 2, 2, 2, 4)
# the seventeen outputs of f3d_window_strain in ABI order, and the F3D_STRAIN_* / F3D_WSTRAIN_G group of each
WINDOW_STRAIN_NAMES = STRAIN_NAMES + ("G00", "G01", "G02", "G10", "G11", "G12", "G20", "G21", "G22")
WINDOW_STRAIN_GROUPS = {"vol": 1, "e": 2, "eq": 4, "grad": 8}
_WINDOW_STRAIN_GROUP_OF = _STRAIN_GROUP_OF + (8,) * 9
# the ten outputs of f3d_principal_strain in ABI order, and the F3D_PRINCIPAL_* group of each
PRINCIPAL_NAMES = ("e1", "e2", "e3", "gmax", "d1x", "d1y", "d1z", "d3x", "d3y", "d3z")
PRINCIPAL_GROUPS = {"val": 1, "shear": 2, "dir1": 4, "dir3": 8}
_PRINCIPAL_GROUP_OF = (1, 1, 1, 2, 4, 4, 4, 8, 8, 8)
# the seven outputs of f3d_polar_decomposition in ABI order, and the F3D_POLAR_* group of each
POLAR_NAMES = ("theta", "rx", "ry", "rz", "l1", "l2", "l3")
POLAR_GROUPS = {"angle": 1, "vector": 2, "stretch": 4}
_POLAR_GROUP_OF = (1, 2, 2, 2, 4, 4, 4)
# the four outputs of f3d_invert_displacement in ABI order, and the modes of f3d_carry_field
INVERSE_NAMES = ("gu", "gv", "gw", "err")
CARRY_MODES = {"linear": 1, "nearest": 2}


# the outputs of OpticalFlow.match in the order of f3d_flow_match_compute, and the F3D_MATCH_* bit of each; f3d_local_correlation
# stores the last two (F3D_CORRELATION_ZNCC, F3D_CORRELATION_RMSD)
MATCH_NAMES = ("warped", "zncc", "rmsd")
MATCH_GROUPS = {"warped": 1, "zncc": 2, "rmsd": 4}
CORRELATION_GROUPS = {"zncc": 1, "rmsd": 2}


# the models of f3d_motion_solve (F3D_MOTION_*)
MOTION_MODELS = {"translation": 0, "rigid": 1, "affine": 2}


def _motion_model(model):
    if model not in MOTION_MODELS:
        raise ValueError(f"unknown motion model {model!r} (one of {', '.join(MOTION_MODELS)})")
    return MOTION_MODELS[model]


# the outputs of f3d_validate_displacement in ABI order, the F3D_VALIDATE_* group of each, and its modes
VALIDATE_NAMES = ("r", "u", "v", "w")
VALIDATE_GROUPS = {"r": 1, "d": 2}
_VALIDATE_GROUP_OF = (1, 2, 2, 2)
VALIDATE_MODES = {"mark": 1, "replace": 2}


def _validate_mode(mode):
    if mode not in VALIDATE_MODES:
        raise ValueError(f"unknown validation mode {mode!r} (one of {', '.join(VALIDATE_MODES)})")
    return VALIDATE_MODES[mode]


def _strain_mask(fields):
    return _mask(fields, STRAIN_GROUPS, "strain")


def _window_strain_mask(fields):
    return _mask(fields, WINDOW_STRAIN_GROUPS, "window strain")


def _window_min_count(radius, min_count):
    """min_count of f3d_window_strain; None: a quarter of the (2 radius + 1)^3 window, at least 4"""
    return max(4, (2 * radius + 1) ** 3 // 4) if min_count is None else min_count


def _window_args(radius, min_count):
    """(radius, min_count) of a window call checked before anything touches the device: radius 1 .. 3, min_count (None:
    _window_min_count's default) 1 .. (2 radius + 1)^3"""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= 3:
        raise ValueError(f"radius must be 1, 2 or 3, not {radius!r}")
    radius = int(radius)
    count = _window_min_count(radius, min_count)
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 1 <= count <= (2 * radius + 1) ** 3:
        raise ValueError(f"min_count must be 1 .. {(2 * radius + 1) ** 3} at radius {radius}, not {min_count!r}")
    return radius, int(count)


def _principal_mask(fields):
    return _mask(fields, PRINCIPAL_GROUPS, "principal strain")


def _polar_mask(fields):
    return _mask(fields, POLAR_GROUPS, "rotation")


def _carry_mode(mode):
    if mode not in CARRY_MODES:
        raise ValueError(f"unknown carry mode {mode!r} (one of {', '.join(CARRY_MODES)})")
    return CARRY_MODES[mode]


def _grouped_fields(fn, what, u, v, w, mask, names, group_of, stats):
    """f3d_flow_strain / f3d_principal_strain / f3d_polar_decomposition of (u, v, w) from anywhere: a dict name -> array of the
    outputs `mask` selects, plus "stats" -> dict"""
    with _on_device((u, v, w), "u, v and w must be three [z, y, x] volumes of one shape") as (box, p, dims):
        outs = [box.alloc() if mask & g else 0 for g in group_of]
        box.set_current()
        check(fn(*p, (_dp * len(outs))(*outs), mask, *dims, C.byref(stats)), what)
        res = {n: box.download(o, dims) for n, o in zip(names, outs) if o}
    res["stats"] = stats.as_dict()
    return res


def flow_strain(u, v, w, fields=("vol", "e", "eq")):
    """Strain fields of a displacement on the device (include/f3d.h, f3d_flow_strain) for volumes from anywhere: u, v, w numpy
    [z, y, x] float32 in voxel units (a pair's flow, a cumulative displacement, the out-of-core or z-slab drivers' results when they
    fit on one device).  fields: groups "vol" (J - 1), "e" (Green-Lagrange exx .. eyz), "eq" (equivalent strain).  Returns a dict
    name -> array for the selected outputs and "stats" -> dict (defined, folded, vol_min, vol_max, eq_max, vol_sum)."""
    fn = _strain_entry()
    return _grouped_fields(fn, "f3d_flow_strain", u, v, w, _strain_mask(fields), STRAIN_NAMES, _STRAIN_GROUP_OF, StrainStats())


def window_strain(u, v, w, radius=2, min_count=None, fields=("vol", "e", "eq")):
    """Strain fields of a displacement over a strain window on the device (include/f3d.h, f3d_window_strain) for volumes from
    anywhere: the gradient of a voxel is the slope of the least-squares plane through the present samples of its (2 radius + 1)^3
    neighbourhood (radius 1 .. 3); a voxel with fewer than min_count of them (None: a quarter of the window, at least 4), or with
    all of them in one plane, is undefined.  fields: the groups of flow_strain() and "grad", the nine entries G00 .. G22 of the
    gradient.  Returns a dict name -> array for the selected outputs and "stats" -> dict (defined, folded, lost, thin, vol_min,
    vol_max, eq_max, vol_sum)."""
    fn = _window_strain_entry()
    mask, stats = _window_strain_mask(fields), WindowStrainStats()
    with _on_device((u, v, w), "u, v and w must be three [z, y, x] volumes of one shape") as (box, p, dims):
        outs = [box.alloc() if mask & g else 0 for g in _WINDOW_STRAIN_GROUP_OF]
        box.set_current()
        check(fn(*p, (_dp * len(outs))(*outs), mask, radius, _window_min_count(radius, min_count), *dims, C.byref(stats)),
              "f3d_window_strain")
        res = {n: box.download(o, dims) for n, o in zip(WINDOW_STRAIN_NAMES, outs) if o}
    res["stats"] = stats.as_dict()
    return res


def principal_strain(u, v, w, fields=("val", "shear")):
    """Principal strains of a displacement on the device (include/f3d.h, f3d_principal_strain) for volumes from anywhere: u, v, w
    numpy [z, y, x] float32 in voxel units.  fields: groups "val" (e1 >= e2 >= e3 of the Green-Lagrange tensor), "shear"
    (gmax = (e1 - e3) / 2), "dir1" / "dir3" (unit directions of e1 / e3 as d1x d1y d1z / d3x d3y d3z).  Returns a dict name -> array
    for the selected outputs and "stats" -> dict (defined, e1_max, e3_min, shear_max)."""
    fn = _principal_entry()
    return _grouped_fields(fn, "f3d_principal_strain", u, v, w, _principal_mask(fields), PRINCIPAL_NAMES, _PRINCIPAL_GROUP_OF,
                           PrincipalStats())


def polar_decomposition(u, v, w, fields=("angle", "vector", "stretch")):
    """Local rotation and principal stretches of a displacement on the device (include/f3d.h, f3d_polar_decomposition) for volumes
    from anywhere: u, v, w numpy [z, y, x] float32 in voxel units.  fields: groups "angle" (theta, radians, of the R of F = R U),
    "vector" (the rotation vector theta * axis as rx ry rz), "stretch" (l1 >= l2 >= l3, the principal stretches; np.log of them
    are the Hencky strains).  Returns a dict name -> array for the selected outputs (NaN where the voxel is undefined or folded)
    and "stats" -> dict (defined, folded, theta_max, l1_max, l3_min, theta_sum)."""
    fn = _polar_entry()
    return _grouped_fields(fn, "f3d_polar_decomposition", u, v, w, _polar_mask(fields), POLAR_NAMES, _POLAR_GROUP_OF, PolarStats())


GRADIENT_NAMES = WINDOW_STRAIN_NAMES[8:]
_GRADIENT_MISMATCH = "grad must be nine [z, y, x] volumes of one shape (G00 G01 G02 G10 G11 G12 G20 G21 G22) or a dict with those names"


def _gradient_volumes(grad):
    """the nine entries of `grad` in ABI order as contiguous float32 [z, y, x] arrays of one shape: from a sequence of nine, or by
    name from the dict window_strain(..., fields=(..., "grad")) returns"""
    if isinstance(grad, dict):
        missing = [n for n in GRADIENT_NAMES if n not in grad]
        if missing:
            raise ValueError(f"grad has no {', '.join(missing)}: {_GRADIENT_MISMATCH}")
        grad = [grad[n] for n in GRADIENT_NAMES]
    try:
        vols = [np.ascontiguousarray(a, dtype=np.float32) for a in grad]
    except (TypeError, ValueError):
        raise ValueError(_GRADIENT_MISMATCH) from None
    if len(vols) != 9 or any(a.ndim != 3 or a.shape != vols[0].shape for a in vols):
        raise ValueError(_GRADIENT_MISMATCH)
    return vols


def _from_gradient(fn, what, box, grad_ptrs, dims, mask, names, group_of, stats):
    """the from-gradient entry `fn` on nine containers of `box` into fresh ones: a dict name -> array of the outputs `mask` selects,
    plus "stats" -> dict"""
    outs = [box.alloc() if mask & g else 0 for g in group_of]
    box.set_current()
    check(fn((_dp * 9)(*grad_ptrs), (_dp * len(outs))(*outs), mask, *dims, C.byref(stats)), what)
    res = {n: box.download(o, dims) for n, o in zip(names, outs) if o}
    res["stats"] = stats.as_dict()
    return res


def principal_from_gradient(grad, fields=("val", "shear")):
    """Principal strains of a stored displacement gradient on the device (include/f3d.h, f3d_principal_from_gradient): grad is a
    sequence of nine [z, y, x] arrays G00 G01 G02 G10 G11 G12 G20 G21 G22 (row = component u v w, column = axis x y z) or the dict
    window_strain(..., fields=(..., "grad")) returns -- or a gradient from anywhere else, an FE solution, a filter of your own.  A
    voxel with a NaN in any entry is undefined.  fields and the result as for principal_strain()."""
    mask, vols = _principal_mask(fields), _gradient_volumes(grad)
    fn = _principal_from_gradient_entry()
    with _on_device(vols, _GRADIENT_MISMATCH) as (box, p, dims):
        return _from_gradient(fn, "f3d_principal_from_gradient", box, p, dims, mask, PRINCIPAL_NAMES, _PRINCIPAL_GROUP_OF, PrincipalStats())


def polar_from_gradient(grad, fields=("angle", "vector", "stretch")):
    """Local rotation and principal stretches of a stored displacement gradient on the device (include/f3d.h,
    f3d_polar_from_gradient): grad as for principal_from_gradient(), fields and the result as for polar_decomposition()."""
    mask, vols = _polar_mask(fields), _gradient_volumes(grad)
    fn = _polar_from_gradient_entry()
    with _on_device(vols, _GRADIENT_MISMATCH) as (box, p, dims):
        return _from_gradient(fn, "f3d_polar_from_gradient", box, p, dims, mask, POLAR_NAMES, _POLAR_GROUP_OF, PolarStats())


def _window_then(fn, what, u, v, w, radius, min_count, mask, names, group_of, stats):
    """one upload of (u, v, w), f3d_window_strain's gradient alone into nine containers, then the from-gradient entry `fn` on them:
    nothing comes back to the host in between"""
    window = _window_strain_entry()
    with _on_device((u, v, w), "u, v and w must be three [z, y, x] volumes of one shape") as (box, p, dims):
        grad = [box.alloc() for _ in range(9)]
        box.set_current()
        check(window(*p, (_dp * 17)(*([0] * 8 + grad)), WINDOW_STRAIN_GROUPS["grad"], radius, min_count, *dims, None), "f3d_window_strain")
        return _from_gradient(fn, what, box, grad, dims, mask, names, group_of, stats)


def window_principal(u, v, w, radius=2, min_count=None, fields=("val", "shear")):
    """Principal strains of a displacement from its least-squares gradient over a strain window: window_strain()'s "grad" (radius,
    min_count as there) handed to principal_from_gradient() on the device.  White noise in (u, v, w) biases e1, e3 and gmax of
    principal_strain() upwards (the eigenvalues of a noisy tensor repel); the window's gradient carries a third (radius 1) to a
    twenty-fifth (radius 3) of that noise.  fields and the result as for principal_strain()."""
    mask, (radius, min_count) = _principal_mask(fields), _window_args(radius, min_count)
    fn = _principal_from_gradient_entry()
    return _window_then(fn, "f3d_principal_from_gradient", u, v, w, radius, min_count, mask, PRINCIPAL_NAMES, _PRINCIPAL_GROUP_OF,
                        PrincipalStats())


def window_rotation(u, v, w, radius=2, min_count=None, fields=("angle", "vector", "stretch")):
    """Local rotation and principal stretches of a displacement from its least-squares gradient over a strain window:
    window_strain()'s "grad" handed to polar_from_gradient() on the device.  radius, min_count as for window_strain(), fields and the
    result as for polar_decomposition()."""
    mask, (radius, min_count) = _polar_mask(fields), _window_args(radius, min_count)
    fn = _polar_from_gradient_entry()
    return _window_then(fn, "f3d_polar_from_gradient", u, v, w, radius, min_count, mask, POLAR_NAMES, _POLAR_GROUP_OF, PolarStats())


def invert_displacement(u, v, w, iterations=32, tolerance=1e-3):
    """The inverse of a displacement on the device (include/f3d.h, f3d_invert_displacement) for volumes from anywhere: u, v, w numpy
    [z, y, x] float32 in voxel units, the displacement of every voxel of frame 0 on frame 0's grid (a pair's flow, a cumulative
    displacement).  Returns (gu, gv, gw, err, stats): g on frame k's grid with g(y) = -d(y + g(y)) by at most `iterations` fixed-point
    steps per voxel, stopped where the round-trip residual is at most `tolerance`; err that residual of the stored g; NaN where the
    point leaves the volume; stats a dict (defined, unconverged, steps_sum, err_max)."""
    fn = _inverse_entry()
    with _on_device((u, v, w), "u, v and w must be three [z, y, x] volumes of one shape") as (box, p, dims):
        outs = [box.alloc() for _ in INVERSE_NAMES]
        box.set_current()
        stats = InverseStats()
        check(fn(*p, *outs, *dims, iterations, tolerance, C.byref(stats)), "f3d_invert_displacement")
        return tuple(box.download(o, dims) for o in outs) + (stats.as_dict(),)


def carry_field(field, u, v, w, mode="linear"):
    """A field gathered through a displacement on the device (include/f3d.h, f3d_carry_field): out(x) = field(x + m(x)) with
    m = (u, v, w), all numpy [z, y, x] float32.  With m the inverse displacement it carries a frame-0 field onto frame k's grid, with
    m the displacement itself it brings a frame-k field back onto frame 0's.  mode "linear" (trilinear) or "nearest" (values copied bit
    for bit: labels).  Returns (out, lost): NaN where the point is outside the volume, and the number of NaN outputs."""
    fn = _carry_entry()
    m = _carry_mode(mode)
    with _on_device((field, u, v, w), "field, u, v and w must be four [z, y, x] volumes of one shape") as (box, p, dims):
        out = box.alloc()
        box.set_current()
        lost = C.c_ulonglong()
        check(fn(*p, out, *dims, m, C.byref(lost)), "f3d_carry_field")
        return box.download(out, dims), int(lost.value)


def local_correlation(a, b, radius=3, threshold=0.8, fields=("zncc", "rmsd")):
    """Per-voxel match quality of two volumes on one grid on the device (include/f3d.h, f3d_local_correlation): a, b numpy [z, y, x]
    float32, in practice frame 0 and frame 1 carried onto frame 0's grid (carry_field; NaN where the point left the volume).  Over the
    (2 radius + 1)^3 window of every voxel, of the voxels present in both: "zncc" the zero-normalised cross-correlation (NaN where the
    window is flat), "rmsd" the RMS difference; both NaN where the voxel itself is absent.  radius 1 .. 4.  Returns a dict name -> array
    for the selected fields and "stats" -> dict (defined, lost, below = defined voxels with zncc < threshold, zncc_min, rmsd_max,
    zncc_sum)."""
    fn = _correlation_entry()
    mask = _mask(fields, CORRELATION_GROUPS, "correlation")
    with _on_device((a, b), "a and b must be two [z, y, x] volumes of one shape") as (box, p, dims):
        outs = [box.alloc() if mask & g else 0 for g in CORRELATION_GROUPS.values()]
        box.set_current()
        stats = CorrelationStats()
        check(fn(*p, (_dp * 2)(*outs), mask, radius, threshold, *dims, C.byref(stats)), "f3d_local_correlation")
        res = {n: box.download(o, dims) for n, o in zip(CORRELATION_GROUPS, outs) if o}
    res["stats"] = stats.as_dict()
    return res


def motion_sums(u, v, w, weight=None, weight_min=0.8):
    """The moment sums of a displacement on the device (include/f3d.h, f3d_motion_sums): u, v, w numpy [z, y, x] float32; weight
    (optional, same shape) masks the voxels with weight < weight_min or NaN out.  Returns a MotionSums (n, Sx, Sxx, Sd, Sxd, Sdd about
    the centre of the volume)."""
    fn, _ = _motion_entry()
    vols = (u, v, w) if weight is None else (u, v, w, weight)
    with _on_device(vols, "u, v, w and weight must be [z, y, x] volumes of one shape") as (box, p, dims):
        box.set_current()
        sums = MotionSums()
        check(fn(p[0], p[1], p[2], p[3] if weight is not None else 0, weight_min, *dims, C.byref(sums)), "f3d_motion_sums")
    return sums


def solve_motion(sums, dims, model="rigid"):
    """f3d_motion_solve (include/f3d_host.h; host code, no device): the MotionFit of `sums` taken over a (width, height, depth) volume"""
    fit = MotionFit()
    fit.centre[:] = [(n - 1) / 2 for n in dims]
    _host_check(host().f3d_motion_solve(C.byref(sums), _motion_model(model), C.byref(fit)), "f3d_motion_solve")
    return fit


def fit_motion(u, v, w, model="rigid", weight=None, weight_min=0.8):
    """The translation, rigid motion or affine map d ~ t + M (x - centre) that fits a displacement best (least squares over the voxels
    where u, v, w are not NaN and, with `weight`, weight >= weight_min): the sums on the device, the solve on the host.  Returns a
    MotionFit with .centre, .t, .matrix (3 x 3, rows = components), .n (voxels that took part), .rms_before and, for "rigid",
    .cos_angle and .axial; .as_dict() gives the same as plain Python."""
    _motion_model(model)
    d, h, w_ = np.shape(u)
    return solve_motion(motion_sums(u, v, w, weight, weight_min), (w_, h, d), model)


def remove_motion(u, v, w, fit):
    """A displacement with a fit taken out on the device (include/f3d.h, f3d_remove_motion): returns (ru, rv, rw, stats) with
    r = d - (t + M (x - centre)) per voxel, NaN where d is, and stats a dict (present, sum_sq, max_abs) of the residual."""
    _, fn = _motion_entry()
    with _on_device((u, v, w), "u, v and w must be three [z, y, x] volumes of one shape") as (box, p, dims):
        outs = [box.alloc() for _ in range(3)]
        box.set_current()
        stats = MotionResidual()
        check(fn(*p, *outs, C.byref(fit), *dims, C.byref(stats)), "f3d_remove_motion")
        return tuple(box.download(o, dims) for o in outs) + (stats.as_dict(),)


# the status of a label after solve_label_motion (F3D_LABEL_*)
LABEL_STATUS = ("ok", "empty", "small", "degenerate")
MAX_LABELS = 1 << 22


def _labels_as_float_bits(labels, n_labels):
    """(the bits of the int32 labels as a float32 volume for the upload, n_labels): labels is any integer array; values that do not fit
    int32 raise; n_labels None means labels.max()"""
    labels = np.asarray(labels)
    if labels.ndim != 3 or not (np.issubdtype(labels.dtype, np.integer) or labels.dtype == np.bool_):
        raise ValueError("labels must be a [z, y, x] volume of integers")
    if labels.dtype == np.bool_:
        labels = labels.astype(np.int32)
    if labels.size and (int(labels.min()) < -2 ** 31 or int(labels.max()) > 2 ** 31 - 1):
        raise ValueError("labels do not fit int32")
    if n_labels is None:
        n_labels = int(labels.max()) if labels.size else 0
    n_labels = int(n_labels)
    if not 1 <= n_labels <= MAX_LABELS:
        raise ValueError(f"n_labels must be 1 .. {MAX_LABELS}, not {n_labels}")
    return np.ascontiguousarray(labels, dtype=np.int32).view(np.float32), n_labels


def label_motion_sums(u, v, w, labels, n_labels=None, weight=None, weight_min=0.8):
    """The exact moment sums of every label of a segmentation on the device (include/f3d.h, f3d_label_motion_sums): u, v, w numpy
    [z, y, x] float32, labels an integer volume of the same shape (0 background, 1 .. n_labels the bodies, anything else ignored;
    n_labels None means labels.max()), weight as in motion_sums.  Returns (sums, info): a ctypes array of n_labels MotionSums about the
    centre of the volume (label L at index L - 1) and a dict of the voxel counts background, foreign, absent, out_of_range, used."""
    fn = _label_sums_entry()
    bits, n_labels = _labels_as_float_bits(labels, n_labels)
    vols = (u, v, w, bits) if weight is None else (u, v, w, bits, weight)
    with _on_device(vols, "u, v, w, labels and weight must be [z, y, x] volumes of one shape") as (box, p, dims):
        box.set_current()
        sums = (MotionSums * n_labels)()
        info = LabelInfo()
        check(fn(p[0], p[1], p[2], p[3], n_labels, p[4] if weight is not None else 0, weight_min, *dims, sums, C.byref(info)),
              "f3d_label_motion_sums")
    return sums, info.as_dict()


class LabelMotion:
    """The fit of every label (solve_label_motion): arrays over the labels, label L at index L - 1.  .status (0 ok, 1 empty, 2 small,
    3 degenerate: LABEL_STATUS), .n, .centre (N, 3: the centroid of an ok label), .t (N, 3: the motion of the body at its centroid),
    .matrix (N, 3, 3; rows = components), .cos_angle, .axial (N, 3) for the rigid model, .rms_before, and .rms_after (None until the
    motion has been removed: remove_label_motion fills it in).  .fits and .status_c are the C arrays f3d_remove_label_motion takes."""

    def __init__(self, fits, status, model):
        self.fits, self.status_c, self.model = fits, status, model
        n = len(fits)
        self.status = np.array(list(status), np.int32).reshape(n)
        self.n = np.array([f.n for f in fits], np.uint64)
        self.centre = np.array([list(f.centre) for f in fits], np.float64).reshape(n, 3)
        self.t = np.array([list(f.t) for f in fits], np.float64).reshape(n, 3)
        self.matrix = np.array([list(f.M) for f in fits], np.float64).reshape(n, 3, 3)
        self.cos_angle = np.array([f.cos_angle for f in fits], np.float64)
        self.axial = np.array([list(f.axial) for f in fits], np.float64).reshape(n, 3)
        self.rms_before = np.array([f.rms_before for f in fits], np.float64)
        self.rms_after = None

    def __len__(self):
        return len(self.fits)

    def as_table(self):
        """one dict per label: label, status (a word of LABEL_STATUS), n, centre, t, matrix, cos_angle, axial, rms_before, rms_after"""
        return [{"label": i + 1, "status": LABEL_STATUS[self.status[i]], "n": int(self.n[i]), "centre": self.centre[i].tolist(),
                 "t": self.t[i].tolist(), "matrix": self.matrix[i].tolist(), "cos_angle": float(self.cos_angle[i]),
                 "axial": self.axial[i].tolist(), "rms_before": float(self.rms_before[i]),
                 "rms_after": None if self.rms_after is None else float(self.rms_after[i])} for i in range(len(self))]


def solve_label_motion(sums, dims, model="rigid", min_voxels=27):
    """f3d_motion_solve_labels (include/f3d_host.h; host code, no device): the LabelMotion of the array `sums` of label_motion_sums taken
    over a (width, height, depth) volume.  A label with fewer than min_voxels voxels is not fitted."""
    n = len(sums)
    if not isinstance(sums, C.Array):
        sums = (MotionSums * n)(*sums)
    fits, status = (MotionFit * n)(), (C.c_int * n)()
    centre = (C.c_double * 3)(*[(k - 1) / 2 for k in dims])
    if int(min_voxels) < 0:
        raise ValueError("min_voxels must not be negative")
    _host_check(host().f3d_motion_solve_labels(sums, n, _motion_model(model), int(min_voxels), centre, fits, status),
                "f3d_motion_solve_labels")
    return LabelMotion(fits, status, model)


def fit_label_motion(u, v, w, labels, model="rigid", n_labels=None, min_voxels=27, weight=None, weight_min=0.8):
    """The translation, rigid motion or affine map of every label of a segmentation (least squares over the label's voxels that take
    part, the displacement quantised to 2^-14 voxel): the exact sums on the device, the solves on the host.  Returns a LabelMotion;
    .info holds the voxel counts of label_motion_sums."""
    _motion_model(model)
    d, h, w_ = np.shape(u)
    sums, info = label_motion_sums(u, v, w, labels, n_labels, weight, weight_min)
    motion = solve_label_motion(sums, (w_, h, d), model, min_voxels)
    motion.info = info
    return motion


def remove_label_motion(u, v, w, labels, motion):
    """A displacement with the fit of each voxel's label taken out on the device (include/f3d.h, f3d_remove_label_motion): returns
    (ru, rv, rw, stats); NaN where the label is background, foreign or not fitted.  motion.rms_after receives the rms of the residual
    of every label (NaN where there is none), from a second f3d_label_motion_sums of the residual."""
    fn = _label_remove_entry()               # the entry this call is named after first: a library without it is reported by that name
    sums_fn = _label_sums_entry()
    n = len(motion)
    bits, n = _labels_as_float_bits(labels, n)
    with _on_device((u, v, w, bits), "u, v, w and labels must be [z, y, x] volumes of one shape") as (box, p, dims):
        outs = [box.alloc() for _ in range(3)]
        box.set_current()
        stats = MotionResidual()
        check(fn(*p, n, motion.fits, motion.status_c, *outs, *dims, C.byref(stats)), "f3d_remove_label_motion")
        after = (MotionSums * n)()
        check(sums_fn(*outs, p[3], n, 0, 0.0, *dims, after, None), "f3d_label_motion_sums")
        res = tuple(box.download(o, dims) for o in outs)
    with np.errstate(invalid="ignore", divide="ignore"):
        motion.rms_after = np.array([np.sqrt(((s.Sdd[0] + s.Sdd[1]) + s.Sdd[2]) / s.n) if s.n else np.nan for s in after], np.float64)
    return res + (stats.as_dict(),)


MAX_CONTACTS = 1 << 24
# the bits of the status of a contact after contact_kinematics (F3D_CONTACT_*)
CONTACT_STATUS = {"small": 1, "flat": 2, "nojump": 4, "unfitted": 8}
_CONTACT_DTYPE = np.dtype([("lo", "<i4"), ("hi", "<i4"), ("faces", "<u8", 3), ("area", "<i8", 3), ("c2", "<i8", 3), ("n_jump", "<u8"),
                           ("J", "<i8", 3)])
_KINEMATICS_DTYPE = np.dtype([("point", "<f8", 3), ("area", "<f8"), ("normal", "<f8", 3), ("jump_normal", "<f8"), ("jump_slip", "<f8"),
                              ("fit_normal", "<f8"), ("fit_slip", "<f8"), ("status", "<u4"), ("pad", "<u4")])


class Contacts:
    """The contacts between the bodies of a segmentation (label_contacts): arrays over the contacts, sorted by (lo, hi).  .lo, .hi (the
    labels, lo < hi), .faces (N, 3: faces per axis), .area_vector (N, 3: the signed face count per axis, pointing from lo to hi), .c2
    (N, 3: the sums of the doubled face-centre coordinates about the volume centre), .n_jump, .J (N, 3: the summed displacement jump hi
    minus lo in units of 2^-14 voxel), all exact integers, and .info, the dict of f3d_contact_info.  .rows is the C array
    f3d_contact_kinematics takes."""

    def __init__(self, rows, count, info):
        self.rows, self.info = rows, info
        table = np.frombuffer(rows, dtype=_CONTACT_DTYPE, count=count) if count else np.zeros(0, _CONTACT_DTYPE)
        self.lo, self.hi = table["lo"].copy(), table["hi"].copy()
        self.faces, self.area_vector, self.c2 = table["faces"].copy(), table["area"].copy(), table["c2"].copy()
        self.n_jump, self.J = table["n_jump"].copy(), table["J"].copy()
        self.kinematics = None

    def __len__(self):
        return len(self.lo)

    def coordination(self, n_labels):
        """the number of contacts of every label, label L at index L - 1"""
        return (np.bincount(self.lo, minlength=n_labels + 1) + np.bincount(self.hi, minlength=n_labels + 1))[1:n_labels + 1]

    def as_table(self):
        """one dict per contact: lo, hi, faces, area_vector, c2, n_jump, J (Python integers)"""
        return [{"lo": int(self.lo[i]), "hi": int(self.hi[i]), "faces": self.faces[i].tolist(), "area_vector": self.area_vector[i].tolist(),
                 "c2": self.c2[i].tolist(), "n_jump": int(self.n_jump[i]), "J": self.J[i].tolist()} for i in range(len(self))]


def _contact_capacity(capacity, n_labels):
    """(the first capacity, whether to retry with twice the room): capacity None starts at 8 * n_labels, at most 2^20"""
    if capacity is None:
        return min(8 * n_labels, 1 << 20), True
    capacity = int(capacity)
    if not 1 <= capacity <= MAX_CONTACTS:
        raise ValueError(f"capacity must be 1 .. {MAX_CONTACTS}, not {capacity}")
    return capacity, False


def label_contacts(u, v, w, labels, n_labels=None, capacity=None):
    """The contacts between the bodies of a segmentation on the device (include/f3d.h, f3d_label_contacts): labels an integer [z, y, x]
    volume (0 background, 1 .. n_labels the bodies, anything else foreign; n_labels None means labels.max()), u, v, w numpy [z, y, x]
    float32 of the same shape, or all three None for the adjacency graph alone.  capacity is the room for distinct contacts: None
    starts at 8 * n_labels (at most 2^20) and doubles until the table is complete; a given capacity is tried once, and a Contacts with no rows and
    info["complete"] == 0 comes back when it does not suffice.  Returns a Contacts."""
    fn = _contacts_entry()
    given = [a is not None for a in (u, v, w)]
    if any(given) and not all(given):
        raise ValueError("u, v and w must be given all three or not at all")
    bits, n_labels = _labels_as_float_bits(labels, n_labels)
    capacity, retry = _contact_capacity(capacity, n_labels)
    vols = (u, v, w, bits) if all(given) else (bits,)
    with _on_device(vols, "u, v, w and labels must be [z, y, x] volumes of one shape") as (box, p, dims):
        box.set_current()
        d = p[:3] if all(given) else [0, 0, 0]
        while True:
            rows, info = (Contact * capacity)(), ContactInfo()
            check(fn(*d, p[-1], n_labels, *dims, capacity, rows, C.byref(info)), "f3d_label_contacts")
            if info.complete or not retry or capacity >= MAX_CONTACTS:
                break
            capacity = min(2 * capacity, MAX_CONTACTS)
    return Contacts(rows, int(info.n_contacts) if info.complete else 0, info.as_dict())


def contact_kinematics(contacts, dims, motion=None, min_faces=4):
    """f3d_contact_kinematics (include/f3d_host.h; host code, no device) of a Contacts found in a (width, height, depth) volume: a
    structured array with a row per contact of point (3), area, normal (3), jump_normal (positive: opening), jump_slip, fit_normal,
    fit_slip and status (bits of CONTACT_STATUS).  motion: the LabelMotion of the same labels for the fit columns, or None."""
    n = len(contacts)
    if int(min_faces) < 0:
        raise ValueError("min_faces must not be negative")
    if len(dims) != 3 or any(int(k) < 1 for k in dims):
        raise ValueError("dims must be (width, height, depth), all positive")
    out = (ContactKinematics * max(n, 1))()
    size = (_sz * 3)(*[int(k) for k in dims])
    fits, status, n_labels = (motion.fits, motion.status_c, len(motion)) if motion is not None else (None, None, 0)
    _host_check(host().f3d_contact_kinematics(contacts.rows, n, size, fits, status, n_labels, int(min_faces), out),
                "f3d_contact_kinematics")
    assert C.sizeof(ContactKinematics) == _KINEMATICS_DTYPE.itemsize
    return np.frombuffer(out, dtype=_KINEMATICS_DTYPE, count=n).copy() if n else np.zeros(0, _KINEMATICS_DTYPE)


_SHAPE_SUMS_DTYPE = np.dtype([("n", "<u8"), ("lo", "<i8", 3), ("hi", "<i8", 3), ("s1", "<u8", 3), ("s2", "<u8", 6), ("pairs", "<u8", 13),
                              ("squares", "<u8", 3), ("cubes", "<u8"), ("border", "<u8", 3)])
_SHAPE_DTYPE = np.dtype([("status", "<i4"), ("pad", "<i4"), ("voxels", "<u8"), ("box_lo", "<i8", 3), ("box_hi", "<i8", 3),
                         ("border", "<u8", 3), ("centroid", "<f8", 3), ("diameter", "<f8"), ("semi_axes", "<f8", 3), ("axes", "<f8", (3, 3)),
                         ("faces", "<u8"), ("surface", "<f8"), ("sphericity", "<f8"), ("euler", "<i8")])


def label_shape_sums(labels, n_labels=None):
    """The exact shape sums of every label of a segmentation on the device (include/f3d.h, f3d_label_shape_sums): labels an integer
    [z, y, x] volume (0 background, 1 .. n_labels the bodies, anything else foreign; n_labels None means labels.max()).  Returns
    (sums, info): a structured array of n_labels rows (label L at index L - 1) with the fields n, lo, hi, s1, s2, pairs, squares,
    cubes, border, and a dict of the voxel counts background, foreign, labelled."""
    fn = _label_shape_entry()
    bits, n_labels = _labels_as_float_bits(labels, n_labels)
    if bits.size == 0:
        raise ValueError("labels must be a non-empty [z, y, x] volume")
    with _on_device((bits,), "labels must be a [z, y, x] volume") as (box, p, dims):
        box.set_current()
        sums, info = (LabelShapeSums * n_labels)(), LabelShapeInfo()
        check(fn(p[0], n_labels, *dims, sums, C.byref(info)), "f3d_label_shape_sums")
    assert C.sizeof(LabelShapeSums) == _SHAPE_SUMS_DTYPE.itemsize
    return np.frombuffer(sums, dtype=_SHAPE_SUMS_DTYPE, count=n_labels).copy(), info.as_dict()


class LabelShapes:
    """The shape of every body of a segmentation (solve_label_shapes): arrays over the labels, label L at index L - 1.  .status (0 ok,
    1 empty: LABEL_STATUS), .voxels, .box (N, 2, 3: the smallest and the largest x, y, z), .border (N, 3: voxels on the two box faces
    of each axis), .centroid (N, 3), .diameter (of the ball of the same volume), .semi_axes (N, 3, descending: of the ellipsoid with the
    same second moments), .axes (N, 3, 3: axes[i, j] is unit axis j of label i), .faces (the staircase area), .surface (the
    Cauchy-Crofton estimate over 13 directions), .sphericity and .euler (pieces - tunnels + cavities under six-connectivity); .info is
    the dict of f3d_label_shape_info when the sums came from the device in the same call, else None."""

    def __init__(self, rows, info=None):
        self.rows, self.info = rows, info
        self.status, self.voxels = rows["status"].copy(), rows["voxels"].copy()
        self.box = np.stack([rows["box_lo"], rows["box_hi"]], axis=1) if len(rows) else np.zeros((0, 2, 3), np.int64)
        self.border, self.centroid, self.diameter = rows["border"].copy(), rows["centroid"].copy(), rows["diameter"].copy()
        self.semi_axes, self.axes = rows["semi_axes"].copy(), rows["axes"].copy()
        self.faces, self.surface, self.sphericity, self.euler = (rows[k].copy() for k in ("faces", "surface", "sphericity", "euler"))

    def __len__(self):
        return len(self.status)

    @property
    def touches_border(self):
        """per label: whether a voxel of it lies on a face of the box (the body may be cut by the edge of the scan)"""
        return self.border.sum(axis=1) > 0

    def as_table(self):
        """one dict per label: label, status (a word of LABEL_STATUS), voxels, box, border, touches_border, centroid, diameter, semi_axes,
        axes, faces, surface, sphericity, euler"""
        touches = self.touches_border
        return [{"label": i + 1, "status": LABEL_STATUS[self.status[i]], "voxels": int(self.voxels[i]), "box": self.box[i].tolist(),
                 "border": self.border[i].tolist(), "touches_border": bool(touches[i]), "centroid": self.centroid[i].tolist(),
                 "diameter": float(self.diameter[i]), "semi_axes": self.semi_axes[i].tolist(), "axes": self.axes[i].tolist(),
                 "faces": int(self.faces[i]), "surface": float(self.surface[i]), "sphericity": float(self.sphericity[i]),
                 "euler": int(self.euler[i])} for i in range(len(self))]


def _shape_rows(out, n):
    assert C.sizeof(LabelShape) == _SHAPE_DTYPE.itemsize
    return np.frombuffer(out, dtype=_SHAPE_DTYPE, count=n).copy() if n else np.zeros(0, _SHAPE_DTYPE)


def solve_label_shapes(sums):
    """f3d_label_shape_solve (include/f3d_host.h; host code, no device): the LabelShapes of the structured array `sums` of
    label_shape_sums."""
    sums = np.ascontiguousarray(sums, dtype=_SHAPE_SUMS_DTYPE)
    if sums.ndim != 1:
        raise ValueError("sums must be a one-dimensional array of shape sums, one row per label")
    n = len(sums)
    out = (LabelShape * max(n, 1))()
    _host_check(host().f3d_label_shape_solve(sums.ctypes.data_as(C.POINTER(LabelShapeSums)), n, out), "f3d_label_shape_solve")
    return LabelShapes(_shape_rows(out, n))


def label_shapes(labels, n_labels=None):
    """The shape table of a segmentation from anywhere: label_shape_sums on the device, solve_label_shapes on the host.  Returns a
    LabelShapes whose .info holds the voxel counts."""
    sums, info = label_shape_sums(labels, n_labels)
    shapes = solve_label_shapes(sums)
    shapes.info = info
    return shapes


MAX_LABEL_FIELD_BINS = 256
MAX_LABEL_FIELD_COUNTS = 1 << 26
_FIELD_SUMS_DTYPE = np.dtype([("n", "<u8"), ("min_key", "<u8"), ("max_key", "<u8"), ("iq", "<i8"), ("iqq_lo", "<u8"), ("iqq_hi", "<u8"),
                              ("below", "<u8"), ("above", "<u8")])
_FIELD_STAT_DTYPE = np.dtype([("status", "<i4"), ("q05_bin", "<i4"), ("median_bin", "<i4"), ("q95_bin", "<i4"), ("n", "<u8"),
                              ("below", "<u8"), ("above", "<u8"), ("min", "<f8"), ("max", "<f8"), ("mean", "<f8"), ("variance", "<f8"),
                              ("std", "<f8"), ("q05", "<f8"), ("median", "<f8"), ("q95", "<f8")])


def _field_bins(bins):
    if int(bins) != bins or not 0 <= int(bins) <= MAX_LABEL_FIELD_BINS:
        raise ValueError(f"bins must be an integer in 0 .. {MAX_LABEL_FIELD_BINS}, not {bins}")
    return int(bins)


def _field_shift(shift):
    if shift is None:
        return None
    if int(shift) != shift or not -100 <= int(shift) <= 100:
        raise ValueError(f"shift must be an integer in -100 .. 100, not {shift}")
    return int(shift)


def label_field_shift(lo, hi, finite=1):
    """f3d_label_field_shift (include/f3d_host.h; host code): the shift for a field whose finite values lie in [lo, hi]: with
    max(|lo|, |hi|) = f * 2^e (frexp) it is 24 - e clamped to -100 .. 100, and 0 when that is 0 or nothing is finite."""
    return int(host().f3d_label_field_shift(float(np.float32(lo)), float(np.float32(hi)), int(finite)))


def _bin_scale_is_finite(lo, hi, bins):
    """whether f3d_histogram's scale (float)bins / (hi - lo) is finite and positive in float32"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        width = np.float32(hi) - np.float32(lo)
        scale = np.float32(bins) / width
    return bool(np.isfinite(width) and width > 0 and np.isfinite(scale) and scale > 0)


def _field_settings(shift, bins, bounds, lo, hi, finite):
    """(shift, bins, bounds, note) with what the caller left open taken from the field's finite range [lo, hi] under the labels"""
    note = None
    if shift is None:
        shift = label_field_shift(lo, hi, finite)
    if bins and bounds is None:
        if finite == 0:
            bins, note = 0, "no bins: the field has no finite voxel under the labels, so there is no range to lay them over"
        elif not lo < hi:
            bins, note = 0, f"no bins: the field is constant ({lo}) under the labels, so there is no range to lay them over"
        elif not _bin_scale_is_finite(lo, hi, bins):
            bins, note = 0, f"no bins: the width of the field's range [{lo}, {hi}] or the scale of {bins} bins over it is not finite in float32"
        else:
            bounds = (float(lo), float(hi))
    return shift, bins, bounds, note


class LabelFieldSums:
    """What f3d_label_field_sums gave (label_field_sums): .rows (a structured array over the labels, label L at index L - 1, with the
    fields n, min_key, max_key, iq, iqq_lo, iqq_hi, below, above), .counts (uint32 [n_labels, bins], None without bins), .shift, .bins,
    .lo and .hi (the float32 bounds of the bins, None without), and .info: the dict of f3d_label_field_info, with a "note" when bins
    were asked for and the field had no range to lay them over."""

    def __init__(self, rows, counts, shift, lo, hi, info):
        self.rows, self.counts, self.shift, self.lo, self.hi, self.info = rows, counts, int(shift), lo, hi, info
        self.bins = 0 if counts is None else counts.shape[1]

    def __len__(self):
        return len(self.rows)


def _field_sums_result(rows, n_labels, counts, shift, bounds, info, note):
    assert C.sizeof(LabelFieldSumsRow) == _FIELD_SUMS_DTYPE.itemsize
    found = info.as_dict()
    if note:
        found["note"] = note
    return LabelFieldSums(np.frombuffer(rows, dtype=_FIELD_SUMS_DTYPE, count=n_labels).copy(), counts, shift,
                          None if counts is None else bounds[0], None if counts is None else bounds[1], found)


def label_field_sums(field, labels, n_labels=None, shift=None, bins=0, range=None):
    """The exact sums of a scalar field over every label of a segmentation on the device (include/f3d.h, f3d_label_field_sums): field a
    [z, y, x] volume (taken as float32), labels an integer volume of its shape (0 background, 1 .. n_labels the bodies, anything else
    foreign; n_labels None means labels.max()).  shift: the quantisation q = rint(s * 2^shift), -100 .. 100; None picks
    label_field_shift of value_range(field, mask=labels), with which nothing finite is out of range.  bins 0 .. 256 over range =
    (lo, hi); range None takes that finite range, and a field that has none (constant, or nothing finite) gets bins = 0 and a note in
    .info.  Returns a LabelFieldSums."""
    fn, bins, shift = _label_field_entry(), _field_bins(bins), _field_shift(shift)
    bounds = None if range is None else _bin_range(range)
    field = np.asarray(field)
    if field.ndim != 3 or field.size == 0:
        raise ValueError("field must be a non-empty [z, y, x] volume")
    bits, n_labels = _labels_as_float_bits(labels, n_labels)
    if bits.shape != field.shape:
        raise ValueError(f"labels must have the shape of the field, {field.shape}")
    if n_labels * bins > MAX_LABEL_FIELD_COUNTS:
        raise ValueError(f"n_labels * bins must be at most 2^26, not {n_labels} * {bins}")
    open_ = shift is None or (bins and bounds is None)
    find = _value_range_entry() if open_ else None
    note = None
    with _on_device((field, bits), "field and labels must be [z, y, x] volumes of one shape") as (box, p, dims):
        box.set_current()
        if open_:
            lo, hi, found = C.c_float(), C.c_float(), RangeInfo()
            check(find(p[0], p[1], *dims, C.byref(lo), C.byref(hi), C.byref(found)), "f3d_value_range")
            shift, bins, bounds, note = _field_settings(shift, bins, bounds, lo.value, hi.value, found.finite)
        rows, info = (LabelFieldSumsRow * n_labels)(), LabelFieldInfo()
        counts = np.zeros((n_labels, bins), np.uint32) if bins else None
        lo_hi = bounds if bins else (0.0, 0.0)
        check(fn(p[0], p[1], n_labels, shift, lo_hi[0], lo_hi[1], bins, *dims, rows,
                 counts.ctypes.data_as(C.POINTER(C.c_uint)) if bins else None, C.byref(info)), "f3d_label_field_sums")
    return _field_sums_result(rows, n_labels, counts, shift, bounds, info, note)


class LabelFieldStats:
    """The statistics of a scalar field per body (solve_label_field): arrays over the labels, label L at index L - 1.  .status (0 ok,
    1 empty, 2 small: LABEL_STATUS), .n (the voxels that took part), .min, .max, .mean, .variance, .std (population), .q05, .median,
    .q95 (the midpoint of the bin that holds the rank; NaN without bins) and their bins .q05_bin, .median_bin, .q95_bin (-1 without),
    .below and .above (voxels outside the range of the bins), .counts (uint32 [n_labels, bins] or None), .shift, .lo, .hi, .bins, .info
    (the dict of f3d_label_field_info, with a "note" when bins were dropped) and .summary: ok, empty, small and mean, the n-weighted
    mean over the ok labels."""

    def __init__(self, rows, summary, sums):
        self.rows, self.summary = rows, summary
        for name in _FIELD_STAT_DTYPE.names:
            setattr(self, name, rows[name].copy())
        self.counts, self.info, self.shift, self.lo, self.hi, self.bins = sums.counts, sums.info, sums.shift, sums.lo, sums.hi, sums.bins

    def __len__(self):
        return len(self.status)

    def as_table(self):
        """one dict per label: label, status (a word of LABEL_STATUS), n, min, max, mean, std, q05, median, q95, below, above"""
        return [{"label": i + 1, "status": LABEL_STATUS[self.status[i]], "n": int(self.n[i]), "min": float(self.min[i]),
                 "max": float(self.max[i]), "mean": float(self.mean[i]), "std": float(self.std[i]), "q05": float(self.q05[i]),
                 "median": float(self.median[i]), "q95": float(self.q95[i]), "below": int(self.below[i]), "above": int(self.above[i])}
                for i in range(len(self))]


def _field_stats_result(out, n, summary, sums):
    assert C.sizeof(LabelFieldStat) == _FIELD_STAT_DTYPE.itemsize
    rows = np.frombuffer(out, dtype=_FIELD_STAT_DTYPE, count=n).copy() if n else np.zeros(0, _FIELD_STAT_DTYPE)
    return LabelFieldStats(rows, {"ok": int(summary.ok), "empty": int(summary.empty), "small": int(summary.small),
                                  "mean": float(summary.mean)}, sums)


def solve_label_field(sums, min_voxels=1):
    """f3d_label_field_solve (include/f3d_host.h; host code, no device): the LabelFieldStats of the LabelFieldSums `sums`; a label
    with fewer than min_voxels voxels is "small" (and still filled)."""
    if not isinstance(sums, LabelFieldSums):
        raise ValueError("sums must be the LabelFieldSums of label_field_sums")
    if int(min_voxels) != min_voxels or not 0 <= int(min_voxels) < 2 ** 64:
        raise ValueError(f"min_voxels must be a non-negative integer, not {min_voxels}")
    rows = np.ascontiguousarray(sums.rows, dtype=_FIELD_SUMS_DTYPE)
    n = len(rows)
    counts = None
    if sums.bins:
        counts = np.ascontiguousarray(sums.counts, dtype=np.uint32)
        if counts.shape != (n, sums.bins):
            raise ValueError(f"counts must be [n_labels, bins] = {(n, sums.bins)}, not {counts.shape}")
    out, summary = (LabelFieldStat * max(n, 1))(), LabelFieldSummary()
    _host_check(host().f3d_label_field_solve(rows.ctypes.data_as(C.POINTER(LabelFieldSumsRow)),
                                             counts.ctypes.data_as(C.POINTER(C.c_uint)) if sums.bins else None, n, sums.shift,
                                             sums.lo if sums.bins else 0.0, sums.hi if sums.bins else 0.0, sums.bins, int(min_voxels), out,
                                             C.byref(summary)), "f3d_label_field_solve")
    return _field_stats_result(out, n, summary, sums)


def label_field_stats(field, labels, n_labels=None, shift=None, bins=0, range=None, min_voxels=1):
    """The statistics of a scalar field per body from anywhere: label_field_sums on the device, solve_label_field on the host.
    Returns a LabelFieldStats."""
    return solve_label_field(label_field_sums(field, labels, n_labels, shift, bins, range), min_voxels)


def _paint_values(values):
    values = np.ascontiguousarray(values, dtype=np.float32)
    if values.ndim != 1 or not 1 <= values.size <= MAX_LABELS:
        raise ValueError(f"values must be a one-dimensional array of 1 .. {MAX_LABELS} numbers, the value of label l at index l - 1")
    return values


def paint_labels(values, labels):
    """A value per label painted into a volume on the device (include/f3d.h, f3d_paint_labels): a float32 [z, y, x] volume with
    values[l - 1] where labels == l in 1 .. len(values) (the bytes are copied: a NaN keeps its payload) and NaN elsewhere."""
    fn, values = _paint_entry(), _paint_values(values)
    bits, n = _labels_as_float_bits(labels, len(values))
    if bits.size == 0:
        raise ValueError("labels must be a non-empty [z, y, x] volume")
    with _on_device((bits,), "labels must be a [z, y, x] volume") as (box, p, dims):
        box.set_current()
        check(fn(p[0], n, values.ctypes.data_as(_fp), p[0], *dims), "f3d_paint_labels")   # in place: each voxel its own word
        return box.download(p[0], dims)


MAX_OVERLAPS = 1 << 24
# the bits of the status of a body after solve_overlaps (F3D_TRACK_*)
TRACK_STATUS = {"empty": 1, "matched": 2, "split": 4, "vanished": 8, "left": 16, "merged": 32, "appeared": 64}
_OVERLAP_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("n", "<u8"), ("ca2", "<i8", 3), ("cb2", "<i8", 3)])
_TRACK_A_DTYPE = np.dtype([("n", "<u8"), ("n_lost", "<u8"), ("n_background", "<u8"), ("n_best", "<u8"), ("best_b", "<i4"),
                           ("n_targets", "<i4"), ("fraction", "<f8"), ("shift", "<f8", 3), ("iou", "<f8"), ("status", "<u4"), ("pad", "<u4")])
_TRACK_B_DTYPE = np.dtype([("m", "<u8"), ("n_unreached", "<u8"), ("n_best", "<u8"), ("best_a", "<i4"), ("n_sources", "<i4"),
                           ("status", "<u4"), ("pad", "<u4")])


class Overlaps:
    """The overlap of two label volumes through a displacement (label_overlap): arrays over the pairs, sorted by (a, b).  .a, .b (the
    labels; b == -1 is the part of body a that left the volume, b == 0 the part that landed on background, a == 0 the part of body b
    nothing reached), .n (voxels), .ca2, .cb2 (N, 3: the sums of the doubled source and target coordinates about the volume centre),
    all exact integers, and .info, the dict of f3d_overlap_info.  .rows is the C array f3d_overlap_solve takes."""

    def __init__(self, rows, count, info):
        self.rows, self.info = rows, info
        table = np.frombuffer(rows, dtype=_OVERLAP_DTYPE, count=count) if count else np.zeros(0, _OVERLAP_DTYPE)
        self.a, self.b, self.n = table["a"].copy(), table["b"].copy(), table["n"].copy()
        self.ca2, self.cb2 = table["ca2"].copy(), table["cb2"].copy()

    def __len__(self):
        return len(self.a)

    def matrix(self, n_a=None, n_b=None):
        """the voxel counts as a mapping: {(a, b): n} without n_a and n_b, else a dense (n_a + 1, n_b + 2) uint64 array whose row is a
        and whose column is b + 1 (column 0 is what left the volume), for small numbers of bodies"""
        if n_a is None or n_b is None:
            return {(int(a), int(b)): int(n) for a, b, n in zip(self.a, self.b, self.n)}
        dense = np.zeros((int(n_a) + 1, int(n_b) + 2), np.uint64)
        dense[self.a, self.b + 1] = self.n
        return dense

    def as_table(self):
        """one dict per pair: a, b, n, ca2, cb2 (Python integers) and shift, (cb2 - ca2) / (2 n), None for b == -1"""
        return [{"a": int(self.a[i]), "b": int(self.b[i]), "n": int(self.n[i]), "ca2": self.ca2[i].tolist(), "cb2": self.cb2[i].tolist(),
                 "shift": None if self.b[i] < 0 else [(int(q) - int(p)) / (2 * int(self.n[i])) for p, q in zip(self.ca2[i], self.cb2[i])]}
                for i in range(len(self))]


def _overlap_capacity(capacity, n_a, n_b):
    """(the first capacity, whether to retry with twice the room): capacity None starts at 8 * (n_a + n_b), at most 2^20"""
    if capacity is None:
        return min(8 * (n_a + n_b), 1 << 20), True
    capacity = int(capacity)
    if not 1 <= capacity <= MAX_OVERLAPS:
        raise ValueError(f"capacity must be 1 .. {MAX_OVERLAPS}, not {capacity}")
    return capacity, False


def label_overlap(labels_a, labels_b, u=None, v=None, w=None, n_a=None, n_b=None, capacity=None):
    """The overlap of two label volumes on the device (include/f3d.h, f3d_label_overlap): labels_a an integer [z, y, x] volume on the
    grid of the displacement u, v, w (numpy [z, y, x] float32, or all three None for the identity), labels_b one of the same shape on
    the grid the displacement leads to; 0 background, 1 .. n_a / n_b the bodies, anything else foreign; n_a / n_b None means the
    volume's maximum.  capacity is the room for distinct pairs: None starts at 8 * (n_a + n_b) (at most 2^20) and doubles until the
    table is complete; a given capacity is tried once, and an Overlaps with no rows and info["complete"] == 0 comes back when it does
    not suffice.  Returns an Overlaps."""
    fn = _overlap_entry()
    given = [x is not None for x in (u, v, w)]
    if any(given) and not all(given):
        raise ValueError("u, v and w must be given all three or not at all")
    bits_a, n_a = _labels_as_float_bits(labels_a, n_a)
    bits_b, n_b = _labels_as_float_bits(labels_b, n_b)
    capacity, retry = _overlap_capacity(capacity, n_a, n_b)
    vols = (bits_a, bits_b, u, v, w) if all(given) else (bits_a, bits_b)
    with _on_device(vols, "labels_a, labels_b and u, v, w must be [z, y, x] volumes of one shape") as (box, p, dims):
        box.set_current()
        d = p[2:] if all(given) else [0, 0, 0]
        while True:
            rows, info = (Overlap * capacity)(), OverlapInfo()
            check(fn(p[0], n_a, p[1], n_b, *d, *dims, capacity, rows, C.byref(info)), "f3d_label_overlap")
            if info.complete or not retry or capacity >= MAX_OVERLAPS:
                break
            capacity = min(2 * capacity, MAX_OVERLAPS)
    assert C.sizeof(Overlap) == _OVERLAP_DTYPE.itemsize
    return Overlaps(rows, int(info.n_pairs) if info.complete else 0, info.as_dict())


class Tracks:
    """The tracks of the bodies of two label volumes (solve_overlaps): .a, a structured array over the bodies of A (body a at index
    a - 1: n, n_lost, n_background, n_best, best_b, n_targets, fraction, shift, iou, status), .b, one over the bodies of B (m,
    n_unreached, n_best, best_a, n_sources, status), status being bits of TRACK_STATUS; .map_b (int32: the number every body of B
    takes so that a matched body carries the number of its body of A, new bodies n_a + 1 .., 0 for a body nothing landed in);
    .summary (dict: matched, split, merged, vanished, appeared, left, n_ids); .info, the dict of f3d_overlap_info when the overlaps
    came from the device in the same call, else None; .relabelled, B under the new numbers when the call made it, else None."""

    def __init__(self, a, b, map_b, summary, info=None):
        self.a, self.b, self.map_b, self.summary, self.info = a, b, map_b, summary, info
        self.relabelled = None

    @staticmethod
    def _words(status):
        return [name for name, bit in TRACK_STATUS.items() if status & bit]

    def as_table(self):
        """one dict per body, those of A first: side ("a" / "b"), label, status (a list of the words of TRACK_STATUS), then the fields"""
        rows = []
        for side, table in (("a", self.a), ("b", self.b)):
            for i in range(len(table)):
                row = {"side": side, "label": i + 1, "status": self._words(int(table["status"][i]))}
                row.update({name: table[name][i].tolist() for name in table.dtype.names if name not in ("status", "pad")})
                if side == "b":
                    row["new_label"] = int(self.map_b[i])
                rows.append(row)
        return rows


def solve_overlaps(overlaps, n_a, n_b, min_fraction=0.1):
    """f3d_overlap_solve (include/f3d_host.h; host code, no device): the Tracks of an Overlaps of volumes with n_a and n_b bodies.  A
    partner counts as a target (source) when it holds at least min_fraction, in (0, 1], of the body's voxels."""
    n_a, n_b, min_fraction = int(n_a), int(n_b), float(min_fraction)
    if not (1 <= n_a <= MAX_LABELS and 1 <= n_b <= MAX_LABELS):
        raise ValueError(f"n_a and n_b must be 1 .. {MAX_LABELS}, not {n_a} and {n_b}")
    if not 0.0 < min_fraction <= 1.0:
        raise ValueError(f"min_fraction must be in (0, 1], not {min_fraction}")
    a, b, map_b, summary = (TrackA * n_a)(), (TrackB * n_b)(), np.zeros(n_b, np.int32), TrackSummary()
    _host_check(host().f3d_overlap_solve(overlaps.rows, len(overlaps), n_a, n_b, min_fraction, a, b, map_b.ctypes.data_as(C.POINTER(C.c_int)),
                                         C.byref(summary)), "f3d_overlap_solve")
    assert C.sizeof(TrackA) == _TRACK_A_DTYPE.itemsize and C.sizeof(TrackB) == _TRACK_B_DTYPE.itemsize
    return Tracks(np.frombuffer(a, _TRACK_A_DTYPE, n_a).copy(), np.frombuffer(b, _TRACK_B_DTYPE, n_b).copy(), map_b, summary.as_dict())


def relabel_labels(labels, mapping, count_foreign=False):
    """New numbers for the bodies of a label volume on the device (include/f3d.h, f3d_relabel_labels): an int32 [z, y, x] volume with
    mapping[l - 1] where labels == l in 1 .. len(mapping) and 0 elsewhere.  No entry of mapping may be negative; two labels may share a
    number.  With count_foreign, (volume, the number of voxels outside 0 .. len(mapping))."""
    fn = _relabel_entry()
    mapping = np.ascontiguousarray(mapping)
    if mapping.ndim != 1 or not np.issubdtype(mapping.dtype, np.integer):
        raise ValueError("mapping must be a one-dimensional array of integers, the new number of label l at index l - 1")
    if mapping.size and (int(mapping.min()) < 0 or int(mapping.max()) > 2 ** 31 - 1):
        raise ValueError("the entries of mapping must be 0 .. 2^31 - 1")
    bits, n = _labels_as_float_bits(labels, len(mapping))
    mapping = mapping.astype(np.int32)
    with _on_device((bits,), "labels must be a [z, y, x] volume") as (box, p, dims):
        box.set_current()
        foreign = C.c_ulonglong()
        check(fn(p[0], n, mapping.ctypes.data_as(C.POINTER(C.c_int)), p[0], *dims, C.byref(foreign)), "f3d_relabel_labels")
        out = box.download(p[0], dims).view(np.int32)
    return (out, int(foreign.value)) if count_foreign else out


def track_labels(labels_a, labels_b, u=None, v=None, w=None, min_fraction=0.1, n_a=None, n_b=None):
    """Which body of B is which body of A, from anywhere: label_overlap on the device, solve_overlaps on the host, relabel_labels of B
    on the device.  Returns a Tracks with .info and .relabelled (B under the numbers of A: a matched body carries the number of its body
    of A, every other body a new one)."""
    overlaps = label_overlap(labels_a, labels_b, u, v, w, n_a, n_b)
    if not overlaps.info["complete"]:
        raise F3dError(f"label_overlap: the two label volumes have more than {MAX_OVERLAPS} distinct pairs")
    n_a = int(np.max(labels_a)) if n_a is None else int(n_a)
    n_b = int(np.max(labels_b)) if n_b is None else int(n_b)
    tracks = solve_overlaps(overlaps, n_a, n_b, min_fraction)
    tracks.info = overlaps.info
    tracks.overlaps = overlaps
    tracks.relabelled = relabel_labels(labels_b, tracks.map_b)
    return tracks


class Components:
    """The connected bodies of a thresholded volume (label_components, OpticalFlow.segment): .labels (int32 [d, h, w]: 0 for background
    and for dropped bodies, 1 .. n_labels in ascending order of a body's smallest linear index), .sizes (uint64, the voxels of label L at
    index L - 1), .n_labels and .info, the dict of f3d_component_info."""

    def __init__(self, labels, sizes, info):
        self.labels, self.sizes, self.info = labels, sizes, info
        self.n_labels = int(info["n_labels"])

    def __len__(self):
        return self.n_labels


def _component_range(lo, hi, min_voxels):
    lo, hi, min_voxels = float(np.float32(lo)), float(np.float32(hi)), int(min_voxels)
    if lo != lo or hi != hi or lo > hi:
        raise ValueError(f"lo and hi must be numbers with lo <= hi, not {lo} and {hi}")
    if not 1 <= min_voxels < 2 ** 64:
        raise ValueError(f"min_voxels must be at least 1, not {min_voxels}")
    return lo, hi, min_voxels


def label_components(volume, lo=-np.inf, hi=np.inf, min_voxels=1):
    """The connected bodies of a volume from anywhere on the device (include/f3d.h, f3d_label_components): volume numpy [z, y, x]
    float32; a voxel is foreground when lo <= value <= hi (a NaN never is), bodies are joined over faces, and those of at least
    min_voxels voxels are numbered in ascending order of their smallest linear index.  Returns a Components."""
    fn = _components_entry()
    lo, hi, min_voxels = _component_range(lo, hi, min_voxels)
    volume = np.asarray(volume)
    if volume.ndim != 3 or volume.size == 0:
        raise ValueError("volume must be a non-empty [z, y, x] volume")
    with _on_device((volume,), "volume must be a [z, y, x] volume") as (box, p, dims):
        out = box.alloc()
        box.set_current()
        info = ComponentInfo()
        check(fn(p[0], lo, hi, min_voxels, out, *dims, None, 0, C.byref(info)), "f3d_label_components")
        n = int(info.n_labels)
        sizes = np.zeros(n, np.uint64)
        if n:                                                  # their number is known now: once more with room for all of them
            check(fn(p[0], lo, hi, min_voxels, out, *dims, sizes.ctypes.data_as(C.POINTER(C.c_ulonglong)), n, C.byref(info)),
                  "f3d_label_components")
        labels = box.download(out, dims).view(np.int32)
    return Components(labels, sizes, info.as_dict())


MAX_BINS = 4096
OTSU_OK, OTSU_DEGENERATE = 0, 1
OTSU_TOKENS = {"otsu": (2, 0), "otsu1": (3, 0), "otsu2": (3, 1)}    # what OpticalFlow.segment takes for lo or hi: (classes, which cut)


def _bins(bins):
    if int(bins) != bins or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f"bins must be an integer in 1 .. {MAX_BINS}, not {bins}")
    return int(bins)


def _bin_range(value_range):
    """(lo, hi) as float32 values of a (lo, hi) pair: both finite, lo < hi"""
    try:
        lo, hi = value_range
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
    except (TypeError, ValueError):
        raise ValueError(f"range must be a pair (lo, hi) of numbers, not {value_range!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"range must be finite with lo < hi, not ({lo}, {hi})")
    return lo, hi


class Otsu:
    """The Otsu cuts of a Histogram: .status (OTSU_OK, or OTSU_DEGENERATE when fewer bins are occupied than classes: cuts and values are
    then empty), .cuts (the first bin of every class but the lowest), .values (float32: the edge of each cut, so that class j is
    values[j - 1] <= s < values[j]), .populations (uint64, the voxels of every class) and .objective."""

    def __init__(self, status, cuts, values, populations, objective):
        self.status, self.cuts, self.values, self.populations, self.objective = status, cuts, values, populations, objective


class Histogram:
    """The grey-value histogram of a volume (histogram, OpticalFlow.histogram): .counts (uint64 [bins]), .lo and .hi (the float32 bounds
    the bins are laid over), .info (the dict of f3d_histogram_info; info["used"] == counts.sum()) and .bins.  The bin rule is
    include/f3d.h's; edge, otsu, rank and quantile are the exact host functions of include/f3d_host.h."""

    def __init__(self, counts, lo, hi, info):
        self.counts, self.lo, self.hi, self.info = counts, float(lo), float(hi), info
        self.bins = len(counts)

    def _counts(self):
        counts = np.ascontiguousarray(self.counts, dtype=np.uint64)
        return counts, counts.ctypes.data_as(C.POINTER(C.c_ulonglong))

    def edge(self, k):
        """the smallest float32 value whose bin is at least k: label_components(volume, lo=h.edge(k), hi=h.hi) has counts[k:].sum()
        foreground voxels"""
        edge = C.c_float()
        _host_check(host().f3d_histogram_edge(self.lo, self.hi, self.bins, int(k), C.byref(edge)), "f3d_histogram_edge")
        return np.float32(edge.value)

    def otsu(self, classes=2):
        if classes not in (2, 3):
            raise ValueError(f"classes must be 2 or 3, not {classes}")
        counts, ptr = self._counts()
        cuts, info = (C.c_uint * 2)(), OtsuInfo()
        _host_check(host().f3d_otsu(ptr, self.bins, classes, cuts, C.byref(info)), "f3d_otsu")
        if info.status != OTSU_OK:
            return Otsu(info.status, np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(classes, np.uint64), 0.0)
        found = np.array(cuts[:classes - 1], np.uint32)
        return Otsu(info.status, found, np.array([self.edge(k) for k in found], np.float32),
                    np.array(info.populations[:classes], np.uint64), info.objective)

    def rank(self, r):
        """the bin that holds the r-th smallest counted voxel (0-based)"""
        if int(r) != r or not 0 <= int(r) < 2 ** 64:
            raise ValueError(f"r must be a non-negative integer, not {r}")
        counts, ptr = self._counts()
        found = C.c_uint()
        _host_check(host().f3d_histogram_rank(ptr, self.bins, int(r), C.byref(found)), "f3d_histogram_rank")
        return found.value

    def quantile(self, q):
        """the bin of rank floor(q * (used - 1)), q in [0, 1]"""
        used = int(np.asarray(self.counts, np.uint64).sum())
        if not 0 <= q <= 1:
            raise ValueError(f"q must lie in [0, 1], not {q}")
        if used == 0:
            raise ValueError("the histogram is empty: it has no quantile")
        return self.rank(int(np.floor(q * (used - 1))))


@contextlib.contextmanager
def _volume_and_mask(volume, mask):
    """volume (and mask, an integer or bool [z, y, x] volume of its shape, or None) in containers of their own: yields
    (source pointer, mask pointer or 0, (w, h, d)) with the container geometry set"""
    volume = np.asarray(volume)
    if volume.ndim != 3 or volume.size == 0:
        raise ValueError("volume must be a non-empty [z, y, x] volume")
    vols = [volume]
    if mask is not None:
        bits = _int32_bits(mask, "mask")
        if bits.shape != volume.shape:
            raise ValueError(f"mask must have the shape of the volume, {volume.shape}")
        vols.append(bits)
    with _on_device(vols, "volume must be a [z, y, x] volume") as (box, p, dims):
        box.set_current()
        yield p[0], (p[1] if mask is not None else 0), dims


def value_range(volume, mask=None):
    """The smallest and the largest finite value of a volume on the device (include/f3d.h, f3d_value_range): volume numpy [z, y, x]
    float32, mask an integer volume whose zeros leave voxels out.  Returns (min, max, info): float32 values (+inf and -inf when nothing
    is finite; -0.0 is below +0.0) and the dict of f3d_range_info."""
    fn = _value_range_entry()
    with _volume_and_mask(volume, mask) as (src, msk, dims):
        lo, hi, info = C.c_float(), C.c_float(), RangeInfo()
        check(fn(src, msk, *dims, C.byref(lo), C.byref(hi), C.byref(info)), "f3d_value_range")
    return np.float32(lo.value), np.float32(hi.value), info.as_dict()


def histogram(volume, bins=256, range=None, mask=None):
    """The grey-value histogram of a volume on the device (include/f3d.h, f3d_histogram): bins 1 .. 4096 laid over range = (lo, hi), or
    over the volume's finite minimum and maximum under the mask when range is None (ValueError when there is no finite voxel or only
    one value).  mask: an integer volume whose zeros leave voxels out.  Returns a Histogram."""
    fn, bins = _histogram_entry(), _bins(bins)
    bounds = None if range is None else _bin_range(range)
    find = _value_range_entry() if bounds is None else None
    with _volume_and_mask(volume, mask) as (src, msk, dims):
        if bounds is None:
            lo, hi, found = C.c_float(), C.c_float(), RangeInfo()
            check(find(src, msk, *dims, C.byref(lo), C.byref(hi), C.byref(found)), "f3d_value_range")
            if found.finite == 0:
                raise ValueError("the volume has no finite voxel: there is no range to lay the bins over")
            if not lo.value < hi.value:
                raise ValueError(f"the volume is constant ({lo.value}): there is no range to lay the bins over")
            bounds = (lo.value, hi.value)
        counts, info = np.zeros(bins, np.uint64), HistogramInfo()
        check(fn(src, msk, bounds[0], bounds[1], bins, *dims, counts.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(info)),
              "f3d_histogram")
    return Histogram(counts, bounds[0], bounds[1], info.as_dict())


# the modes, the flag and the outputs of f3d_nearest_seed in ABI order
SEED_MODES = {"nonzero": 0, "zero": 1}
NEAREST_D2_FLOAT = 1
NEAREST_OUTPUTS = ("d2", "index", "value")


def _int32_bits(labels, what):
    """the bits of an integer (or bool) [z, y, x] volume as float32 for the upload; values that do not fit int32 raise"""
    labels = np.asarray(labels)
    if labels.ndim != 3 or labels.size == 0 or not (np.issubdtype(labels.dtype, np.integer) or labels.dtype == np.bool_):
        raise ValueError(f"{what} must be a non-empty [z, y, x] volume of integers")
    if labels.dtype != np.bool_ and (int(labels.min()) < -2 ** 31 or int(labels.max()) > 2 ** 31 - 1):
        raise ValueError(f"{what} does not fit int32")
    return np.ascontiguousarray(labels.astype(np.int32)).view(np.float32)


def nearest_seed(labels, mode="nonzero", outputs=NEAREST_OUTPUTS, d2_float=False):
    """The exact squared Euclidean distance and nearest-seed transform on the device (include/f3d.h, f3d_nearest_seed): labels an integer
    [z, y, x] volume whose seeds are the voxels != 0 (mode "nonzero") or == 0 (mode "zero").  Returns (fields, info): fields a dict with
    the asked-for ones of "d2" (squared distance to the nearest seed; float32 with d2_float), "index" (its x + W (y + H z), -1 without a
    seed) and "value" (labels there), int32 [z, y, x] each; of several seeds at one distance the one with the smallest index wins.
    info: the dict of f3d_nearest_info."""
    fn = _nearest_entry()
    if mode not in SEED_MODES:
        raise ValueError(f"mode must be one of {sorted(SEED_MODES)}, not {mode!r}")
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or any(o not in NEAREST_OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError(f"outputs must be some of {NEAREST_OUTPUTS}, each once, not {outputs!r}")
    bits = _int32_bits(labels, "labels")
    with _on_device((bits,), "labels must be a [z, y, x] volume") as (box, p, dims):
        out = [box.alloc() if name in outputs else 0 for name in NEAREST_OUTPUTS]
        box.set_current()
        info = NearestInfo()
        check(fn(p[0], SEED_MODES[mode], NEAREST_D2_FLOAT if d2_float else 0, *out, *dims, C.byref(info)), "f3d_nearest_seed")
        fields = {name: box.download(o, dims) for name, o in zip(NEAREST_OUTPUTS, out) if o}
    return {name: a if name == "d2" and d2_float else a.view(np.int32) for name, a in fields.items()}, info.as_dict()


def distance_transform(mask):
    """The squared Euclidean distance of every voxel of mask (any [z, y, x] volume; a voxel counts where it is != 0) to the nearest voxel
    where mask == 0, exactly, as int32 [z, y, x]: 0 outside the mask, 2^31 - 1 everywhere when the mask has no zero (nearest_seed in
    mode "zero")."""
    mask = np.asarray(mask)
    if mask.ndim != 3 or mask.size == 0:
        raise ValueError("mask must be a non-empty [z, y, x] volume")
    return nearest_seed(mask != 0, mode="zero", outputs=("d2",))[0]["d2"]


def _core_d2(radius, core_d2):
    """the core_d2 of f3d_split_components from exactly one of a radius in voxels (ceil(radius^2)) and the exact integer"""
    if (radius is None) == (core_d2 is None):
        raise ValueError("give exactly one of radius and core_d2")
    if radius is not None:
        radius = float(radius)
        if not (np.isfinite(radius) and radius > 0):
            raise ValueError(f"radius must be finite and positive, not {radius}")
        core_d2 = int(np.ceil(radius * radius))
    if int(core_d2) != core_d2 or not 1 <= int(core_d2) < 2 ** 64:
        raise ValueError(f"core_d2 must be an integer of at least 1, not {core_d2}")
    return int(core_d2)


def split_components(volume, lo=-np.inf, hi=np.inf, radius=None, core_d2=None, min_voxels=1):
    """The bodies of a volume from anywhere with touching bodies taken apart, on the device (include/f3d.h, f3d_split_components): the
    foreground (lo <= value <= hi) is eroded to the voxels whose squared distance to the background is at least core_d2 (or
    ceil(radius^2); exactly one of the two is given), those cores are joined over faces, and every foreground voxel goes to the nearest
    core voxel's body when that lies in its own connected component, else to the remainder of its component.  core_d2 = 1 is
    label_components.  Returns a Components whose info is the dict of f3d_split_info."""
    fn = _split_entry()
    lo, hi, min_voxels = _component_range(lo, hi, min_voxels)
    core_d2 = _core_d2(radius, core_d2)
    volume = np.asarray(volume)
    if volume.ndim != 3 or volume.size == 0:
        raise ValueError("volume must be a non-empty [z, y, x] volume")
    with _on_device((volume,), "volume must be a [z, y, x] volume") as (box, p, dims):
        out = box.alloc()
        box.set_current()
        info = SplitInfo()
        check(fn(p[0], lo, hi, core_d2, min_voxels, out, *dims, None, 0, C.byref(info)), "f3d_split_components")
        n = int(info.n_labels)
        sizes = np.zeros(n, np.uint64)
        if n:                                                  # their number is known now: once more with room for all of them
            check(fn(p[0], lo, hi, core_d2, min_voxels, out, *dims, sizes.ctypes.data_as(C.POINTER(C.c_ulonglong)), n, C.byref(info)),
                  "f3d_split_components")
        labels = box.download(out, dims).view(np.int32)
    return Components(labels, sizes, info.as_dict())


def validate_displacement(u, v, w, weight=None, weight_min=0.8, step=1, eps=0.1, threshold=2.0, min_neighbours=9, mode="replace",
                          fill_passes=0, fields=("r", "d")):
    """The normalised median test of a displacement on the device (include/f3d.h, f3d_validate_displacement): u, v, w numpy [z, y, x]
    float32; every vector is compared with the median of its up to 26 neighbours `step` voxels away, in units of the median residual
    of those neighbours plus eps.  A voxel is absent where u, v or w is NaN or, with `weight` (same shape, e.g. the zncc of a match),
    where weight < weight_min or NaN.  Vectors with r > threshold (tested with at least min_neighbours neighbours) and absent voxels
    are rejected: NaN under mode "mark", the neighbour median under "replace" (NaN with fewer than min_neighbours neighbours).
    fill_passes (needs "d"): up to that many further passes over the result with threshold inf and no weight, each of which gives
    undefined voxels with enough defined neighbours their median; they stop when nothing is undefined or the count stops falling.
    fields: "r" (the normalised residual, NaN where untested), "d" (the validated u, v, w).  Returns a dict name -> array for the
    selected outputs and "stats" -> dict (present, tested, outliers, replaced, undefined, r_max) of the first pass with replaced and
    undefined brought to the final state."""
    fn = _validate_entry()
    mask, m = _mask(fields, VALIDATE_GROUPS, "validation"), _validate_mode(mode)
    if fill_passes and not mask & VALIDATE_GROUPS["d"]:
        raise ValueError("fill_passes needs the validated displacement (\"d\" in fields)")
    vols = (u, v, w) if weight is None else (u, v, w, weight)
    with _on_device(vols, "u, v, w and weight must be [z, y, x] volumes of one shape") as (box, p, dims):
        outs = [box.alloc() if mask & g else 0 for g in _VALIDATE_GROUP_OF]
        box.set_current()
        stats = ValidateStats()
        check(fn(p[0], p[1], p[2], p[3] if weight is not None else 0, weight_min, step, eps, threshold, min_neighbours, m,
                 (_dp * 4)(*outs), mask, *dims, C.byref(stats)), "f3d_validate_displacement")
        spare = [0] + [box.alloc() for _ in range(3)] if fill_passes and stats.undefined else None
        for _ in range(fill_passes):
            if not stats.undefined:
                break
            filled = ValidateStats()
            check(fn(outs[1], outs[2], outs[3], 0, 0.0, step, eps, float("inf"), min_neighbours, VALIDATE_MODES["replace"],
                     (_dp * 4)(*spare), VALIDATE_GROUPS["d"], *dims, C.byref(filled)), "f3d_validate_displacement")
            outs[1:], spare[1:] = spare[1:], outs[1:]
            fell = filled.undefined < stats.undefined
            stats.replaced += filled.replaced
            stats.undefined = filled.undefined
            if not fell:
                break
        res = {n: box.download(o, dims) for n, o in zip(VALIDATE_NAMES, outs) if o}
    res["stats"] = stats.as_dict()
    return res


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_fp)


def make_params(**kw):
    d = dict(DEFAULT_PARAMS)
    unknown = set(kw) - set(d)
    if unknown:
        raise TypeError(f"unknown flow parameters: {sorted(unknown)}")
    d.update(kw)
    return FlowParams(**d)


# ---- host-only helpers --------------------------------------------------------------------------------------

def max_warp_level(width, height, depth, scale_factor):
    return int(host().f3d_max_warp_level(width, height, depth, scale_factor))


def level_geometry(width, height, depth, scale_factor, level):
    size = Size4()
    hx, hy, hz = C.c_float(), C.c_float(), C.c_float()
    check(host().f3d_level_geometry(width, height, depth, scale_factor, level, C.byref(size), hx, hy, hz))
    return (size.width, size.height, size.depth), (hx.value, hy.value, hz.value)


def gaussian_taps(sigma):
    taps = np.zeros(51, np.float32)
    radius = _sz()
    if host().f3d_gaussian_taps(sigma, taps.ctypes.data_as(_fp), 51, C.byref(radius)) != 0:
        raise F3dError("sigma too large for the 51-tap limit")
    return int(radius.value), taps[: 2 * radius.value + 1].copy()


def read_raw(path, dims, u8=True):
    w, h, d = dims
    out = np.empty((d, h, w), np.float32)
    fn = host().f3d_raw_read_u8 if u8 else host().f3d_raw_read_f32
    if fn(os.fsencode(path), w, h, d, out.ctypes.data_as(_fp)) != 0:
        raise F3dError(f"cannot read {path} as {w}x{h}x{d}")
    return out


def write_raw(path, vol, u8=False):
    vol, p = _f32(vol)
    d, h, w = vol.shape
    fn = host().f3d_raw_write_u8 if u8 else host().f3d_raw_write_f32
    if fn(os.fsencode(path), p, w, h, d) != 0:
        raise F3dError(f"cannot write {path}")


def write_vtk(path, u, v, w_):
    u, pu = _f32(u)
    v, pv = _f32(v)
    w_, pw = _f32(w_)
    d, h, w = u.shape
    if host().f3d_vtk_write_flow(os.fsencode(path), pu, pv, pw, w, h, d) != 0:
        raise F3dError(f"cannot write {path}")


def synth_pair(width, height, depth):
    f0 = np.empty((depth, height, width), np.float32)
    f1 = np.empty_like(f0)
    check(host().f3d_synth_pair(width, height, depth, f0.ctypes.data_as(_fp), f1.ctypes.data_as(_fp)))
    return f0, f1


def synth_planes(width, height, depth, z_lo, z_hi, frame_0, frame_1):
    """Render planes [z_lo, z_hi) of the synthetic pair, unscaled, into full-size arrays; returns max(frame_0 planes)."""
    m = C.c_float()
    check(host().f3d_synth_planes(width, height, depth, z_lo, z_hi, frame_0.ctypes.data_as(_fp), frame_1.ctypes.data_as(_fp),
                                  C.byref(m)), "f3d_synth_planes")
    return m.value


def flow_plane_digests(flow, z_lo=0, z_hi=None):
    """sha256 of every plane z_lo <= z < z_hi of each of (u, v, w) (float32, -0 normalised to +0): three lists of 32-byte
    digests.  Planes hash independently, so the ranks of a z-slab run can each hash what they own."""
    import hashlib
    out = []
    for vol in flow:
        hi = vol.shape[0] if z_hi is None else z_hi
        out.append([hashlib.sha256(np.ascontiguousarray(vol[z] + np.float32(0.0)).tobytes()).digest() for z in range(z_lo, hi)])
    return out


def combine_plane_digests(per_component):
    """One hex digest from the per-plane digests of (u, v, w), all planes of u first, in plane order."""
    import hashlib
    h = hashlib.sha256()
    for comp in per_component:
        for d in comp:
            h.update(d)
    return h.hexdigest()


# ---- device memory ---------------------------------------------------------------------------------------------

class Containers:
    """A set of equally sized pitched device containers (what OpticalFlowE::InitCudaMemory allocates)."""

    def __init__(self, width, height, depth, device=-1):
        check(hip().f3d_init(device), "f3d_init")
        self.width, self.height, self.depth = width, height, depth
        self.pitch = 0
        self._ptrs = []

    @property
    def size4(self):
        return Size4(self.width, self.height, self.depth, self.pitch)

    def set_current(self):
        s = self.size4
        check(hip().f3d_set_container(C.byref(s)), "f3d_set_container")

    def alloc(self, fill=None):
        ptr, pitch = _dp(), _sz()
        check(hip().f3d_alloc_pitched(C.byref(ptr), C.byref(pitch), self.width * 4, self.height * self.depth),
              "f3d_alloc_pitched")
        if self.pitch and pitch.value != self.pitch:
            raise F3dError("containers came back with different pitches")
        self.pitch = pitch.value
        self._ptrs.append(ptr.value)
        if fill is not None:
            # byte pattern over the whole pitched allocation (0xFF.. = NaN poison)
            check(hip().f3d_memset2d(ptr.value, self.pitch, fill, self.pitch, self.height * self.depth))
        return ptr.value

    def upload(self, ptr, vol, plane0=0):
        vol, p = _f32(vol)
        d, h, w = vol.shape
        check(hip().f3d_copy3d_h2d(ptr, self.pitch, self.height, plane0, p, w, h, d), "f3d_copy3d_h2d")

    def download(self, ptr, dims, plane0=0):
        w, h, d = dims
        out = np.empty((d, h, w), np.float32)
        check(hip().f3d_copy3d_d2h(out.ctypes.data_as(_fp), w, h, d, ptr, self.pitch, self.height, plane0),
              "f3d_copy3d_d2h")
        return out

    def new(self, vol=None, fill=0xFF):
        """Allocate a NaN-poisoned container and optionally upload a [d, h, w] sub-box into its corner."""
        p = self.alloc(fill=fill)
        if vol is not None:
            self.upload(p, vol)
        return p

    def free(self):
        for p in self._ptrs:
            hip().f3d_free(p)
        self._ptrs = []


def sync():
    check(hip().f3d_stream_sync(), "f3d_stream_sync")


class Lane:
    """A stream and a container geometry of one's own (include/f3d.h, f3d_lane_*): a driver created and used between
    make_current() and release() in ONE thread runs beside the drivers of other threads instead of in line with them.
        with f3d.Lane():            # in a worker thread
            flow = f3d.OpticalFlow(); flow.initialize(w, h, d); u, v, w = flow.compute(f0, f1); flow.destroy()"""

    def __init__(self):
        check(hip().f3d_init(-1), "f3d_init")
        self._h = C.c_void_p()
        check(hip().f3d_lane_create(C.byref(self._h)), "f3d_lane_create")

    def make_current(self):
        check(hip().f3d_lane_make_current(self._h), "f3d_lane_make_current")

    def release(self):
        hip().f3d_lane_make_current(None)

    def destroy(self):
        if self._h:
            hip().f3d_lane_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        self.make_current()
        return self

    def __exit__(self, *exc):
        self.release()
        self.destroy()
        return False


def mem_info():
    """(free, total) bytes of device memory."""
    check(hip().f3d_init(-1), "f3d_init")
    free, total = _sz(), _sz()
    check(hip().f3d_mem_info(C.byref(free), C.byref(total)), "f3d_mem_info")
    return free.value, total.value


# ---- operator layer (CudaOperation* through the string-keyed bag) -------------------------------------------------

_PTR_KEYS = {
    "dev_frame_0", "dev_frame_1", "dev_flow_u", "dev_flow_v", "dev_flow_w", "dev_phi", "dev_ksi", "dev_flow_du",
    "dev_flow_dv", "dev_flow_dw", "dev_temp_du", "dev_temp_dv", "dev_temp_dw", "dev_input", "dev_output", "dev_temp",
    "operand_0", "operand_1",
}
_SIZE_T_KEYS = {"outer_iterations_count", "inner_iterations_count", "radius", "warp_levels_count", "median_radius"}
_FLOAT_KEYS = {"equation_alpha", "equation_smoothness", "equation_data", "hx", "hy", "hz", "gaussian_sigma",
               "warp_scale_factor"}
_SIZE4_KEYS = {"data_size", "resample_size", "container_size"}


class Stat3(C.Structure):
    """src/data_types/data_structs.h:29-33"""
    _fields_ = [("min", C.c_float), ("max", C.c_float), ("avg", C.c_float)]


class HostVolume:
    """Dense host volume [z, y, x] float32 handed to the piecemeal operators as a Data3D* (f3d_volume_wrap).  Like the
    reference's Data3D::Swap, registration_p / solve_p exchange STORAGE between the volumes of one call, so a volume may
    end up holding the array another one was created with.  The class therefore keeps every wrapped array alive in a
    table keyed by its address, together with whether it is page-locked, and a volume that goes away releases the storage
    it holds AT THAT MOMENT (f3d_volume_data), never the one it started with: the survivor of a swapped pair keeps its
    memory, its page-lock and its .array.  A finalizer does the same for volumes that are dropped without destroy()."""
    _storage = {}   # address -> [array, page-locked]

    def __init__(self, array, pin=False):
        a = np.ascontiguousarray(array, dtype=np.float32)
        if a.ndim != 3:
            raise ValueError("volume must be [z, y, x]")
        if pin and a.nbytes < (32 << 20):
            # A small array lives in the allocator's shared heap: page-locked there it shares pages with its neighbours and sits under
            # a heap top that moves (a GPU memory access fault once in ~4 000 small runs, LABBOOK round 4).  The volume gets a mapping of
            # its own instead and the values are copied in; `.array` is that storage.
            import mmap
            own = np.frombuffer(mmap.mmap(-1, max(a.nbytes, mmap.PAGESIZE)), dtype=np.float32, count=a.size).reshape(a.shape)
            own[...] = a
            a = own
        if a.ctypes.data in HostVolume._storage:
            raise ValueError("this array is already wrapped by another HostVolume")
        self._h = C.c_void_p()
        d, h, w = a.shape
        check(host().f3d_volume_wrap(C.byref(self._h), a.ctypes.data_as(_fp), w, h, d), "f3d_volume_wrap")
        entry = [a, False]
        HostVolume._storage[a.ctypes.data] = entry
        if pin:  # page-locked: full link rate, and a precondition of the solver's overlapped schedule
            try:
                check(hip().f3d_init(-1), "f3d_init")
                check(hip().f3d_host_register(C.c_void_p(a.ctypes.data), a.nbytes), "f3d_host_register")
            except Exception:
                self.destroy()
                raise
            entry[1] = True
        self._finalizer = weakref.finalize(self, HostVolume._release, self._h.value)

    @staticmethod
    def _release(handle):
        """drop the Data3D and whatever storage it holds now"""
        if not handle or _host is None:
            return
        cur = _host.f3d_volume_data(C.c_void_p(handle))
        _host.f3d_volume_destroy(C.c_void_p(handle))
        entry = HostVolume._storage.pop(cur, None)
        if entry is not None and entry[1] and _hip is not None and _hip.f3d_is_initialized():
            _hip.f3d_host_unregister(C.c_void_p(cur))

    @classmethod
    def release_all(cls):
        """exit hook: remove every page-lock that is still in place (the arrays themselves are numpy's to free)"""
        for addr, entry in list(cls._storage.items()):
            if entry[1] and _hip is not None and _hip.f3d_is_initialized():
                _hip.f3d_host_unregister(C.c_void_p(addr))
            entry[1] = False

    @property
    def object(self):
        return host().f3d_volume_object(self._h)

    @property
    def array(self):
        return HostVolume._storage[host().f3d_volume_data(self._h)][0]

    def destroy(self):
        if self._h:
            fin = getattr(self, "_finalizer", None)
            if fin is not None:
                fin.detach()
            HostVolume._release(self._h.value)
            self._h = C.c_void_p()


def plan_solve_piecemeal(budget_bytes, width, height, depth, inner_iterations, outer_iterations, forced_outer_per_pass=0,
                         overlap_mode=0):
    """(chunk, outer_per_pass, halo, max_planes, overlapped) the piecemeal solver would use for a level (host arithmetic);
    overlap_mode 0 = serial schedule, 1 = copies beside the kernels, -1 = the cost model's choice."""
    out = [C.c_int() for _ in range(5)]
    check(host().f3d_plan_solve_piecemeal(budget_bytes, width, height, depth, inner_iterations, outer_iterations,
                                          forced_outer_per_pass, overlap_mode, *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def plan_sweeps(inner, fused, tri, carry):
    """[(sweeps, next_weights), ...]: the launches the solver drivers cut the `inner` sweeps of one outer iteration into (host
    arithmetic).  fused / tri: the solve takes the fused / the three-stage launches; carry: another outer iteration follows and
    the driver can take its weights along."""
    cap = max(1, inner)
    sweeps, weights = (C.c_int * cap)(), (C.c_int * cap)()
    n = host().f3d_plan_sweeps(inner, int(bool(fused)), int(bool(tri)), int(bool(carry)), sweeps, weights, cap)
    if n < 0:
        raise F3dError("f3d_plan_sweeps failed")
    return [(sweeps[i], bool(weights[i])) for i in range(n)]


def plan_sweeps_weights_first(inner):
    """[(first, sweeps, weights_first, next_weights), ...]: the weights-first cut of the `inner` sweeps of one outer iteration (host
    arithmetic; first = index of the launch's first sweep): launch 0 computes the iteration's phi / ksi in front of its first sweep, pairs follow, a single sweep ends an even
    count."""
    cap = max(1, inner)
    start, sweeps, first, nxt = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
    n = host().f3d_plan_sweeps_weights_first(inner, start, sweeps, first, nxt, cap)
    if n < 0:
        raise F3dError("f3d_plan_sweeps_weights_first failed")
    return [(start[i], sweeps[i], bool(first[i]), bool(nxt[i])) for i in range(n)]


Pair8Plan = collections.namedtuple("Pair8Plan", "A a b zc_a zc_b wgs cost tiles")


def pair8_plan(width, rows, planes, ty, zc_limit=None, per_round=0, fold=False):
    """How a fused solver launch of a width x rows x planes window with `ty` rows per tile is cut into workgroups (host arithmetic):
    the first A tiles in `a` chunks of zc_a planes, the other tiles in `b` chunks of zc_b planes; A = 0 is the uniform plan.
    per_round 0 = 256 (or F3D_PAIR8_ROUND); F3D_PAIR8_PLAN=0 gives the uniform plan."""
    out = (C.c_longlong * 8)()
    check(host().f3d_pair8_plan(width, rows, planes, ty, planes if zc_limit is None else zc_limit, per_round, int(bool(fold)), out))
    return Pair8Plan(*[int(v) for v in out])


def solver_chunk_limit(plane_bytes, reach):
    """The planes a z-chunk of a solver launch may hold at most in a container whose planes are `plane_bytes` (container height x
    pitch in bytes), for a launch that reads `reach` halo planes on either side of a chunk (1: phi/ksi or one sweep, 2: the
    two-stage launches, 3: the three-stage ones); 0 where not even one plane fits the 32-bit offsets and the launch is refused."""
    return int(host().f3d_solver_chunk_limit(int(plane_bytes), int(reach)))


def pair8_decode(width, rows, ty, fold, plan, xcd_remap, z_lo, z_hi):
    """The kernel's decode of every workgroup number of a launch under `plan` (a Pair8Plan), run on the host: an int array
    [grid, 6] of tile, tile column, tile row, folded, z0, z1 -- rows of -1 for the padding numbers of an XCD's run."""
    cut = (C.c_longlong * 8)(*plan)
    grid = C.c_int()
    args = (width, rows, ty, int(bool(fold)), cut, int(bool(xcd_remap)), z_lo, z_hi)
    check(host().f3d_pair8_decode(*args, 0, 0, None, C.byref(grid)))
    out = np.empty((grid.value, 6), np.int32)
    check(host().f3d_pair8_decode(*args, 0, grid.value, out.ctypes.data_as(C.POINTER(C.c_int)), None))
    return out


Pair8WidePlan = collections.namedtuple("Pair8WidePlan", "classes cost wgs tiles")


def pair8_plan_wide(width, rows, planes, ty, zc_limit=None, per_round=0, fold=False):
    """The plan the fused z-marching launches take (the launcher's own function, host arithmetic): `classes` is a tuple of up to three
    (tiles, chunks, planes per chunk) in tile order, every class but the last filling whole rounds.  F3D_PAIR8_PLAN (read per
    call) unset or 2 = the wide plan where it is strictly cheaper than pair8_plan's, 1 = pair8_plan's, 0 = the uniform plan."""
    out = (C.c_longlong * 12)()
    check(host().f3d_pair8_plan_wide(width, rows, planes, ty, planes if zc_limit is None else zc_limit, per_round, int(bool(fold)), out))
    v = [int(x) for x in out]
    return Pair8WidePlan(tuple(tuple(v[i:i + 3]) for i in (0, 3, 6) if v[i]), v[10], v[9], v[11])


def pair8_decode_wide(width, rows, ty, fold, plan, xcd_remap, z_lo, z_hi):
    """pair8_decode under a Pair8WidePlan"""
    classes = [c for c in plan.classes] + [(0, 0, 0)] * (3 - len(plan.classes))
    cut = (C.c_longlong * 9)(*[x for c in classes for x in c])
    grid = C.c_int()
    args = (width, rows, ty, int(bool(fold)), cut, int(bool(xcd_remap)), z_lo, z_hi)
    check(host().f3d_pair8_decode_wide(*args, 0, 0, None, C.byref(grid)))
    out = np.empty((grid.value, 6), np.int32)
    check(host().f3d_pair8_decode_wide(*args, 0, grid.value, out.ctypes.data_as(C.POINTER(C.c_int)), None))
    return out


class Operation:
    """One of the operators (add, convolution, median, registration, resample, solve, stat), driven exactly like the reference drives them: Initialize({"container_size"}),
    Execute(bag of pointers to caller variables).  After execute() the (possibly swapped) pointer values are
    available in .values (the solver swaps dev_flow_d* / dev_temp_d* through the bag)."""

    def __init__(self, name):
        self._h = C.c_void_p()
        if host().f3d_op_create(C.byref(self._h), name.encode()) != 0:
            raise F3dError(f"unknown operation {name!r}")
        self.values = {}

    @property
    def name(self):
        return host().f3d_op_name(self._h).decode()

    def initialize(self, containers=None):
        if containers is None:
            return host().f3d_op_initialize(self._h, None) == 0
        s = containers.size4
        return host().f3d_op_initialize(self._h, C.byref(s)) == 0

    def set_slab(self, slab):
        self._slab = slab
        host().f3d_op_set_slab(self._h, C.byref(slab) if slab is not None else None)

    def execute(self, **params):
        store = {}
        volumes = {}
        for k, v in params.items():
            if isinstance(v, HostVolume):
                volumes[k] = v          # Data3D* keys of the piecemeal operators: the bag holds the object itself
            elif k in _PTR_KEYS:
                store[k] = _dp(v)
            elif k in _SIZE_T_KEYS:
                store[k] = _sz(v)
            elif k in _FLOAT_KEYS:
                store[k] = C.c_float(v)
            elif k in _SIZE4_KEYS:
                store[k] = Size4(v[0], v[1], v[2], 0) if not isinstance(v, Size4) else v
            elif k == "max_mag":
                store[k] = _sz(v)
            elif k == "stat":
                store[k] = v            # a Stat3 the operator fills in
            elif k == "flow_update":
                store[k] = C.c_bool(bool(v))   # solve: asks for flow += increments inside the solve; comes back True where it was done
            else:
                raise TypeError(f"unknown parameter key {k!r}")
        n = len(store) + len(volumes)
        keys = (C.c_char_p * n)(*[k.encode() for k in list(store) + list(volumes)])
        ptrs = (C.c_void_p * n)(*([C.cast(C.byref(v), C.c_void_p) for v in store.values()] +
                                  [C.c_void_p(v.object) for v in volumes.values()]))
        check(host().f3d_op_execute(self._h, keys, ptrs, n), "f3d_op_execute")
        self.values = {k: (v.value if hasattr(v, "value") else v) for k, v in store.items()}
        return self.values

    def execute_batch(self, bags):
        """ExecuteBatch of the add / median / resample operators: a list of parameter dicts, one per volume."""
        stores = []
        for params in bags:
            store = {}
            for k, v in params.items():
                if k in _PTR_KEYS:
                    store[k] = _dp(v)
                elif k in _SIZE_T_KEYS:
                    store[k] = _sz(v)
                elif k in _SIZE4_KEYS:
                    store[k] = Size4(v[0], v[1], v[2], 0) if not isinstance(v, Size4) else v
                else:
                    raise TypeError(f"unknown parameter key {k!r}")
            stores.append(store)
        n = sum(len(s) for s in stores)
        keys = (C.c_char_p * n)(*[k.encode() for s in stores for k in s])
        ptrs = (C.c_void_p * n)(*[C.cast(C.byref(v), C.c_void_p) for s in stores for v in s.values()])
        counts = (C.c_size_t * len(stores))(*[len(s) for s in stores])
        check(host().f3d_op_execute_batch(self._h, keys, ptrs, counts, len(stores)), "f3d_op_execute_batch")

    def solve_p_fused_weights(self):
        """whether the last solve_p execute fused the last sweep of an outer iteration with the next weights"""
        f = C.c_int()
        check(host().f3d_op_solve_p_fused_weights(self._h, C.byref(f)), "f3d_op_solve_p_fused_weights")
        return bool(f.value)

    def solve_p_last(self):
        """(chunk, outer_per_pass, halo, passes, overlapped) of the last solve_p execute"""
        c, n, h, p, o = C.c_int(), C.c_int(), C.c_int(), _sz(), C.c_int()
        check(host().f3d_op_solve_p_last(self._h, C.byref(c), C.byref(n), C.byref(h), C.byref(p), C.byref(o)), "f3d_op_solve_p_last")
        return c.value, n.value, h.value, p.value, bool(o.value)

    def destroy(self):
        if self._h:
            host().f3d_op_destroy(self._h)
            self._h = C.c_void_p()


# ---- driver (OpticalFlowE) ----------------------------------------------------------------------------------------

class OpticalFlow:
    """OpticalFlowE: Initialize(DataSize4) / ComputeFlow(frame_0, frame_1 -> u, v, w) / Destroy()."""

    def __init__(self):
        self._h = C.c_void_p()
        check(host().f3d_flow_create(C.byref(self._h)), "f3d_flow_create")
        self.dims = None

    def initialize(self, width, height, depth):
        if host().f3d_flow_initialize(self._h, width, height, depth) != 0:
            raise F3dError("OpticalFlowE::Initialize failed: " + (hip().f3d_last_error() or b"").decode())
        self.dims = (width, height, depth)
        return True

    def compute(self, frame_0, frame_1, silent=True, out=None, initial=None, **kw):
        """OpticalFlowE::ComputeFlow: upload, solve, download.  `out` = three preallocated C-contiguous float32 [z,y,x] arrays
        to receive u, v, w (the reference's caller owns its flow volumes too, page-locked or not); fresh ones otherwise.
        `initial` (see set_initial): the displacement the pyramid starts from instead of zero; None is the call as it always was."""
        f0, p0 = _f32(frame_0)
        f1, p1 = _f32(frame_1)
        w, h, d = self.dims
        if f0.shape != (d, h, w) or f1.shape != (d, h, w):
            raise ValueError(f"frames must be [z,y,x] = {(d, h, w)}")
        if out is None:
            u, v, ww = (np.empty((d, h, w), np.float32) for _ in range(3))
        else:
            u, v, ww = out
            for a in (u, v, ww):
                if a.dtype != np.float32 or a.shape != (d, h, w) or not a.flags["C_CONTIGUOUS"]:
                    raise ValueError(f"out arrays must be C-contiguous float32 [z,y,x] = {(d, h, w)}")
        prm = make_params(**kw)
        if initial is not None:
            if isinstance(initial, str) and initial in ("block-match", "held"):
                raise ValueError(f"initial={initial!r} reads the pair that is resident, and compute() uploads its own afterwards: "
                                 "upload() the pair and use compute_resident(initial=...)")
            self.set_initial(initial)
            _host_check(host().f3d_flow_compute_from_initial(self._h, p0, p1, C.byref(prm), int(silent), u.ctypes.data_as(_fp),
                                                             v.ctypes.data_as(_fp), ww.ctypes.data_as(_fp)),
                        "f3d_flow_compute_from_initial")
            return u, v, ww
        check(host().f3d_flow_compute(self._h, p0, p1, C.byref(prm), int(silent), u.ctypes.data_as(_fp),
                                      v.ctypes.data_as(_fp), ww.ctypes.data_as(_fp)), "f3d_flow_compute")
        return u, v, ww

    def upload(self, frame_0, frame_1):
        f0, p0 = _f32(frame_0)
        f1, p1 = _f32(frame_1)
        check(host().f3d_flow_upload(self._h, p0, p1), "f3d_flow_upload")

    def compute_resident(self, silent=True, initial=None, **kw):
        """solve the uploaded pair; `initial` (see set_initial) starts the pyramid from a displacement instead of zero"""
        prm = make_params(**kw)
        secs = C.c_float()
        if initial is not None:
            self.set_initial(initial)
            _host_check(host().f3d_flow_compute_resident_from_initial(self._h, C.byref(prm), int(silent), C.byref(secs)),
                        "f3d_flow_compute_resident_from_initial")
            return secs.value
        check(host().f3d_flow_compute_resident(self._h, C.byref(prm), int(silent), C.byref(secs)),
              "f3d_flow_compute_resident")
        return secs.value

    def download(self):
        w, h, d = self.dims
        u, v, ww = (np.empty((d, h, w), np.float32) for _ in range(3))
        check(host().f3d_flow_download(self._h, u.ctypes.data_as(_fp), v.ctypes.data_as(_fp), ww.ctypes.data_as(_fp)))
        return u, v, ww

    # ---- the displacement a solve starts from (include/f3d_host.h, f3d_flow_initial_*) ----
    def set_initial(self, initial):
        """Hold `initial` as the flow the next compute(initial=...) calls start their pyramid from: a tuple of three [z, y, x]
        arrays (a guess from outside), "flow" (a copy of what compute_resident() left on the device) or "trajectory" (a copy of the
        cumulative displacement).  A voxel with a component that is not finite starts from zero.  Returns the InitialInfo.  The
        flow is kept, unchanged by any solve, until it is set again, initial_end() or destroy().  "block-match": the guess of
        block_match() with its defaults on the uploaded pair, through set_initial_from_nodes().  "held": whatever is held already
        (set_initial or set_initial_from_nodes before), nothing is set and None is returned."""
        info = InitialInfo()
        if isinstance(initial, str) and initial == "held":
            return None
        if isinstance(initial, str) and initial == "block-match":
            self.block_match()
            return self.set_initial_from_nodes()[1]
        if isinstance(initial, str):
            _host_check(host().f3d_flow_initial_take(self._h, _source(initial), C.byref(info)), "f3d_flow_initial_take")
            return info
        parts = list(initial)
        w, h, d = self.dims
        if len(parts) != 3:
            raise ValueError("initial must be 'flow', 'trajectory' or three [z, y, x] volumes")
        held = [_f32(a) for a in parts]
        if any(a.shape != (d, h, w) for a, _ in held):
            raise ValueError(f"the components of the initial flow must be [z,y,x] = {(d, h, w)}")
        _host_check(host().f3d_flow_initial_upload(self._h, held[0][1], held[1][1], held[2][1], C.byref(info)), "f3d_flow_initial_upload")
        return info

    def initial_download(self):
        """(u, v, w): the prepared initial flow as the solve will read it"""
        w, h, d = self.dims
        u, v, ww = (np.empty((d, h, w), np.float32) for _ in range(3))
        _host_check(host().f3d_flow_initial_download(self._h, u.ctypes.data_as(_fp), v.ctypes.data_as(_fp), ww.ctypes.data_as(_fp)),
                    "f3d_flow_initial_download")
        return u, v, ww

    def initial_end(self):
        """free the containers of the initial flow (destroy() does too)"""
        _host_check(host().f3d_flow_initial_end(self._h), "f3d_flow_initial_end")

    # ---- the guess from the frames themselves (include/f3d_host.h, f3d_flow_block_match, f3d_flow_initial_from_nodes) ----
    def block_match(self, step=16, window=8, search=8, bins=256, range=None, centre=None, min_zncc=0.5):
        """block_match() of the module on the pair the driver holds (upload first), on the library stream; the grid is the one
        block_match_grid lays over the volume.  Returns a BlockMatchNodes; the table also stays with the driver for
        set_initial_from_nodes()."""
        radii = (int(search),) * 3 if np.isscalar(search) else tuple(int(r) for r in search)
        if len(radii) != 3:
            raise ValueError("search must be one radius or three")
        grid = BlockMatchGrid()
        _host_check(host().f3d_block_match_layout(*self.dims, int(step), int(window), *radii, C.byref(grid)), "f3d_block_match_layout")
        nodes = grid.nx * grid.ny * grid.nz
        centre = _centre_array(centre, nodes)
        bounds = None if range is None else (C.c_float * 2)(*_bin_range(range))
        info, summary = BlockMatchInfo(), BlockMatchSummary()
        _host_check(host().f3d_flow_block_match(self._h, int(step), int(window), *radii, int(bins), bounds,
                                                None if centre is None else centre.ctypes.data, float(min_zncc), C.byref(grid),
                                                C.byref(info), C.byref(summary)), "f3d_flow_block_match")
        records, rows = np.zeros((nodes, BLOCK_MATCH_RECORD_WORDS), np.int32), np.zeros(nodes, BLOCK_MATCH_NODE)
        _host_check(host().f3d_flow_block_match_rows(self._h, nodes, records.ctypes.data, rows.ctypes.data), "f3d_flow_block_match_rows")
        return BlockMatchNodes(rows, records, info.as_dict(), summary.as_dict(), grid, centre)

    def set_initial_from_nodes(self):
        """Hold the guess of the last block_match() as the flow compute_resident(initial=True) starts from: the node vectors through
        the median test on the node grid (validate_displacement, replace mode, its defaults), expanded over the volume (expand_nodes)
        and prepared as set_initial prepares a flow.  Returns (the dict of the median test's statistics, InitialInfo)."""
        validated, info = ValidateStats(), InitialInfo()
        _host_check(host().f3d_flow_initial_from_nodes(self._h, C.byref(validated), C.byref(info)), "f3d_flow_initial_from_nodes")
        return validated.as_dict(), info

    def subset_match(self, start="flow", step=16, window=8, model="affine", max_iterations=20, tolerance=1e-3, reach=None, min_zncc=0.8):
        """subset_match() of the module on the pair the driver holds (upload first), on the library stream, on the grid
        subset_grid lays over the volume.  start: "zero"; "block-match", the table of the last block_match() (each node takes the
        vector of the nearest block-match node, NaN unless that one is ok or edge); "flow", the held flow at the node voxels
        (compute_resident first).  Whenever a flow is held it is also the comparison: the summary has the rms, median and 95 %
        quantile of |flow - subset| over the accepted nodes.  Returns a SubsetNodes; the table also stays with the driver."""
        sources = {"zero": 0, "block-match": 1, "flow": 2}
        if start not in sources or model not in SUBSET_MODELS:
            raise ValueError(f"start must be one of {sorted(sources)} and model one of {sorted(SUBSET_MODELS)}")
        grid, info, summary = SubsetGrid(), SubsetInfo(), SubsetSummary()
        _host_check(host().f3d_flow_subset_match(self._h, int(step), int(window), SUBSET_MODELS[model], sources[start], int(max_iterations),
                                                 float(tolerance), 0.0 if reach is None else float(reach), float(min_zncc), C.byref(grid),
                                                 C.byref(info), C.byref(summary)), "f3d_flow_subset_match")
        nodes = grid.nx * grid.ny * grid.nz
        records, rows = np.zeros(nodes, SUBSET_RECORD), np.zeros(nodes, SUBSET_NODE)
        _host_check(host().f3d_flow_subset_match_rows(self._h, nodes, records.ctypes.data, rows.ctypes.data), "f3d_flow_subset_match_rows")
        return SubsetNodes(rows, records, info.as_dict(), summary.as_dict(), grid)

    def set_level_stats(self, enable=True):
        """record, per pyramid level of every later compute, the residual before the solve and the flow statistics after it"""
        check(host().f3d_flow_set_level_stats(self._h, int(bool(enable))))

    def level_stats(self):
        """list of dicts, coarsest level first"""
        n = _sz()
        check(host().f3d_flow_level_stat_count(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            st = LevelStat()
            check(host().f3d_flow_level_stat(self._h, i, C.byref(st)))
            out.append({k: getattr(st, k) for k, _ in LevelStat._fields_})
        return out

    def final_residual(self):
        """((rms, mean |.|, max |.|) of frame_1 registered with the flow on the device against frame_0, the same unregistered)"""
        a, b = (C.c_double * 3)(), (C.c_double * 3)()
        check(host().f3d_flow_final_residual(self._h, a, b), "f3d_flow_final_residual")
        return tuple(a), tuple(b)

    # ---- trajectory of a frame sequence (include/f3d_host.h, f3d_flow_trajectory_*) ----
    def trajectory_begin(self):
        """start (or restart) the cumulative displacement at zero; allocates three containers on first use"""
        _host_check(host().f3d_flow_trajectory_begin(self._h), "f3d_flow_trajectory_begin")

    def trajectory_append(self):
        """compose the flow of the last compute_resident() into the displacement, on the device"""
        _host_check(host().f3d_flow_trajectory_append(self._h), "f3d_flow_trajectory_append")

    def trajectory_download(self):
        """(u, v, w, lost): the displacement of every voxel of frame 0 (frame 0's grid, voxel units; NaN where the point has left
        the volume) and the number of voxels whose u is NaN"""
        w, h, d = self.dims
        u, v, ww = (np.empty((d, h, w), np.float32) for _ in range(3))
        lost = C.c_ulonglong()
        _host_check(host().f3d_flow_trajectory_download(self._h, u.ctypes.data_as(_fp), v.ctypes.data_as(_fp),
                                                        ww.ctypes.data_as(_fp), C.byref(lost)), "f3d_flow_trajectory_download")
        return u, v, ww, int(lost.value)

    def trajectory_end(self):
        _host_check(host().f3d_flow_trajectory_end(self._h), "f3d_flow_trajectory_end")

    # ---- derived fields of the held flow or the trajectory (include/f3d_host.h, f3d_flow_{strain,principal,polar,inverse,match,motion,label_motion,validate}_*) ----
    def _derived(self, compute, src, selected, stats, *args, fit=None):
        """one f3d_flow_*_compute into fresh host arrays: a list with an array per selected output and None for the others
        (fit: the MotionFit f3d_flow_motion_compute takes between the arrays and the statistics)"""
        w, h, d = self.dims
        arrays = [np.empty((d, h, w), np.float32) if s else None for s in selected]
        ptrs = (_fp * len(arrays))(*[a.ctypes.data_as(_fp) if a is not None else None for a in arrays])
        tail = (C.byref(stats),) if fit is None else (C.byref(fit), C.byref(stats))
        _host_check(getattr(host(), compute)(self._h, src, *args, ptrs, *tail), compute)
        return arrays

    def strain(self, source="flow", fields=("vol", "e", "eq")):
        """Strain fields of the flow the driver holds (source="flow", after compute_resident) or of the trajectory
        (source="trajectory", after trajectory_begin); same result shape as flow_strain().  Works between the yields of
        compute_sequence, where the driver holds both."""
        src, mask, stats = _source(source), _strain_mask(fields), StrainStats()
        arrays = self._derived("f3d_flow_strain_compute", src, [mask & g for g in _STRAIN_GROUP_OF], stats, mask)
        res = {n: a for n, a in zip(STRAIN_NAMES, arrays) if a is not None}
        res["stats"] = stats.as_dict()
        return res

    def strain_end(self):
        """free the strain containers (destroy() does too)"""
        _host_check(host().f3d_flow_strain_end(self._h), "f3d_flow_strain_end")

    def window_strain(self, source="flow", radius=2, min_count=None, fields=("vol", "e", "eq")):
        """Strain fields over a strain window of the flow the driver holds (source="flow", after compute_resident) or of the
        trajectory (source="trajectory", after trajectory_begin); same arguments and result shape as window_strain().  Works between
        the yields of compute_sequence, where the driver holds both."""
        src, mask, stats = _source(source), _window_strain_mask(fields), WindowStrainStats()
        arrays = self._derived("f3d_flow_window_strain_compute", src, [mask & g for g in _WINDOW_STRAIN_GROUP_OF], stats, mask, radius,
                               _window_min_count(radius, min_count))
        res = {n: a for n, a in zip(WINDOW_STRAIN_NAMES, arrays) if a is not None}
        res["stats"] = stats.as_dict()
        return res

    def window_strain_end(self):
        """free the window strain containers (destroy() does too)"""
        _host_check(host().f3d_flow_window_strain_end(self._h), "f3d_flow_window_strain_end")

    def principal(self, source="flow", fields=("val", "shear")):
        """Principal strains of the flow the driver holds (source="flow", after compute_resident) or of the trajectory
        (source="trajectory", after trajectory_begin); same result shape as principal_strain().  Works between the yields of
        compute_sequence, where the driver holds both."""
        src, mask, stats = _source(source), _principal_mask(fields), PrincipalStats()
        arrays = self._derived("f3d_flow_principal_compute", src, [mask & g for g in _PRINCIPAL_GROUP_OF], stats, mask)
        res = {n: a for n, a in zip(PRINCIPAL_NAMES, arrays) if a is not None}
        res["stats"] = stats.as_dict()
        return res

    def principal_end(self):
        """free the principal strain containers (destroy() does too)"""
        _host_check(host().f3d_flow_principal_end(self._h), "f3d_flow_principal_end")

    def rotation(self, source="flow", fields=("angle", "vector", "stretch")):
        """Local rotation and principal stretches of the flow the driver holds (source="flow", after compute_resident) or of the
        trajectory (source="trajectory", after trajectory_begin); same result shape as polar_decomposition().  Works between the
        yields of compute_sequence, where the driver holds both."""
        src, mask, stats = _source(source), _polar_mask(fields), PolarStats()
        arrays = self._derived("f3d_flow_polar_compute", src, [mask & g for g in _POLAR_GROUP_OF], stats, mask)
        res = {n: a for n, a in zip(POLAR_NAMES, arrays) if a is not None}
        res["stats"] = stats.as_dict()
        return res

    def rotation_end(self):
        """free the rotation and stretch containers (destroy() does too)"""
        _host_check(host().f3d_flow_polar_end(self._h), "f3d_flow_polar_end")

    def window_principal(self, source="flow", radius=2, min_count=None, fields=("val", "shear")):
        """Principal strains from the least-squares gradient over a strain window of the flow the driver holds (source="flow") or of
        the trajectory (source="trajectory"); same arguments and result shape as window_principal().  The call depends on its
        arguments only: it needs no window_strain() before it and leaves that one's containers as they are."""
        src, mask, stats = _source(source), _principal_mask(fields), PrincipalStats()
        radius, min_count = _window_args(radius, min_count)
        arrays = self._derived("f3d_flow_window_principal_compute", src, [mask & g for g in _PRINCIPAL_GROUP_OF], stats, mask, radius,
                               min_count)
        res = {n: a for n, a in zip(PRINCIPAL_NAMES, arrays) if a is not None}
        res["stats"] = stats.as_dict()
        return res

    def window_principal_end(self):
        """free the window principal strain containers, and the gradient's when window_rotation holds none (destroy() does too)"""
        _host_check(host().f3d_flow_window_principal_end(self._h), "f3d_flow_window_principal_end")

    def window_rotation(self, source="flow", radius=2, min_count=None, fields=("angle", "vector", "stretch")):
        """Local rotation and principal stretches from the least-squares gradient over a strain window of the flow the driver holds
        (source="flow") or of the trajectory (source="trajectory"); same arguments and result shape as window_rotation()."""
        src, mask, stats = _source(source), _polar_mask(fields), PolarStats()
        radius, min_count = _window_args(radius, min_count)
        arrays = self._derived("f3d_flow_window_polar_compute", src, [mask & g for g in _POLAR_GROUP_OF], stats, mask, radius, min_count)
        res = {n: a for n, a in zip(POLAR_NAMES, arrays) if a is not None}
        res["stats"] = stats.as_dict()
        return res

    def window_rotation_end(self):
        """free the window rotation and stretch containers, and the gradient's when window_principal holds none (destroy() does too)"""
        _host_check(host().f3d_flow_window_polar_end(self._h), "f3d_flow_window_polar_end")

    def inverse(self, source="flow", iterations=32, tolerance=1e-3):
        """The inverse displacement of the flow the driver holds (source="flow", after compute_resident) or of the trajectory
        (source="trajectory", after trajectory_begin); same result shape as invert_displacement().  Works between the yields of
        compute_sequence, where the driver holds both."""
        stats = InverseStats()
        arrays = self._derived("f3d_flow_inverse_compute", _source(source), [True] * 4, stats, iterations, tolerance)
        return tuple(arrays) + (stats.as_dict(),)

    def inverse_end(self):
        """free the inverse displacement containers (destroy() does too)"""
        _host_check(host().f3d_flow_inverse_end(self._h), "f3d_flow_inverse_end")

    def match(self, fields=("zncc", "rmsd"), radius=3, threshold=0.8):
        """Match quality of the flow the driver holds against the frames it holds (after upload + compute_resident): frame 1 carried
        onto frame 0's grid through the flow ("warped", NaN where the point leaves the volume) and its local correlation with frame 0
        ("zncc", "rmsd"; local_correlation() has the definition).  Returns a dict name -> array for the selected fields and
        "stats" -> dict.  Works between the yields of compute_sequence for the pair just solved; the cumulative displacement has no
        match quality (frame 0 is not kept)."""
        mask, stats = _mask(fields, MATCH_GROUPS, "match"), CorrelationStats()
        arrays = self._derived("f3d_flow_match_compute", 0, [mask & g for g in MATCH_GROUPS.values()], stats, mask, radius, threshold)
        res = {n: a for n, a in zip(MATCH_NAMES, arrays) if a is not None}
        res["stats"] = stats.as_dict()
        return res

    def match_end(self):
        """free the match quality containers (destroy() does too)"""
        _host_check(host().f3d_flow_match_end(self._h), "f3d_flow_match_end")

    def motion(self, source="flow", model="rigid", min_zncc=None):
        """The motion of the flow the driver holds (source="flow") or of the trajectory (source="trajectory") fitted and taken out on
        the device: a dict with the residual "u", "v", "w", "fit" -> MotionFit and "stats" -> dict (present, sum_sq, max_abs).
        min_zncc: fit only where the zncc of the last match() of this pair is at least that (match() first; not for the trajectory)."""
        fit, stats = MotionFit(), MotionResidual()
        arrays = self._derived("f3d_flow_motion_compute", _source(source), [True] * 3, stats, _motion_model(model),
                               float("nan") if min_zncc is None else min_zncc, fit=fit)
        res = dict(zip("uvw", arrays))
        res["fit"], res["stats"] = fit, stats.as_dict()
        return res

    def motion_end(self):
        """free the motion residual containers (destroy() does too)"""
        _host_check(host().f3d_flow_motion_end(self._h), "f3d_flow_motion_end")

    def label_motion(self, labels, source="flow", model="rigid", min_voxels=27, n_labels=None):
        """The motion of every label of a segmentation in the flow the driver holds (source="flow") or in the trajectory
        (source="trajectory"), fitted and taken out on the device: a dict with the residual "u", "v", "w" (NaN where a voxel's label
        has no fit), "motion" -> LabelMotion (with .rms_after and .info).  labels: an integer [z, y, x] volume on the grid of the
        displacement, or None for the labels of the previous call, which the driver keeps on the device (n_labels is then required)."""
        w, h, d = self.dims
        if labels is None:
            if n_labels is None:
                raise ValueError("n_labels is required when the labels of the previous call are reused")
            lab, ptr = None, None
        else:
            bits, n_labels = _labels_as_float_bits(labels, n_labels)
            if bits.shape != (d, h, w):
                raise ValueError(f"labels must be a [z, y, x] volume of shape {(d, h, w)}")
            lab = bits.view(np.int32)
            ptr = lab.ctypes.data_as(C.POINTER(C.c_int))
        n = int(n_labels)
        if not 1 <= n <= MAX_LABELS:
            raise ValueError(f"n_labels must be 1 .. {MAX_LABELS}, not {n}")
        fits, status, rms, info = (MotionFit * n)(), (C.c_int * n)(), (C.c_double * n)(), LabelInfo()
        arrays = [np.empty((d, h, w), np.float32) for _ in range(3)]
        ptrs = (_fp * 3)(*[a.ctypes.data_as(_fp) for a in arrays])
        _host_check(host().f3d_flow_label_motion_compute(self._h, _source(source), ptr, n, _motion_model(model), int(min_voxels), ptrs,
                                                         fits, status, rms, C.byref(info)), "f3d_flow_label_motion_compute")
        motion = LabelMotion(fits, status, model)
        motion.rms_after = np.array(list(rms), np.float64)
        motion.info = info.as_dict()
        res = dict(zip("uvw", arrays))
        res["motion"] = motion
        return res

    def label_motion_end(self):
        """free the containers of the per-label residual and of the labels (destroy() does too)"""
        _host_check(host().f3d_flow_label_motion_end(self._h), "f3d_flow_label_motion_end")

    def histogram(self, bins=256, range=None):
        """The grey-value histogram of the resident frame 0, the frame segment() thresholds (include/f3d_host.h, f3d_flow_histogram): a
        Histogram over range = (lo, hi), or over the frame's finite minimum and maximum when range is None."""
        bins = _bins(bins)
        bounds = None if range is None else (C.c_float * 2)(*_bin_range(range))
        counts, info, lo, hi = np.zeros(bins, np.uint64), HistogramInfo(), C.c_float(), C.c_float()
        _host_check(host().f3d_flow_histogram(self._h, 0, bounds, bins, counts.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(info),
                                              C.byref(lo), C.byref(hi)), "f3d_flow_histogram")
        return Histogram(counts, lo.value, hi.value, info.as_dict())

    def _otsu_bounds(self, lo, hi, bins, value_range):
        """lo and hi of segment() with the strings of OTSU_TOKENS replaced: on the lo side by the edge e of the cut (s >= e), on the hi
        side by the largest float32 below it (s < e)"""
        tokens = [b for b in (lo, hi) if isinstance(b, str)]
        if not tokens:
            return lo, hi
        for t in tokens:
            if t not in OTSU_TOKENS:
                raise ValueError(f"lo and hi must be numbers or one of {sorted(OTSU_TOKENS)}, not {t!r}")
        classes = {OTSU_TOKENS[t][0] for t in tokens}
        if len(classes) != 1:
            raise ValueError("'otsu' is the cut of two classes, 'otsu1' and 'otsu2' are the cuts of three: they cannot be mixed")
        if len(tokens) == 2 and OTSU_TOKENS[lo][1] >= OTSU_TOKENS[hi][1]:
            raise ValueError(f"lo {lo!r} is above hi {hi!r}")
        found = self.histogram(bins, value_range).otsu(classes.pop())
        if found.status != OTSU_OK:
            raise F3dError("segment: fewer bins of the frame's histogram are occupied than classes: there is no Otsu cut")
        if isinstance(lo, str):
            lo = found.values[OTSU_TOKENS[lo][1]]
        if isinstance(hi, str):
            hi = np.nextafter(found.values[OTSU_TOKENS[hi][1]], np.float32(-np.inf))
        return lo, hi

    def segment(self, lo=-np.inf, hi=np.inf, min_voxels=27, split=None, bins=256, value_range=None):
        """The connected bodies of the resident frame 0 (the raw frame of the last upload()), labelled on the device and left there: a
        Components, after which label_motion(None, ..., n_labels=c.n_labels) and contacts(None, n_labels=c.n_labels) run on these
        bodies.  lo, hi, min_voxels as in label_components.  split: None, or the core_d2 of split_components (an integer of at least 1,
        e.g. ceil(radius^2)), which takes touching bodies apart; the info is then that of f3d_split_info.  lo or hi may also be "otsu"
        (the cut of two classes) or "otsu1" / "otsu2" (the lower and upper cut of three) of histogram(bins, value_range): as lo the
        foreground starts at the cut, as hi it ends below it."""
        lo, hi = self._otsu_bounds(lo, hi, bins, value_range)
        lo, hi, min_voxels = _component_range(lo, hi, min_voxels)
        w, h, d = self.dims
        sizes, count = C.POINTER(C.c_ulonglong)(), _sz(0)
        if split is None:
            info = ComponentInfo()
            _host_check(host().f3d_flow_labels_compute(self._h, 0, lo, hi, min_voxels, C.byref(sizes), C.byref(count), C.byref(info)),
                        "f3d_flow_labels_compute")
        else:
            info = SplitInfo()
            _host_check(host().f3d_flow_labels_split(self._h, 0, lo, hi, _core_d2(None, split), min_voxels, C.byref(sizes), C.byref(count),
                                                     C.byref(info)), "f3d_flow_labels_split")
        own = np.array(sizes[:count.value], np.uint64)         # the driver owns its list: a copy outlives the next call
        labels = np.empty((d, h, w), np.int32)
        _host_check(host().f3d_flow_labels_download(self._h, labels.ctypes.data_as(C.POINTER(C.c_int))), "f3d_flow_labels_download")
        self._segmented_labels = int(info.n_labels)            # what label_shapes() takes for n_labels when it is not given
        self._segment_settled = (lo, hi, min_voxels, split)    # what segment_next() repeats on the later frame: the cuts as numbers
        return Components(labels, own, info.as_dict())

    def segment_next(self, lo=None, hi=None, min_voxels=None, split=None):
        """The bodies of the resident LATER frame (the raw frame 1 of the last upload()), labelled on the device into a second label
        volume, "B", beside the one segment() fills: a Components, after which track() finds which body of it is which body of frame
        0.  lo, hi, min_voxels and split as in segment(), numbers only; with all four None, what the last segment() settled (an Otsu
        cut of frame 0 is kept as the number it came to and not taken again on this frame)."""
        if lo is None and hi is None and min_voxels is None and split is None:
            settled = getattr(self, "_segment_settled", None)
            if settled is None:
                raise ValueError("segment_next() without arguments repeats the last segment(), and there was none")
            lo, hi, min_voxels, split = settled
        else:
            lo = -np.inf if lo is None else lo
            hi = np.inf if hi is None else hi
            if isinstance(lo, str) or isinstance(hi, str):
                raise ValueError("segment_next() takes numbers for lo and hi: an Otsu cut is not taken again on the later frame")
            lo, hi, min_voxels = _component_range(lo, hi, 27 if min_voxels is None else min_voxels)
        w, h, d = self.dims
        sizes, count, info = C.POINTER(C.c_ulonglong)(), _sz(0), SplitInfo()
        core_d2 = 0 if split is None else _core_d2(None, split)
        _host_check(host().f3d_flow_labels_b_segment(self._h, 0, lo, hi, core_d2, min_voxels, C.byref(sizes), C.byref(count), C.byref(info)),
                    "f3d_flow_labels_b_segment")
        own = np.array(sizes[:count.value], np.uint64)         # the driver owns its list: a copy outlives the next call
        labels = np.empty((d, h, w), np.int32)
        _host_check(host().f3d_flow_labels_b_download(self._h, labels.ctypes.data_as(C.POINTER(C.c_int))), "f3d_flow_labels_b_download")
        self._segmented_labels_b = int(info.n_labels)
        found = info.as_dict()
        if split is None:                                      # the counters of f3d_component_info alone
            found = {name: found[name] for name, _ in ComponentInfo._fields_}
        return Components(labels, own, found)

    def track(self, labels_b=None, source="flow", n_a=None, n_b=None, min_fraction=0.1, relabel=True):
        """Which body of the second label volume is which body of the labels on frame 0's grid, through the flow the driver holds
        (source="flow") or the trajectory (source="trajectory"): f3d_label_overlap on the device, f3d_overlap_solve on the host and,
        with relabel, f3d_relabel_labels of the second volume on the device.  labels_b: an integer [z, y, x] volume on the grid the
        displacement leads to, or None for the bodies segment_next() left on the device.  n_a / n_b None mean the number of bodies of
        the last segment() / segment_next() (labels_b.max() when labels_b is given).  Returns a Tracks with .info, .overlaps and, with
        relabel, .relabelled: the second volume under frame 0's numbers, which also replaces it on the device."""
        w, h, d = self.dims
        if labels_b is not None:
            bits, n_b = _labels_as_float_bits(labels_b, n_b)
            if bits.shape != (d, h, w):
                raise ValueError(f"labels_b must be a [z, y, x] volume of shape {(d, h, w)}")
            lab = bits.view(np.int32)
            _host_check(host().f3d_flow_labels_b_upload(self._h, lab.ctypes.data_as(C.POINTER(C.c_int))), "f3d_flow_labels_b_upload")
        elif n_b is None:
            n_b = getattr(self, "_segmented_labels_b", None)
        if n_a is None:
            n_a = getattr(self, "_segmented_labels", None)
        if n_a is None or n_b is None:
            raise ValueError("n_a and n_b are required when the labels on the device were not made by segment() and segment_next()")
        n_a, n_b = int(n_a), int(n_b)
        if not (1 <= n_a <= MAX_LABELS and 1 <= n_b <= MAX_LABELS):
            raise ValueError(f"n_a and n_b must be 1 .. {MAX_LABELS}, not {n_a} and {n_b}")
        if not 0.0 < float(min_fraction) <= 1.0:
            raise ValueError(f"min_fraction must be in (0, 1], not {min_fraction}")
        rows, count, info = C.POINTER(Overlap)(), _sz(0), OverlapInfo()
        _host_check(host().f3d_flow_overlap_compute(self._h, _source(source), n_a, n_b, C.byref(rows), C.byref(count), C.byref(info)),
                    "f3d_flow_overlap_compute")
        own = (Overlap * max(count.value, 1))()                # the driver owns its list: a copy outlives the next call
        if count.value:
            C.memmove(own, rows, count.value * C.sizeof(Overlap))
        overlaps = Overlaps(own, count.value, info.as_dict())
        tracks = solve_overlaps(overlaps, n_a, n_b, min_fraction)
        tracks.info, tracks.overlaps = overlaps.info, overlaps
        if relabel:
            _host_check(host().f3d_flow_labels_b_relabel(self._h, tracks.map_b.ctypes.data_as(C.POINTER(C.c_int)), n_b),
                        "f3d_flow_labels_b_relabel")
            tracks.relabelled = np.empty((d, h, w), np.int32)
            _host_check(host().f3d_flow_labels_b_download(self._h, tracks.relabelled.ctypes.data_as(C.POINTER(C.c_int))),
                        "f3d_flow_labels_b_download")
            self._segmented_labels_b = max(int(tracks.summary["n_ids"]), 1)   # the second volume now carries these numbers
        return tracks

    def track_end(self):
        """free the driver's list of overlaps (both label volumes stay on the device until label_motion_end() or destroy())"""
        _host_check(host().f3d_flow_overlap_end(self._h), "f3d_flow_overlap_end")

    def label_shapes(self, labels=None, n_labels=None):
        """The shape table of a segmentation on the grid of the driver: a LabelShapes (see there) with .info.  labels: an integer
        [z, y, x] volume, or None for the labels segment(), label_motion() or contacts() left on the device; n_labels None then
        means the number of bodies of the last segment().  No displacement is needed: this runs before any solve."""
        w, h, d = self.dims
        if labels is None:
            if n_labels is None:
                n_labels = getattr(self, "_segmented_labels", None)
            if n_labels is None:
                raise ValueError("n_labels is required when the labels on the device were not made by segment()")
            ptr = None
        else:
            bits, n_labels = _labels_as_float_bits(labels, n_labels)
            if bits.shape != (d, h, w):
                raise ValueError(f"labels must be a [z, y, x] volume of shape {(d, h, w)}")
            lab = bits.view(np.int32)
            ptr = lab.ctypes.data_as(C.POINTER(C.c_int))
        n = int(n_labels)
        if not 1 <= n <= MAX_LABELS:
            raise ValueError(f"n_labels must be 1 .. {MAX_LABELS}, not {n}")
        out, info = (LabelShape * n)(), LabelShapeInfo()
        _host_check(host().f3d_flow_label_shapes_compute(self._h, ptr, n, out, C.byref(info)), "f3d_flow_label_shapes_compute")
        return LabelShapes(_shape_rows(out, n), info.as_dict())

    def _device_labels(self, n_labels):
        if n_labels is None:
            n_labels = getattr(self, "_segmented_labels", None)
        if n_labels is None:
            raise ValueError("n_labels is required when the labels on the device were not made by segment()")
        n = int(n_labels)
        if not 1 <= n <= MAX_LABELS:
            raise ValueError(f"n_labels must be 1 .. {MAX_LABELS}, not {n}")
        return n

    def label_field(self, field="eq", n_labels=None, shift=None, bins=0, range=None, min_voxels=1):
        """The statistics of a field per body of the labels segment(), label_motion(), contacts() or label_shapes() left on the device: a
        LabelFieldStats (see there).  field: the name of a field the driver holds -- "grey" (the raw frame 0 of the last upload()),
        "vol", "eq" (after strain()), "gmax" (principal()), "angle" (rotation()), "zncc", "rmsd" (match()), "wvol", "weq"
        (window_strain()) -- which stays on the device, or a [z, y, x] array on the driver's grid, which is taken through
        label_field_stats with the downloaded labels.  n_labels None means the number of bodies of the last segment(); shift, bins,
        range and min_voxels as in label_field_sums and solve_label_field."""
        n = self._device_labels(n_labels)
        bins, shift = _field_bins(bins), _field_shift(shift)
        bounds = None if range is None else _bin_range(range)
        w, h, d = self.dims
        if not isinstance(field, str):
            field = np.asarray(field)
            if field.shape != (d, h, w):
                raise ValueError(f"field must be a name or a [z, y, x] volume of shape {(d, h, w)}")
            labels = np.empty((d, h, w), np.int32)
            _host_check(host().f3d_flow_labels_download(self._h, labels.ctypes.data_as(C.POINTER(C.c_int))), "f3d_flow_labels_download")
            return label_field_stats(field, labels, n, shift, bins, range, min_voxels)
        if n * bins > MAX_LABEL_FIELD_COUNTS:
            raise ValueError(f"n_labels * bins must be at most 2^26, not {n} * {bins}")
        ptr = _dp(0)
        _host_check(host().f3d_flow_field_container(self._h, field.encode(), C.byref(ptr)), "f3d_flow_field_container")
        note = None
        if shift is None or (bins and bounds is None):
            lo, hi, found = C.c_float(), C.c_float(), RangeInfo()
            _host_check(host().f3d_flow_label_field_range(self._h, ptr, C.byref(lo), C.byref(hi), C.byref(found)),
                        "f3d_flow_label_field_range")
            shift, bins, bounds, note = _field_settings(shift, bins, bounds, lo.value, hi.value, found.finite)
        out, info, summary = (LabelFieldStat * n)(), LabelFieldInfo(), LabelFieldSummary()
        counts = np.zeros((n, bins), np.uint32) if bins else None
        _host_check(host().f3d_flow_label_field_compute(self._h, ptr, n, shift, (C.c_float * 2)(*bounds) if bins else None, bins,
                                                        int(min_voxels), out, counts.ctypes.data_as(C.POINTER(C.c_uint)) if bins else None,
                                                        C.byref(info), C.byref(summary)), "f3d_flow_label_field_compute")
        found = info.as_dict()
        if note:
            found["note"] = note
        sums = LabelFieldSums(np.zeros(0, _FIELD_SUMS_DTYPE), counts, shift, bounds[0] if bins else None, bounds[1] if bins else None, found)
        return _field_stats_result(out, n, summary, sums)

    def paint_labels(self, values):
        """values[l - 1] painted into the voxels of label l of the labels on the device, NaN elsewhere (f3d_paint_labels): a float32
        [z, y, x] volume, e.g. paint_labels(label_field("eq").mean)."""
        values = _paint_values(values)
        w, h, d = self.dims
        out = np.empty((d, h, w), np.float32)
        _host_check(host().f3d_flow_labels_paint(self._h, values.ctypes.data_as(_fp), len(values), out.ctypes.data_as(_fp)),
                    "f3d_flow_labels_paint")
        return out

    def segment_end(self):
        """free the driver's list of sizes (the labels stay on the device until label_motion_end() or destroy())"""
        _host_check(host().f3d_flow_labels_end(self._h), "f3d_flow_labels_end")

    def contacts(self, labels, source="flow", motion=None, n_labels=None, min_faces=4):
        """The contacts between the bodies of a segmentation in the flow the driver holds (source="flow") or in the trajectory
        (source="trajectory"): a Contacts whose .kinematics is contact_kinematics of it (the fit columns filled from `motion`, the
        LabelMotion of the same labels, e.g. label_motion(...)["motion"]).  labels: an integer [z, y, x] volume on the grid of the
        displacement, or None for the labels an earlier contacts() or label_motion() left on the device (n_labels is then required)."""
        w, h, d = self.dims
        if labels is None:
            if n_labels is None:
                raise ValueError("n_labels is required when the labels of the previous call are reused")
            ptr = None
        else:
            bits, n_labels = _labels_as_float_bits(labels, n_labels)
            if bits.shape != (d, h, w):
                raise ValueError(f"labels must be a [z, y, x] volume of shape {(d, h, w)}")
            lab = bits.view(np.int32)
            ptr = lab.ctypes.data_as(C.POINTER(C.c_int))
        n = int(n_labels)
        if not 1 <= n <= MAX_LABELS:
            raise ValueError(f"n_labels must be 1 .. {MAX_LABELS}, not {n}")
        if motion is not None and len(motion) != n:
            raise ValueError(f"motion has {len(motion)} labels, not {n}")
        rows, count, info = C.POINTER(Contact)(), _sz(0), ContactInfo()
        _host_check(host().f3d_flow_contacts_compute(self._h, _source(source), ptr, n, C.byref(rows), C.byref(count), C.byref(info)),
                    "f3d_flow_contacts_compute")
        own = (Contact * max(count.value, 1))()                # the driver owns its list: a copy outlives the next call
        if count.value:
            C.memmove(own, rows, count.value * C.sizeof(Contact))
        found = Contacts(own, count.value, info.as_dict())
        found.kinematics = contact_kinematics(found, (w, h, d), motion, min_faces)
        return found

    def contacts_end(self):
        """free the driver's list of contacts (the labels stay on the device until label_motion_end() or destroy())"""
        _host_check(host().f3d_flow_contacts_end(self._h), "f3d_flow_contacts_end")

    def validate(self, source="flow", step=1, eps=0.1, threshold=2.0, min_neighbours=9, mode="replace", fill_passes=0,
                 fields=("r", "d"), min_zncc=None):
        """The flow the driver holds (source="flow") or the trajectory (source="trajectory") validated on the device by the normalised
        median test (validate_displacement has the parameters): a dict name -> array for "r" and / or "u", "v", "w" as `fields` selects,
        and "stats" -> dict.  min_zncc: voxels whose zncc of the last match() of this pair is below that are rejected as well and are
        no neighbour of anyone (match() first; not for the trajectory)."""
        mask = _mask(fields, VALIDATE_GROUPS, "validation")
        stats = ValidateStats()
        arrays = self._derived("f3d_flow_validate_compute", _source(source), [bool(mask & g) for g in _VALIDATE_GROUP_OF], stats, step,
                               eps, threshold, min_neighbours, _validate_mode(mode), fill_passes,
                               float("nan") if min_zncc is None else min_zncc)
        res = {n: a for n, a in zip(VALIDATE_NAMES, arrays) if a is not None}
        res["stats"] = stats.as_dict()
        return res

    def validate_end(self):
        """free the containers of the validated displacement (destroy() does too)"""
        _host_check(host().f3d_flow_validate_end(self._h), "f3d_flow_validate_end")

    def compute_sequence(self, frames, cumulative=False, silent=True, total=False, warm_start=False, initial=None, **kw):
        """Generator over the pairs of `frames` (an iterable of [z, y, x] volumes): yields (k, (u, v, w), disp) for pair k, where disp
        is None, or with cumulative=True the trajectory_download() tuple (u, v, w, lost) of the displacement frame 0 -> frame k+1.
        Each pair is uploaded and solved with compute_resident().  Pair k is frame k -> k+1, unless total=True: then it is
        frame 0 -> frame k+1, solved directly and started from the result of the pair before (set_initial("flow")), and the flow
        yielded is that total displacement on frame 0's grid (exclusive with cumulative, which composes it from the pairs).
        warm_start=True keeps the consecutive pairs and starts pair k from pair k-1's flow as it stands (steady motion).
        `initial` (see set_initial) starts pair 0."""
        if total and cumulative:
            raise ValueError("total=True solves frame 0 -> frame k+1 directly; cumulative=True composes it from the pairs: choose one")
        if total and warm_start:
            raise ValueError("total=True starts every pair from the one before already; warm_start belongs to consecutive pairs")
        first = previous = None
        k = 0
        if cumulative:
            self.trajectory_begin()
        try:
            for frame in frames:
                if previous is not None:
                    self.upload(first if total else previous, frame)
                    start = initial if k == 0 else ("flow" if (total or warm_start) else None)
                    self.compute_resident(silent=silent, initial=start, **kw)
                    flow = self.download()
                    disp = None
                    if cumulative:
                        self.trajectory_append()
                        disp = self.trajectory_download()
                    yield k, flow, disp
                    k += 1
                else:
                    first = frame
                previous = frame
        finally:
            if cumulative and self._h:
                self.trajectory_end()

    def destroy(self):
        if self._h:
            host().f3d_flow_destroy(self._h)
            self._h = C.c_void_p()


class PiecemealOpticalFlow:
    """OpticalFlowP: every volume stays in host memory, z-chunks stream through the device (no pre-blur, no median, like
    the reference's piecemeal driver).  F3D_P_BUDGET_MB bounds the device memory it uses."""

    def __init__(self):
        self._h = C.c_void_p()
        check(host().f3d_pflow_create(C.byref(self._h)), "f3d_pflow_create")
        self.device_seconds = 0.0

    def initialize(self, width, height, depth):
        if host().f3d_pflow_initialize(self._h, width, height, depth) != 0:
            raise F3dError("OpticalFlowP::Initialize failed: " + (hip().f3d_last_error() or b"").decode())
        self.dims = (width, height, depth)
        return True

    def compute(self, frame_0, frame_1, silent=True, **kw):
        f0, p0 = _f32(frame_0)
        f1, p1 = _f32(frame_1)
        w, h, d = self.dims
        if f0.shape != (d, h, w) or f1.shape != (d, h, w):
            raise ValueError(f"frames must be [z,y,x] = {(d, h, w)}")
        u, v, ww = (np.empty((d, h, w), np.float32) for _ in range(3))
        prm = make_params(**kw)
        secs = C.c_float()
        check(host().f3d_pflow_compute(self._h, p0, p1, w, h, d, C.byref(prm), int(silent), u.ctypes.data_as(_fp),
                                       v.ctypes.data_as(_fp), ww.ctypes.data_as(_fp), C.byref(secs)), "f3d_pflow_compute")
        self.device_seconds = secs.value
        return u, v, ww

    def operator_seconds(self):
        """wall seconds of the last compute per operator"""
        t = (C.c_double * 6)()
        check(host().f3d_pflow_operator_seconds(self._h, t), "f3d_pflow_operator_seconds")
        return dict(zip(("frames", "flow_resample", "registration", "solve", "add", "resident_levels"), t))

    def originals_on_device(self):
        """True when the resident levels of the last compute read the original frames from device copies"""
        y = C.c_int()
        check(host().f3d_pflow_originals_on_device(self._h, C.byref(y)), "f3d_pflow_originals_on_device")
        return bool(y.value)

    def set_full_pipeline(self, enabled):
        """also run the Gaussian pre-blur and the per-level median: OpticalFlowE's whole pipeline on host volumes"""
        check(host().f3d_pflow_set_full_pipeline(self._h, int(bool(enabled))), "f3d_pflow_set_full_pipeline")

    def set_resident(self, enabled):
        """coarse levels that fit the budget stay on the device (default) or every level goes through the host"""
        check(host().f3d_pflow_set_resident(self._h, int(bool(enabled))), "f3d_pflow_set_resident")

    def stats(self):
        """(solver residencies, levels cut into chunks, coarse levels run wholly on the device) of the last compute"""
        a, b, c = _sz(), _sz(), _sz()
        check(host().f3d_pflow_stats(self._h, C.byref(a), C.byref(b), C.byref(c)), "f3d_pflow_stats")
        return a.value, b.value, c.value

    def levels_registered_inside(self):
        """host levels of the last compute whose frame 1 was registered inside the solver's first residency"""
        a = _sz()
        check(host().f3d_pflow_levels_registered_inside(self._h, C.byref(a)), "f3d_pflow_levels_registered_inside")
        return a.value

    def levels_with_constants_on_device(self):
        """host levels of the last compute whose solver held the frames and u, v, w on the device for the whole level"""
        a = _sz()
        check(host().f3d_pflow_levels_with_constants_on_device(self._h, C.byref(a)), "f3d_pflow_levels_with_constants_on_device")
        return a.value

    def destroy(self):
        if self._h:
            host().f3d_pflow_destroy(self._h)
            self._h = C.c_void_p()


# ---- multi-GPU z-slab driver (OpticalFlowSlab) -----------------------------------------------------------------------

def plan_owned(depth, rank, n_ranks):
    lo, hi = C.c_int(), C.c_int()
    check(host().f3d_plan_owned(depth, rank, n_ranks, C.byref(lo), C.byref(hi)), "f3d_plan_owned")
    return lo.value, hi.value


def plan_exchange(depth, rank, n_ranks, need_lo, need_hi):
    """[(peer, (send_lo, send_hi), (recv_lo, recv_hi)), ...] in global planes."""
    cap = max(1, n_ranks)
    arr = [(C.c_int * cap)() for _ in range(5)]
    n = host().f3d_plan_exchange(depth, rank, n_ranks, need_lo, need_hi, *arr, cap)
    if n < 0:
        raise F3dError("f3d_plan_exchange failed")
    return [(arr[0][i], (arr[1][i], arr[2][i]), (arr[3][i], arr[4][i])) for i in range(n)]


def plan_resample_source(in_depth, out_depth, out_lo, out_hi):
    lo, hi = C.c_int(), C.c_int()
    check(host().f3d_plan_resample_source(in_depth, out_depth, out_lo, out_hi, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def comm_unique_id():
    buf = C.create_string_buffer(128)
    check(hip().f3d_comm_unique_id(buf), "f3d_comm_unique_id")
    return buf.raw


def comm_init(unique_id, rank, n_ranks, device=-1):
    check(hip().f3d_init(device), "f3d_init")
    buf = C.create_string_buffer(bytes(unique_id), 128)
    check(hip().f3d_comm_init(buf, rank, n_ranks), "f3d_comm_init")


def comm_destroy():
    hip().f3d_comm_destroy()


def comm_info():
    """what the transport says about itself: RCCL's own rank count / rank / device for the live communicator, bytes and
    exchanges this rank has handed to it"""
    be, n, r, dev = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    sent, ex = C.c_ulonglong(), C.c_ulonglong()
    check(hip().f3d_comm_info(C.byref(be), C.byref(n), C.byref(r), C.byref(dev), C.byref(sent), C.byref(ex)), "f3d_comm_info")
    return {"backend": {0: "none", 1: "rccl", 2: "shm"}.get(be.value, "?"), "ranks": n.value, "rank": r.value,
            "device": dev.value, "sent_bytes": sent.value, "exchanges": ex.value}


def comm_timing(enable):
    """HIP-event timing of the halo exchanges (f3d_comm_timing): on also clears the sums"""
    check(hip().f3d_comm_timing(1 if enable else 0), "f3d_comm_timing")


def comm_timing_read():
    """{class: {count, mean_us, min_us, max_us, mean_bytes_sent}} for the three classes of interval of include/f3d.h"""
    out = {}
    for cls, name in ((0, "blocking_exchange"), (1, "overlapped_exchange_incl_interior"), (2, "grouped_send_recv_alone")):
        us, n, mn, mx, by = C.c_double(), C.c_ulonglong(), C.c_double(), C.c_double(), C.c_ulonglong()
        check(hip().f3d_comm_timing_read(cls, C.byref(us), C.byref(n), C.byref(mn), C.byref(mx), C.byref(by)), "f3d_comm_timing_read")
        out[name] = {"count": n.value, "mean_us": round(us.value / n.value, 2) if n.value else None,
                     "min_us": round(mn.value, 2) if n.value else None, "max_us": round(mx.value, 2) if n.value else None,
                     "mean_bytes_sent": int(by.value / n.value) if n.value else None}
    return out


class SlabOpticalFlow:
    """OpticalFlowSlab: the same solve on n_ranks z-slabs.  local_ranks = [rank] with RCCL (call comm_init first), or
    list(range(n_ranks)) for the one-GPU rehearsal."""

    def __init__(self, n_ranks, local_ranks, halo_capacity=16):
        self._h = C.c_void_p()
        lr = (C.c_int * len(local_ranks))(*local_ranks)
        check(host().f3d_slabflow_create(C.byref(self._h), n_ranks, lr, len(local_ranks), halo_capacity), "f3d_slabflow_create")
        self.dims = None

    def initialize(self, width, height, depth):
        if host().f3d_slabflow_initialize(self._h, width, height, depth) != 0:
            raise F3dError("OpticalFlowSlab::Initialize failed: " + (hip().f3d_last_error() or b"").decode())
        self.dims = (width, height, depth)

    def compute(self, frame_0, frame_1, **kw):
        f0, p0 = _f32(frame_0)
        f1, p1 = _f32(frame_1)
        w, h, d = self.dims
        u, v, ww = (np.zeros((d, h, w), np.float32) for _ in range(3))
        prm = make_params(**kw)
        check(host().f3d_slabflow_compute(self._h, p0, p1, C.byref(prm), u.ctypes.data_as(_fp), v.ctypes.data_as(_fp),
                                          ww.ctypes.data_as(_fp)), "f3d_slabflow_compute")
        return u, v, ww

    def upload(self, frame_0, frame_1):
        f0, p0 = _f32(frame_0)
        f1, p1 = _f32(frame_1)
        check(host().f3d_slabflow_upload(self._h, p0, p1), "f3d_slabflow_upload")

    def compute_resident(self, **kw):
        prm = make_params(**kw)
        secs = C.c_float()
        check(host().f3d_slabflow_compute_resident(self._h, C.byref(prm), C.byref(secs)), "f3d_slabflow_compute_resident")
        return secs.value

    def download(self):
        w, h, d = self.dims
        u, v, ww = (np.zeros((d, h, w), np.float32) for _ in range(3))
        check(host().f3d_slabflow_download(self._h, u.ctypes.data_as(_fp), v.ctypes.data_as(_fp), ww.ctypes.data_as(_fp)))
        return u, v, ww

    def overlapped_iterations(self):
        n = _sz()
        check(host().f3d_slabflow_overlapped_iterations(self._h, C.byref(n)))
        return n.value

    def stage_exchanges(self):
        """exchanges of the last compute made after a solver stage (F3D_SLAB_EXCHANGE=stage)"""
        n = _sz()
        check(host().f3d_slabflow_stage_exchanges(self._h, C.byref(n)))
        return n.value

    def set_exchange_per_stage(self, per_stage):
        """exchange order of the solves that follow: False = once per outer iteration (default), True = after every solver stage"""
        check(host().f3d_slabflow_set_exchange_per_stage(self._h, 1 if per_stage else 0), "f3d_slabflow_set_exchange_per_stage")

    def gathered_warps(self):
        """pyramid levels of the last compute whose warp needed frame 1 gathered beyond the halo room"""
        n = _sz()
        check(host().f3d_slabflow_gathered_warps(self._h, C.byref(n)))
        return n.value

    def batched_exchanges(self):
        """groups of several outer iterations the last compute ran between two exchanges"""
        n = _sz()
        check(host().f3d_slabflow_batched_exchanges(self._h, C.byref(n)))
        return n.value

    def destroy(self):
        if self._h:
            host().f3d_slabflow_destroy(self._h)
            self._h = C.c_void_p()
