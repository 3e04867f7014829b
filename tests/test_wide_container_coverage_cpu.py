"""No entry point that launches a kernel over a container's box arrives without a wide-container case: every declaration of
include/f3d.h that takes an f3d_devptr (or a const f3d_devptr*) is named in tests/test_gpu_wide_container_offsets.py, in
tests/test_gpu_wide_container_analysis.py or in the helper both are built on (tests/wide_container.py, which holds the solver
family's launches), or stands in EXCLUDED with the reason why it launches no kernel over a box.  No GPU is needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("test_gpu_wide_container_offsets.py", "test_gpu_wide_container_analysis.py", "wide_container.py")

# name -> why it launches no kernel over a container's box (one line each)
EXCLUDED = {
    "f3d_alloc_pitched": "allocation: hipMalloc, no kernel",
    "f3d_free": "hipFree, no kernel",
    "f3d_copy_planes_h2d": "host to device copy: hipMemcpy2DAsync / hipMemcpy3DAsync, 64-bit offsets formed on the host",
    "f3d_copy_planes_d2h": "device to host copy: hipMemcpy2DAsync / hipMemcpy3DAsync, 64-bit offsets formed on the host",
    "f3d_copy_planes_h2d_on": "f3d_copy_planes_h2d on a queue of the caller's",
    "f3d_copy_planes_d2h_on": "f3d_copy_planes_d2h on a queue of the caller's",
    "f3d_copy_rect_d2d": "device to device copy: one hipMemcpy3DAsync",
    "f3d_copy_d2d": "device to device copy: one hipMemcpyAsync of a byte count",
    "f3d_comm_sendrecv": "RCCL send / receive of a dense staging buffer: no container geometry",
    "f3d_comm_sendrecv_begin": "RCCL send / receive of a dense staging buffer: no container geometry",
}


def declarations(text):
    """[(name, arguments)] of every function include/f3d.h declares"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.findall(r"\b(?:int|void|const char\s*\*)\s+(f3d_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)


def device_entries(text):
    return [name for name, arguments in declarations(text) if re.search(r"\bf3d_devptr\b", arguments)]


def named(name, sources):
    return any(re.search(r"\b%s\b" % re.escape(name), s) for s in sources)


def uncovered(entries, sources, excluded):
    return [e for e in entries if e not in excluded and not named(e, sources)]


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_every_entry_that_takes_a_container_has_a_wide_container_case_or_a_reason():
    entries = device_entries(read("include", "f3d.h"))
    assert len(entries) == len(set(entries)) >= 80 and "f3d_label_overlap" in entries and "f3d_median_n" in entries
    sources = [read("tests", m) for m in MODULES]
    assert uncovered(entries, sources, EXCLUDED) == []
    stale = [e for e in EXCLUDED if e not in entries]
    assert stale == [], f"EXCLUDED names what include/f3d.h no longer declares with a device pointer: {stale}"
    both = [e for e in EXCLUDED if named(e, sources[:2])]
    assert both == [], f"excluded and covered: {both}"
    assert all(reason and "\n" not in reason for reason in EXCLUDED.values())


def test_the_check_notices_a_missing_case_and_a_new_entry():
    header = read("include", "f3d.h")
    entries = device_entries(header)
    sources = [read("tests", m) for m in MODULES]
    without = [s.replace("f3d_carry_field", "f3d_c_f") for s in sources]
    assert uncovered(entries, without, EXCLUDED) == ["f3d_carry_field"]
    more = header + "\nint f3d_new_entry(f3d_devptr volume, size_t width,\n    size_t height, size_t depth);\nint f3d_new_list(const f3d_devptr* volumes);\n"
    assert uncovered(device_entries(more), sources, EXCLUDED) == ["f3d_new_entry", "f3d_new_list"]
    assert "f3d_set_conv_taps" not in entries and "f3d_stream_sync" not in entries      # no device pointer: not this check's business


def test_the_analysis_module_names_27_entries_each_once_and_marches_32_planes_in_geometry_b():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_wide_container_analysis as analysis
    names = [e for case in analysis.CASES for e in case.entries]
    assert len(names) == len(set(names)) == 27 and set(names) <= set(device_entries(read("include", "f3d.h")))
    csrc = os.path.join(ROOT, "cuda-flow3d_amd", "csrc")
    marching = [f for f in sorted(os.listdir(csrc)) if "constexpr int kZ = 32;" in read("cuda-flow3d_amd", "csrc", f)]
    assert marching == ["f3d_components_passes.h", "f3d_correlation.hip", "f3d_histogram.hip", "f3d_label_contacts.hip", "f3d_label_field.hip",
                        "f3d_label_motion.hip", "f3d_label_overlap.hip", "f3d_label_shape.hip", "f3d_motion.hip", "f3d_strain_grad.h",
                        "f3d_validate.hip", "f3d_window_strain.hip"]
    # the others gather or map voxel by voxel: one thread per voxel, no march (f3d_gather.h, f3d_trajectory.hip, f3d_inverse.hip,
    # f3d_initial_flow.hip); they take the 256 MiB planes
    assert [c.__name__ for c in analysis.CASES if c.geometry == "A"] == ["ComposeFlow", "InitialFlow", "InvertDisplacement", "CarryField"]
    # the host blocks of a case: the image of a view in geometry B
    w, h, d = analysis.W + analysis.wc.MX, analysis.H + analysis.wc.MY, analysis.GEOMETRY["B"][1]
    assert 250_000 < w * h * d * 4 <= analysis.wc.HOST_BLOCK_LIMIT
