"""Build-time checks of the 5^3 median kernel that shares sorted columns and keeps the merged plane pairs in LDS
(k_median_share): its generated networks are what the checked generator writes, and the gfx950 assembly that the Makefile's flags
for f3d_median.hip give has the resources the launcher counts on.  Runs on the CPU: hipcc only cross-compiles."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generated_share_networks_are_current():
    """csrc/f3d_median_nets_share.h is what tools/gen_median_nets.py main_share() writes (every network is checked against
    sorted() on random inputs with ties before it is emitted): a 5-sort of 9 exchanges and the merge of five sorted columns."""
    gen = load_tool("gen_median_nets")
    text, counts = gen.main_share()
    assert counts == [18, 202]
    with open(gen.HEADER_SHARE) as f:
        assert f.read() == text


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_share_kernel_resources_and_no_canonicalisation():
    """No `v_max_f32 vN, vN, vN` in front of the min/max networks (the kernel reads in-box voxels only; the file is built with
    NaN-free min/max), no scratch, at most 256 VGPRs (two waves per SIMD) and LDS for two workgroups per CU."""
    report = load_tool("median_isa").report()
    assert "k_median_share" in report, sorted(report)
    k = report["k_median_share"]
    print(k)
    assert k["canonicalise"] == 0
    assert k["scratch"] == 0
    assert k["vgprs"] <= 256 and k["waves_per_simd"] >= 2
    assert k["lds"] <= 80 * 1024
    # the networks are there: four unrolled steps of two plane lists, one merge25, the candidates and two selection chains
    assert k["minmax"] > 4000
    for name, other in report.items():
        assert other["scratch"] == 0, name
