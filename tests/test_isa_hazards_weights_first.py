"""Build-time check of k_wpair8 -- the weights-first launch and the two sweeps with the flow update (csrc/f3d_solve_pair8.h) --, on the
CPU: hipcc cross-compiles f3d_solve.hip to assembly and tools/isa_hazards.py walks the loader wave of every instantiation."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = {(mode, ty, folds) for mode in (2, 3) for ty in (4, 8, 12) for folds in (0, 1)}


def load_tool():
    spec = importlib.util.spec_from_file_location("isa_hazards", os.path.join(ROOT, "tools", "isa_hazards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pieces_per_plane_of_the_weights_first_rings():
    """6 stencilled + 4 centre-only arrays; the centre ring holds the core rows alone"""
    tool = load_tool()
    assert [tool.wpair8_per_plane(2, ty) for ty in (4, 8, 12)] == [6 * 2 + 2, 6 * 3 + 3, 6 * 4 + 3]
    assert [tool.wpair8_centre_per_plane(2, ty) for ty in (4, 8, 12)] == [4, 8, 12]
    for ty in (4, 8, 12):     # two sweeps + flow: the rings of the frame-derivative two-sweep launch
        assert tool.wpair8_per_plane(3, ty) == tool.pair8_per_plane(ty, True)
        assert tool.wpair8_centre_per_plane(3, ty) == tool.pair8_centre_per_plane(ty, True)
        assert tool.wpair8_per_plane(2, ty) <= 63


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_wpair8_loader_waits_resources_and_a_mutant(tmp_path):
    """Every shipped instantiation: no scratch, the counted wait equals the pieces per plane computed in the tool from the tile shape,
    one or two planes between a barrier and that wait, 12-row builds at no more than 128 VGPRs (four waves per SIMD), LDS within the
    160 KB of a CU.  Then a build whose counted wait is one short must fail."""
    tool = load_tool()
    asm = tool.compile_to_asm()
    report, resources = tool.run_wpair8(asm)
    assert {tool.wpair8_params(name) for name in report} == SHIPPED, list(report)
    assert set(resources) == set(report)
    for name, bad in report.items():
        assert not bad, f"{name}: {bad[:5]}"
    for name, r in resources.items():
        mode, ty, folds = tool.wpair8_params(name)
        print(f"k_wpair8<{mode}, {ty}, {folds}>: {r['vgprs']} VGPRs, {r['lds']} B LDS, {r['scratch']} B scratch")
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        assert r["lds"] <= tool.LDS_LIMIT, f"{name}: {r['lds']} bytes of LDS"
        if ty == 12:
            assert r["vgprs"] <= 128, f"{name}: {r['vgprs']} VGPRs"
    # the existing kernels keep their names out of this one's: the stamp of the counter record and the fixed list of k_pair8 builds
    for name in report:
        assert not any(key in name for key in ("k_pair8", "k_tri", "k_sweep6", "k_sweep7", "k_phiksi6"))

    # the mutant: the same sources with the steady-state wait one short
    src_dir = os.path.join(ROOT, "cuda-flow3d_amd", "csrc")
    for f in os.listdir(src_dir):
        shutil.copy(os.path.join(src_dir, f), tmp_path / f)
    header = tmp_path / "f3d_solve_pair8.h"
    text = header.read_text()
    assert text.count('"n"(L::kPerPlane)') == 1
    header.write_text(text.replace('"n"(L::kPerPlane)', '"n"(L::kPerPlane - 1)'))
    flags = [f if not f.startswith("-I" + src_dir) else "-I" + str(tmp_path) for f in tool.FLAGS]
    out = tmp_path / "mutant.s"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + [str(tmp_path / "f3d_solve.hip"), "-o", str(out)],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    mutant, _ = tool.run_wpair8(str(out))
    assert mutant and all(any(v[0] == "P3" for v in bad) for bad in mutant.values()), "a wrong wait count went unnoticed"
