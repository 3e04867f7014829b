"""The launches of tests/test_gpu_wide_container_offsets.py whose chunk length only F3D_ZCHUNK sets, which is read once per process:
one fresh interpreter with F3D_ZCHUNK=7 and F3D_PAIR8=0 (set by the parent), its own 5 GiB allocation.
argv: inputs.npz results.npz -- the parent wrote the inputs (boxes and the oracle's weights) and compares the boxes written here."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_container as wc

assert os.environ.get("F3D_ZCHUNK") == "7" and os.environ.get("F3D_PAIR8") == "0"
f3d = importlib.import_module("cuda-flow3d_amd")
given = np.load(sys.argv[1])
rig = wc.Wide(f3d)
results = {}
try:
    for tag, dims, window, zones in wc.CHILD_CASES:
        arrays = [given[f"{tag}/{i}"] for i in range(10)]
        case = wc.SolverCase(rig, arrays[:8], arrays[8:], dims, window)
        for name, tri_ty in wc.CHILD_LAUNCHES:
            if tri_ty:
                os.environ["F3D_TRI_TY"] = str(tri_ty)
            else:
                os.environ.pop("F3D_TRI_TY", None)
            res = case.run(name, zones=zones if name == "f3d_phi_ksi_zones" else None)
            for i, box in enumerate(res["boxes"]):
                results[f"{tag}/{name}/{tri_ty}/{i}"] = box
finally:
    rig.close()
np.savez(sys.argv[2], **results)
print("ok")
