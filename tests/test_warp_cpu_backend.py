"""f3d_warp on the host-memory stand-in of the device library (tests/cpu_device: the C ABI of include/f3d.h on host memory, the oracle's
kernels as the compute; see tests/test_host_on_cpu_backend.py for the manner), without a GPU.

 * The contract of include/f3d.h, which is the reference operator's: frame_0 may be the output, frame_1 may not.
   tests/test_gpu_stream_routes.py pins the same on the device.
 * The slab windows of tests/test_gpu_stream_routes.py, run by that file's own check: every one of the six volumes is addressed by
   z - z_base, and the windowed result is the whole-volume one cut to the window."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")

CASE = textwrap.dedent('''
    import importlib, os, sys
    sys.path[:0] = [os.environ["F3D_ROOT"], os.path.join(os.environ["F3D_ROOT"], "tests")]
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    from oracle import oracle as orc
    import test_gpu_stream_routes as T
    T.test_warp_may_write_frame_0_and_never_frame_1(pkg, orc)
    for h in T.SPACINGS:
        for window in [None] + T.WARP_WINDOWS:
            T.test_warp_on_slab_windows(pkg, orc, window, h)
    pkg.shutdown()
    print("ok warp")
''')


def test_warp_contract_and_slab_windows_on_the_stand_in():
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=os.path.join(CPU, "_build", "plain"), OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok warp" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
