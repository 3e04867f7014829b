"""The flow update inside the solve, without a GPU: libf3d_host.so built against a host-memory stand-in of the device library (the C
ABI of include/f3d.h on host memory, the oracle's kernels as the compute; see tests/test_host_on_cpu_backend.py for the manner), once
WITH f3d_solve_sweep_add (tests/cpu_device_sweep_add: the stand-in of tests/cpu_device plus that entry) and once WITHOUT it
(tests/cpu_device as it is: the host library links the entry weakly).

 * with the entry the resident driver asks the Solve operator for `flow += increments` in the level's last launch and skips its add
   where the operator says it did; a whole ComputeFlow must still be the oracle's, bit for bit -- with an odd inner count (update
   inside the solve), an even one (the add runs as before) and a single sweep per outer iteration;
 * the operator itself, through the bag: asked and able (5 sweeps), asked and unable (4 sweeps), and not asked;
 * without the entry the host library loads, the operator reports the update not done, and the driver's results are the oracle's."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")

CASE = textwrap.dedent('''
    import ctypes as C, importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    from oracle import oracle as orc
    same = lambda a, b: a.shape == b.shape and bool(np.all(a == b)) and not np.isnan(a).any()
    what = sys.argv[1]
    have = os.environ["F3D_TEST_HAS_ENTRY"] == "1"
    assert hasattr(pkg.hip(), "f3d_solve_sweep_add") == have
    if what == "driver":
        W, H, D = 26, 22, 20
        f0, f1 = pkg.synth_pair(W, H, D)
        for inner in (5, 4, 1):
            kw = dict(warp_levels_count=5, outer_iterations_count=3, inner_iterations_count=inner)
            (eu, ev, ew), _ = orc.compute_flow(f0, f1, **kw)
            flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
            got = flow.compute(f0, f1, silent=True, **kw); flow.destroy()
            assert all(same(g, e) for g, e in zip(got, (eu, ev, ew))), inner
    elif what == "operator":
        op = pkg.Operation("solve")
        rng = np.random.default_rng(3)
        cdims, dims, outer = (128, 24, 12), (70, 21, 9), 3
        cw, ch, cd = cdims; w, h, d = dims
        cont = pkg.Containers(*cdims)
        def put(lo, hi):
            c = np.zeros((cd, ch, cw), np.float32)
            c[:d, :h, :w] = rng.uniform(lo, hi, size=(d, h, w)).astype(np.float32)
            return c, cont.new(c)
        hosts, ptrs = zip(*[put(*r) for r in [(0, 255), (0, 255), (-2, 2), (-2, 2), (-2, 2)]])
        names = ["dev_flow_du", "dev_flow_dv", "dev_flow_dw", "dev_phi", "dev_ksi", "dev_temp_du", "dev_temp_dv", "dev_temp_dw"]
        extra = {n: cont.new() for n in names}
        assert op.initialize(cont)
        sp = (1.5, 1.2, 2.0)
        for inner, ask, done in ((5, True, have), (4, True, False), (5, False, False)):
            more = dict(flow_update=False) if ask else {}
            vals = op.execute(dev_frame_0=ptrs[0], dev_frame_1=ptrs[1], dev_flow_u=ptrs[2], dev_flow_v=ptrs[3], dev_flow_w=ptrs[4],
                              outer_iterations_count=outer, inner_iterations_count=inner, equation_alpha=7.5, equation_smoothness=0.001,
                              equation_data=0.001, hx=sp[0], hy=sp[1], hz=sp[2], data_size=dims, **extra, **more)
            pkg.sync()
            assert vals.get("flow_update", False) is done, (inner, ask, vals.get("flow_update"))
            du = np.zeros_like(hosts[0]); dv, dw = du.copy(), du.copy()
            for _ in range(outer):
                phi, ksi = orc.phi_ksi(*hosts, du, dv, dw, dims, sp, 0.001, 0.001)
                for _ in range(inner):
                    du, dv, dw = orc.solve_sweep(*hosts, du, dv, dw, phi, ksi, dims, sp, 7.5)
            expect = [du, dv, dw]
            if done:
                expect = []
                for flow_c, inc in zip(hosts[2:], (du, dv, dw)):
                    e = flow_c.copy(); orc.add(e, inc, dims); expect.append(e)
            for key, e in zip(("dev_flow_du", "dev_flow_dv", "dev_flow_dw", "dev_phi", "dev_ksi"), expect + [phi, ksi]):
                g = cont.download(vals[key], cdims)
                assert same(g[:d, :h, :w], e[:d, :h, :w]), (inner, ask, key)
            for c, host in zip("uvw", hosts[2:]):   # the flow itself is not written, and the six containers are still the three pairs
                assert same(cont.download(ptrs[2 + "uvw".index(c)], cdims), host), c
                assert {vals[f"dev_flow_d{c}"], vals[f"dev_temp_d{c}"]} == {extra[f"dev_flow_d{c}"], extra[f"dev_temp_d{c}"]}
            extra = {n: vals[n] for n in names}
        op.destroy()
        cont.free()
    pkg.shutdown()
    print("ok", what)
''')


def run_case(what, libdir, has_entry):
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, F3D_TEST_HAS_ENTRY="1" if has_entry else "0", OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE, what], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and f"ok {what}" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.fixture(scope="module")
def with_entry(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpu_device_sweep_add"))
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpu_device_sweep_add"), "OUT=" + out, "-j4"], check=True, stdout=subprocess.DEVNULL)
    return out


@pytest.fixture(scope="module")
def without_entry():
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(CPU, "_build", "plain")


def test_resident_driver_with_the_flow_update_inside_the_solve_equals_the_oracle(with_entry):
    run_case("driver", with_entry, True)


def test_solve_operator_reports_the_flow_update_through_the_bag(with_entry):
    run_case("operator", with_entry, True)


def test_host_library_without_the_entry_still_solves_and_reports_the_update_not_done(without_entry):
    run_case("driver", without_entry, False)
    run_case("operator", without_entry, False)
