"""Where a row wave of the weights-first launch reads the x neighbours of its lanes (csrc/f3d_pair8_plan.h: pair8_x_neighbours and
pair8_x_neighbour_offset, the functions the kernel calls), without a GPU: tests/pair8_x_neighbours_main.cpp walks every lane of every
tile column for the widths 1 .. 200 over a model of a ring slot and checks which column of the volume each read names -- x - 1 and
x + 1, the mirrored one at x = 0 and x = W - 1, the halo piece at lanes 0 and 63 only and never where it was fetched from inside the
row -- with every address inside the slot.  The program is built once with AddressSanitizer and UBSan and run on its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-flow3d_amd", "csrc")


def test_every_lane_names_its_neighbours_under_the_sanitizers(tmp_path):
    exe = tmp_path / "pair8_x_neighbours"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "pair8_x_neighbours_main.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-2000:], run.stderr[-3000:])
