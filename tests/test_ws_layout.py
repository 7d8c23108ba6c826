"""-m "not gpu": the workspace layouts of the C-ABI layer (csrc/vigo_ws_layout.hpp) on host memory.  tests/ws_layout_check.cpp
is a program of its own: built here with the address and undefined-behaviour sanitizers, it carves every layout out of
an allocation of exactly the size the layout asks for, writes every array over the extent the kernels index, and checks
alignment, disjointness and the byte count (see its header)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")


def test_every_layout_fits_its_own_size_aligned_and_disjoint(tmp_path):
    exe = str(tmp_path / "ws_layout_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I", CSRC, os.path.join(HERE, "ws_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "layouts carved and written" in r.stdout
