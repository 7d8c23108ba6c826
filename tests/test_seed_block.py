"""-m "not gpu": the two blocks the facade's seed stage moves per group (host/src/seedBlock.h: every input of
vigo_seed_paths in one upload, every output in one download) on host memory.  tests/seed_block_check.cpp is a program of
its own: built here with the address and undefined-behaviour sanitizers, it carves both blocks for T in {1, 2, 3}, S in
{0, 1, 5}, deg in {0, 7, 15}, cap in {0, 1, 128} out of allocations of exactly the size the layout asks for and checks
alignment, order, tiling, the extents of include/vigo.h and a pattern written through one view and read through the other
(see its header)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "trajectory_planner_amd", "host", "src")


def test_seed_blocks_tile_align_and_read_back(tmp_path):
    exe = str(tmp_path / "seed_block_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I", SRC, os.path.join(HERE, "seed_block_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "seed_block_check: 162 blocks carved, written and read back" in r.stdout
