"""The paired reductions of the axis-per-lane solve kernel (csrc/vigo_solver.hip: pair_tree32, pack_xy) on a 64-lane model
of the wave, no GPU: tests/axis_pair_tree_check.cpp.

In the axis layout the xor-32 exchange of a dot product comes before the 32-lane tree, so group_sum<32, K> runs the same
tree on the same operands in both halves of the wave.  pair_tree32 gives the lower half one sum and the upper half
another.  The model runs both over random packed inputs (ordinary values, any bit pattern, -0, infinities, NaN with
payloads, denormals, and two sums 800 binades apart) and demands

  * both totals of the pair tree with the BITS of the two single trees, in every lane;
  * no read of a lane of the other half in any of the five tree levels (every read of the model is recorded);
  * pack_xy of two per-lane products with the bits of the two dot_xy it replaces, each in the half that carries it.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("axis_pair_tree") / "axis_pair_tree_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-ffp-contract=off",
                    os.path.join(HERE, "axis_pair_tree_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}


def test_pair_tree_has_the_bits_of_two_single_trees(figures):
    assert figures["inputs"] >= 3_000_000, "a few million packed inputs"
    assert figures["special_inputs"] >= figures["inputs"] // 50, "zeros, infinities, NaN and denormals are among them"
    assert figures["tree_diffs"] == 0


def test_no_half_reads_the_other_before_the_last_exchange(figures):
    assert figures["cross_reads"] == 0


def test_pack_xy_has_the_bits_of_two_dot_xy(figures):
    assert figures["dot_diffs"] == 0
