#!/bin/bash
# dev: an alternative build of the solve kernels for A/B timing (tools/exp_solver.py, VIGO_EXP_LIB=trajectory_planner_amd/lib/exp/libvigo_NAME.so)
#   bash tools/build_variant.sh NAME "-DMY_SWITCH=1 ..."
# The Makefile's `variant` target: the shipped flags plus these, linked with the shipped objects of the other files,
# under a vigo_build_id() of its own.
set -e
make -C "$(dirname "$0")/../trajectory_planner_amd/csrc" -j4 variant VLIB=../lib/exp/libvigo_$1.so EXTRA="$2"
echo built trajectory_planner_amd/lib/exp/libvigo_$1.so
