#!/bin/bash
# Host-side sources (no HIP) under AddressSanitizer + UBSan: the .bt reader on every map given on the command
# line, 300 random min-snap QPs (with and without corridors, feasible and infeasible), B-spline fits/evaluations, A* searches, pwlTraj plans, soft-constraint QPs, the ESDF build's host twin on hostile sizes, the seed-path stage's rules and serial driver (csrc/vigo_seed_core.hpp) on min-snap polynomials; then, as a second programme, the facade's own steps of that stage.
#   bash tools/sanitize_host.sh /root/reference/map/*.bt
# (GPU sanitizers are not available on the pool; the device code is covered by the parity tests and the fuzz sweep.)
set -e
cd "$(dirname "$0")/../trajectory_planner_amd/host"
g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -o /tmp/vigo_san_test \
    ../../tools/sanitize_host_main.cpp src/octomapBt.cpp src/polyTrajSolver.cpp src/bspline.cpp src/astarOcc.cpp src/piecewiseLinearTraj.cpp
/tmp/vigo_san_test "$@"
# the facade's own steps of the seed-path stage (bsplineTraj's sources need the HIP headers and link libvigo_hip.so, built
# first by `make -C trajectory_planner_amd/csrc`; the steps themselves use neither, and no GPU)
ROCM=${ROCM:-/opt/rocm}
g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -Iinclude -I$ROCM/include -pthread \
    -o /tmp/vigo_san_seed_facade ../../tools/sanitize_seed_facade_main.cpp src/bsplineTraj.cpp src/bsplineTrajSeed.cpp src/bsplineTrajBatch.cpp src/polyTrajOccMap.cpp src/polyTrajSolver.cpp \
    src/bspline.cpp src/astarOcc.cpp src/piecewiseLinearTraj.cpp src/mapAdapter.cpp -L../lib -lvigo_hip -L$ROCM/lib -lamdhip64 \
    -Wl,-rpath,"$PWD/../lib" -Wl,-rpath,$ROCM/lib
/tmp/vigo_san_seed_facade
# the plan's last stage on the host (vigo_traj_finish_host: csrc/vigo_finish_core.hpp through the host side of
# csrc/vigo_finish.hip, whose sources are HIP: hipcc compiles them, the sanitizers instrument the host code only; no GPU)
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
$HIPCC --offload-arch=gfx950 -std=c++17 -g -O1 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
    -I../../include -o /tmp/vigo_san_finish ../../tools/sanitize_finish_main.cpp -x hip ../csrc/vigo_finish.hip
/tmp/vigo_san_finish
