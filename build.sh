#!/bin/bash
# Build libdvsg_amd.so (gfx950 only) in-tree.  Usage: ./build.sh [extra hipcc flags]
# DVSG_BUILD_OUT and DVSG_BUILD_OBJ name another library and object directory (tools/build_stamps.sh).
set -euo pipefail
cd "$(dirname "$0")"
SRC=coupe/dvsg_amd/csrc
OUT=${DVSG_BUILD_OUT:-coupe/dvsg_amd/libdvsg_amd.so}
OBJ=${DVSG_BUILD_OBJ:-build/obj}
mkdir -p "$OBJ" "$(dirname "$OUT")"
COMMON="-O3 --offload-arch=gfx950 -fPIC -std=c++17 -Wall -Wno-unused-function $*"
# The one list of sources: "file | extra flags".  The compile loop and the link line are both made from it.
# -ffp-contract=off: separately rounded ops --
#   warps, losses, crop and the root conv's fused scale_RGB: float32 ops like the reference graph
#   scene cuts: the luma's float32 ops rounded one by one, like its NumPy restatement
#   frame formats: float64 ops like NumPy / OpenCV on the host
#   NV12 frames: the integer conversion, frames.hip's float64 ops and the warps' float32 ops
SOURCES=(
  "warp_kernels.hip      | -ffp-contract=off"
  "loss_kernels.hip      | -ffp-contract=off"
  "crop_kernels.hip      | -ffp-contract=off"
  "scene_kernels.hip     | -ffp-contract=off"
  "shake_kernels.hip     |"
  "conv1_f16.hip         | -ffp-contract=off"
  "conv1_f32.hip         | -ffp-contract=off"
  "conv1_x3.hip          | -ffp-contract=off"
  "root_pool.hip         | -ffp-contract=off"
  "conv1.hip             | -ffp-contract=off"
  "frames.hip            | -ffp-contract=off"
  "nv12.hip              | -ffp-contract=off"
  "conv_gemm.hip         |"
  "conv_gemm_x3.hip      |"
  "conv_fused.hip        |"
  "conv_fused_x3.hip     |"
  "conv_gemm_wide16.hip  |"
  "head.hip              |"
  "locnet.hip            |"
  "views.cpp             | -x hip"
  "api_common.cpp        | -x hip"
)
JOBS=16   # compiles at a time
objs=()
running=0
for entry in "${SOURCES[@]}"; do
  file=${entry%%|*}
  file=${file// /}
  flags=${entry#*|}
  obj=$OBJ/${file%.*}.o
  objs+=("$obj")
  if [ "$running" -ge "$JOBS" ]; then
    wait -n
    running=$((running - 1))
  fi
  hipcc $COMMON $flags -c "$SRC/$file" -o "$obj" &
  running=$((running + 1))
done
while [ "$running" -gt 0 ]; do
  wait -n
  running=$((running - 1))
done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" "${objs[@]}"
echo "built $OUT"
