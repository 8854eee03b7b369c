#!/bin/bash
# Diagnostic build of the library with -DDVSG_STAMPS (per-workgroup s_memtime stamps) into build/lib_stamps.so: tools/build_stamps.sh -DDVSG_STAMPS
# build.sh's own list of sources, another library and object directory; the flags are the caller's.
set -euo pipefail
cd "$(dirname "$0")/.."
DVSG_BUILD_OUT=build/lib_stamps.so DVSG_BUILD_OBJ=build/obj_stamps exec ./build.sh "$@"
