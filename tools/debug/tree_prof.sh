#!/bin/bash
# tuning: a variant of the library whose deflate_kernels.hip has phase stamps and a placement probe (-DCCT_TREE_PROF, a flag
# of its own: csrc/tuning.h), built next to the release library (tools/ab_build.sh, after a finished `make` in csrc) and
# loaded through CCT_HIP_LIB; prints the phase times of one tree wave, then where and when every tree wave of a 256-payload
# call ran (tools/debug/tree_placement.py: waves per CU and SIMD, start spread, wave life against co-resident waves, clock).
# The second program starts only if the first one ended well.
#   tools/debug/tree_prof.sh [tree_waves: 0 automatic (default), 1 or 16]
set -e
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
LIB=$ROOT/build_ab/libcompact_hip_tree_prof.so
$ROOT/tools/ab_build.sh tree_prof deflate_kernels.hip -DCCT_TREE_PROF
cd $ROOT
CCT_HIP_LIB=$LIB timeout -k 10 200 python tools/prof_codec.py --reps 2 --what enc 2>&1 | grep -E "tree prof|^enc" | tail -4 &&
CCT_HIP_LIB=$LIB timeout -k 10 200 python tools/debug/tree_placement.py --slices 256 --tree-waves ${1:-0} 2>&1 | grep -v "tree prof"
