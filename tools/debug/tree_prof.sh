#!/bin/bash
# tuning: a variant of the library whose deflate_kernels.hip has phase stamps (-DCCT_TREE_PROF, a flag of its own: csrc/tuning.h),
# built next to the release library (tools/ab_build.sh, after a finished `make` in csrc) and loaded through CCT_HIP_LIB;
# prints the phase times of one tree workgroup
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
$ROOT/tools/ab_build.sh tree_prof deflate_kernels.hip -DCCT_TREE_PROF
cd $ROOT && CCT_HIP_LIB=$ROOT/build_ab/libcompact_hip_tree_prof.so timeout -k 10 200 python tools/prof_codec.py --reps 2 --what enc 2>&1 | grep -E "tree prof|^enc" | tail -4
