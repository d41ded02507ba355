#!/bin/bash
# Diagnostic build of the library with in-kernel s_memtime timelines (-DSNR_STAMPS; the stamps overwrite the sigma / d_t outputs).
# usage: tools/build_diag.sh NAME [-DFLAG ...]   ->  tools/_diag/libsupnerf_stamps_NAME.so
set -e
cd "$(dirname "$0")/.."
name=$1; shift
python sup-nerf_amd/build.py --out tools/_diag/libsupnerf_stamps_${name}.so -DSNR_STAMPS "$@"
