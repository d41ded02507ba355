#!/bin/bash
# Build a variant of the library with extra -D flags or sources into tools/_diag/libvariant_NAME.so (for A/B timing with tools/ab_*.py)
# usage: tools/build_variant.sh NAME [-DFLAG ...] [EXTRA.hip ...]
set -e
cd "$(dirname "$0")/.."
name=$1; shift
python sup-nerf_amd/build.py --out tools/_diag/libvariant_${name}.so "$@"
