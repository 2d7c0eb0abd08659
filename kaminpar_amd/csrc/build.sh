#!/bin/bash
# Builds kaminpar_amd/libkaminpar_lp.so (gfx950). Run from csrc/.
# The units compile in parallel, at most min(16, nproc) at a time; a unit that
# fails to compile fails the script.
set -e
cd "$(dirname "$0")"

# the longest compile first, so it does not start late
HIP_UNITS="lp_hip jet_hip extract_hip edges_hip sparsify_hip vcycle_hip resident_hip"
CPP_UNITS="graph_gen partition_host pipeline_host"

compile() {
  case "$1" in
    *.hip) hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c "$1" -o "${1%.hip}.o" ;;
    pipeline_host.cpp) g++ -O3 -fPIC -std=c++17 -Wall -c "$1" -o "${1%.cpp}.o" ;;
    *.cpp) g++ -O3 -fPIC -std=c++17 -fopenmp -Wall -c "$1" -o "${1%.cpp}.o" ;;
  esac || { echo "build.sh: compiling $1 FAILED" >&2; echo "$1" >> "$FAILED_LIST"; return 1; }
}
FAILED_LIST=$(mktemp)
trap 'rm -f "$FAILED_LIST"' EXIT
export -f compile
export FAILED_LIST

jobs=$(nproc)
if [ "$jobs" -gt 16 ]; then
  jobs=16
fi
sources=""
objects=""
for u in $HIP_UNITS; do sources="$sources $u.hip"; objects="$objects $u.o"; done
for u in $CPP_UNITS; do sources="$sources $u.cpp"; objects="$objects $u.o"; done
if ! printf '%s\n' $sources | xargs -P "$jobs" -n 1 bash -c 'compile "$0"'; then
  echo "build.sh: not linking; failed to compile: $(tr '\n' ' ' < "$FAILED_LIST")" >&2
  exit 1
fi
hipcc -shared -fPIC $objects -o ../libkaminpar_lp.so -lgomp -L/opt/rocm/lib -lrccl
echo "built kaminpar_amd/libkaminpar_lp.so"
