#!/bin/bash
# builds the attention harness into tests/microbench/bin/ (git-ignored).  The kernels have one code path: a binary per VARIANT name
# is only useful to time two source trees side by side
set -e
cd "$(dirname "$0")"
mkdir -p bin && rm -f bin/mb_*
build() { # name, flags...
  local name=$1; shift
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -fno-honor-nans -mno-amdgpu-ieee -fno-slp-vectorize -I ../../include -DVARIANT="\"$name\"" "$@" attn_microbench.hip -o bin/mb_$name &
}
build base
wait %1      # the compiler's exit status (set -e)
ls bin
