#!/bin/bash
# Development aid: builds the kernel library with extra -D flags into distributed_sddmm_amd/lib/libhnh_kernels_<name>.so
# (selected at run time with HNH_KERNEL_LIB_DEV=<path> by the kernel-level tools, or loaded whole with api.load_backend(<path>), which
# gat_skip_profile.py --kernel-lib does).  Usage: tools/build_variant.sh pipe0 -DHNH_PIPE=0
# HNH_VARIANT_TREE=<root of another checkout> compiles THAT tree's csrc/hip and include (a `git worktree` of the parent commit, say)
# into this tree's lib/: two commits' kernels side by side in one session.
set -euo pipefail
R="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
NAME=$1; shift
T="${HNH_VARIANT_TREE:-$R}"
SRC=$T/distributed_sddmm_amd/csrc/hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I"$T/include" -I"$SRC" "$@" \
  "$SRC/hnh_runtime.hip" "$SRC/hnh_kernels.hip" "$SRC/hnh_comm.hip" "$SRC/hnh_tuples.hip" "$SRC/hnh_ipc.hip" "$SRC/hnh_grad.hip" \
  -o "$R/distributed_sddmm_amd/lib/libhnh_kernels_$NAME.so" -lrccl -Wl,-Bsymbolic
