#!/bin/bash
# Tools builds of one translation unit with extra -D flags (the in-tree generated core is used as it is, nothing in the tree is
# rewritten, so several can be built in parallel):   tools/dbg/build_abl.sh trace -DDINER_F16_DIAG   (the TRACE instantiation)
# Another translation unit: SRC=train_core tools/dbg/build_abl.sh coretr -DDINER_CORE_TRACE
# -> tools/dbg/libdiner_hip_<name>.so (git-ignored; ships to the GPU box with the snapshot).  A/B them with tools/dbg/ab_bench.py.
set -e
cd "$(dirname "$0")/../../diner_amd/csrc"
name=$1; shift
SRC=${SRC:-points_mlp_f16}
UNROLL=""
if [ "$SRC" = points_mlp_f16 ]; then UNROLL=-fno-unroll-loops; fi
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function -Wno-inline-asm $UNROLL "$@" \
    -c $SRC.hip -o /tmp/${SRC}_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/dbg/libdiner_hip_$name.so $(ls build/*.o | grep -v "/$SRC.o") /tmp/${SRC}_$name.o
echo built tools/dbg/libdiner_hip_$name.so
