#!/bin/bash
# Builds libovm3d.so for gfx950 in-tree (the .so travels to the GPU box with the repo snapshot).
set -e
cd "$(dirname "$0")"
OUT=../libovm3d.so
mkdir -p build
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result"
# OVM_DIAG=1: diagnostic build (in-kernel s_memtime stamps and the timing-only attention ablations of scratch/; never shipped) - delete build/ when switching
if [ -n "$OVM_DIAG" ]; then FLAGS="$FLAGS -DOVM_DIAG"; fi
pids=()
OBJS="gemm gemm256 mlp_fused gemm_small elementwise attn attn64 roi_cube det2d ops gops gdino_kernels dec_chain gdino gdino_load gdino_plan box3d eval_match eval3d geo ground resize jpeg jpeg_enc jpeg_dec mask_rle mask_cc mask_overlay scene_ply render panels loader tower sam depthpro api"
for f in $OBJS; do
  if [ ! -f build/$f.o ] || [ $f.hip -nt build/$f.o ] || [ -n "$(find . -maxdepth 1 -name '*.hpp' -newer build/$f.o)" ] || [ ../../include/ovm3d.h -nt build/$f.o ]; then
    # at most 16 compiles at once
    if [ ${#pids[@]} -ge 16 ]; then wait ${pids[0]}; pids=("${pids[@]:1}"); fi
    hipcc $FLAGS -c $f.hip -o build/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $(for f in $OBJS; do printf 'build/%s.o ' $f; done) -L/opt/rocm/lib -lrccl
echo "built $OUT"
