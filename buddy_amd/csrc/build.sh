#!/bin/bash
# Build libbuddy_hip.so for gfx950 in-tree (buddy_amd/libbuddy_hip.so).  hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
OUT=../libbuddy_hip.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -Wno-unused-result"
mkdir -p obj
pids=()
for f in options igemm wgemm wgemm16 wprep wino wino4 wino6 ops attn attn16 sampler net operator wpe wpe_mc mpdr resample acoustics metrics align srmr decay level spectral ism wgrad optim rng noise tail denoise compare capi; do
  if [ ! -f obj/$f.o ] || [ $f.hip -nt obj/$f.o ] || [ common.h -nt obj/$f.o ] || [ wgemm_tile.h -nt obj/$f.o ] || [ net.h -nt obj/$f.o ] || [ fft512.h -nt obj/$f.o ] || [ reduce.h -nt obj/$f.o ] || [ select.h -nt obj/$f.o ] || [ philox.h -nt obj/$f.o ] || [ ../../include/buddy_hip.h -nt obj/$f.o ]; then
    hipcc $FLAGS -c $f.hip -o obj/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT obj/options.o obj/igemm.o obj/wgemm.o obj/wgemm16.o obj/wprep.o obj/wino.o obj/wino4.o obj/wino6.o obj/ops.o obj/attn.o obj/attn16.o obj/sampler.o obj/net.o obj/operator.o obj/wpe.o obj/wpe_mc.o obj/mpdr.o obj/resample.o obj/acoustics.o obj/metrics.o obj/align.o obj/srmr.o obj/decay.o obj/level.o obj/spectral.o obj/ism.o obj/wgrad.o obj/optim.o obj/rng.o obj/noise.o obj/tail.o obj/denoise.o obj/compare.o obj/capi.o
echo "built $(readlink -f $OUT)"
