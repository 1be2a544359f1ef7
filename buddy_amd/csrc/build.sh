#!/bin/bash
# Build libbuddy_hip.so for gfx950 in-tree (buddy_amd/libbuddy_hip.so).  hipcc cross-compiles without a GPU.
# Every *.hip of this directory is a source of the library; an object is stale if its source, any *.h here or the public header is newer.
set -e -o pipefail
cd "$(dirname "$0")"
OUT=../libbuddy_hip.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -Wno-unused-result"
JOBS=${MAX_JOBS:-16}
[ "$JOBS" -ge 1 ] 2>/dev/null && [ "$JOBS" -le 16 ] || JOBS=16          # at most 16 compiles in flight, whatever the machine's core count
mkdir -p obj
objs=()
stale=()
for src in *.hip; do
  f=${src%.hip}
  objs+=(obj/$f.o)
  for dep in $src *.h ../../include/buddy_hip.h; do
    if [ ! -f obj/$f.o ] || [ $dep -nt obj/$f.o ]; then stale+=($f); break; fi
  done
done
# xargs exits non-zero if any compile failed, which ends the script (set -e) before the link: a stale object is never linked
printf '%s\n' "${stale[@]}" | xargs -r -P "$JOBS" -I{} hipcc $FLAGS -c {}.hip -o obj/{}.o
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT "${objs[@]}"
echo "built $(readlink -f $OUT)"
