#!/bin/bash
# Build libvstrains_hip.so from the csrc of the tree this script lies in, as it stands, into tools/_ab/<name>.so (git-ignored):
# tools/ab_build.sh <name>.  To compare commits, run it in a worktree of each and copy the libraries into one tools/_ab/; then
# A/B sweeps on ONE GPU (tools/ab_sweep.sh, tools/ab_kstats.sh).
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"; name="$1"
W="$R/tools/_ab/build_$name"; rm -rf "$W"; mkdir -p "$W/vs/csrc" "$W/include"
cp "$R"/vstrains_amd/csrc/*.hip "$R"/vstrains_amd/csrc/*.h "$R"/vstrains_amd/csrc/*.cpp "$R"/vstrains_amd/csrc/Makefile "$W/vs/csrc/"
cp "$R"/include/*.h "$W/include/"
# (the Makefile names ../../include relative to csrc)
mkdir -p "$W/vs/include"; cp "$R"/include/*.h "$W/vs/include/" 2>/dev/null || true
( cd "$W/vs/csrc" && make -s -j6 )
cp "$W/vs/libvstrains_hip.so" "$R/tools/_ab/$name.so"; rm -rf "$W"; ls -la "$R/tools/_ab/$name.so"
