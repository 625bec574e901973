#!/bin/bash
# Developer script: build the working tree's library as offline_raytracer_amd/lib/libort_<tag>.so (A/B runs through ORT_LIB).
# Every kernel unit is compiled with the flags csrc/Makefile compiles it with (make print-kernel-flags), the host sources with
# its FLAGS (make print-flags); what is given here is added to them.
# usage: [W5FLAGS=...] [UNITFLAGS_<unit>=...] tools/build_variant.sh [--dry-run] <tag> [extra hipcc flags for ort_kernels.hip and the host sources, e.g. -DORT_PROLOGUE_DEFER=0]
# (W5FLAGS: extra flags for the five-waves unit ort_kernels_w5.hip; UNITFLAGS_ort_kernels_adaptive=... and so on: for that unit)
# --dry-run prints the commands, one line each, and builds nothing.
set -e
cd "$(dirname "$0")/../offline_raytracer_amd/csrc"
dry=0
if [ "$1" = "--dry-run" ]; then dry=1; shift; fi
tag=$1; shift
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
run() { if [ $dry = 1 ]; then echo "$@"; else "$@"; fi; }
[ $dry = 1 ] || mkdir -p ../lib/.build
objs=""
pids=""
for u in $(make -s print-kernel-units); do
  extra=UNITFLAGS_$u
  extra="${!extra}"
  [ $u = ort_kernels_w5 ] && extra="$W5FLAGS $extra"
  o=../lib/.build/${u}_$tag.o
  objs="$objs $o"
  kflags=$(make -s print-kernel-flags UNIT=$u)
  if [ $u = ort_kernels ]; then extra="$extra $*"; fi
  if [ $dry = 1 ]; then
    echo "$HIPCC" $kflags $extra -x hip -c $u.hip -o $o
  else   # the units compile side by side
    "$HIPCC" $kflags $extra -x hip -c $u.hip -o $o &
    pids="$pids $!"
  fi
done
for p in $pids; do wait $p; done
run "$HIPCC" $(make -s print-flags) "$@" -shared -x hip ort_api.cpp ort_parse.cpp ort_tree.cpp ort_reftree.cpp ort_hdr.cpp ort_comm.cpp \
  -x none $objs -o ../lib/libort_$tag.so -ldl
[ $dry = 1 ] || ls -la ../lib/libort_$tag.so
