#!/bin/bash
# dev: build libraysnail_hip with extra flags into raysnail_amd/lib/var_<name>.so (the same translation
# units and per-unit flags as raysnail_amd/csrc/Makefile, its unit-flags-<unit> target; compiled in parallel)
# usage: tools/build_variant.sh <name> [flags...]
#   NOUNIT=1: the Makefile's common flags for every unit (without its per-unit ones), for A/B of those
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
N=$1; shift
B=/tmp/rs_var_$N; mkdir -p $B
M="make -s --no-print-directory -C $R/raysnail_amd/csrc"
for t in common 0 1 2 3 4 5 6 7 8; do
  if [ -n "${NOUNIT:-}" ] && [ $t != common ]; then F="$($M unit-flags-common | sed 's/-DRS_TU=-1//') -DRS_TU=$t"; else F=$($M unit-flags-$t); fi
  /opt/rocm/bin/hipcc $F "$@" -c $R/raysnail_amd/csrc/rs_kernels.hip -o $B/k$t.o &
done
/opt/rocm/bin/hipcc $($M unit-flags-common | sed 's/-DRS_TU=-1//') "$@" -x hip -c $R/raysnail_amd/csrc/rs_host.cpp -o $B/h.o &
# the frame operators' units and their host unit (scene-free: the flags only name them)
for u in denoise denoise_var adaptive robust matte; do
  /opt/rocm/bin/hipcc $($M unit-flags-$u) "$@" -c $R/raysnail_amd/csrc/rs_$u.hip -o $B/k_$u.o &
done
/opt/rocm/bin/hipcc $($M unit-flags-common | sed 's/-DRS_TU=-1//') "$@" -x hip -c $R/raysnail_amd/csrc/rs_frames.cpp -o $B/h_frames.o &
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/raysnail_amd/lib/var_$N.so $B/k*.o $B/h.o $B/h_frames.o
echo built var_$N.so
