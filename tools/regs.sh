#!/bin/bash
# dev: VGPRs / scratch / occupancy of the kernels of one kernel unit (a unit of rs_kernels.hip, or one of the frame
# operators' units rs_denoise.hip, rs_denoise_var.hip, rs_adaptive.hip, rs_robust.hip, rs_matte.hip: tools/unit_src.sh) whose names
# match a pattern, compiled with exactly the flags raysnail_amd/csrc/Makefile gives that unit (its unit-flags-<unit>
# target).
# usage: tools/regs.sh <pattern> <unit> [extra hipcc flags ...]
# one line per kernel: VGPRs scratch-bytes waves/SIMD name
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
. "$R/tools/unit_src.sh"
[ $# -ge 2 ] || { echo "usage: $0 <pattern> <unit: $UNITS_USAGE> [extra hipcc flags ...]" >&2; exit 2; }
pat=$1; unit=$2; shift 2
src=$(unit_src "$unit")
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
flags=$(make -s --no-print-directory -C "$R/raysnail_amd/csrc" unit-flags-$unit)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
$HIPCC $flags "$@" -c "$R/raysnail_amd/csrc/$src" -o "$tmp/regs.o" -Rpass-analysis=kernel-resource-usage > "$tmp/log" 2>&1 \
  || { cat "$tmp/log" >&2; exit 1; }
grep -E "remark: +(Function Name|VGPRs|ScratchSize|Occupancy)" "$tmp/log" | sed -E 's/.*remark: +//; s/ \[-Rpass.*//' \
  | awk -v p="$pat" '/Function Name/{n=$3; next} /^VGPRs:/{v=$NF} /^ScratchSize/{s=$NF} /^Occupancy/{if (n ~ p) print v, s, $NF, n}'
