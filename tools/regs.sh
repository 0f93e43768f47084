#!/bin/bash
# dev: VGPRs / scratch / occupancy of the kernels of one unit of rs_kernels.hip (or of rs_denoise.hip: unit `denoise`;
# of rs_denoise_var.hip: unit `denoise_var`; of rs_adaptive.hip: unit `adaptive`; of rs_robust.hip: unit `robust`) whose names match a pattern, compiled with exactly the flags raysnail_amd/csrc/Makefile gives that unit (its
# unit-flags-<unit> target).
# usage: tools/regs.sh <pattern> <unit: common | 0 .. 6 | denoise | denoise_var | adaptive | robust> [extra hipcc flags ...]
# one line per kernel: VGPRs scratch-bytes waves/SIMD name
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
[ $# -ge 2 ] || { echo "usage: $0 <pattern> <unit: common | 0 .. 6 | denoise | denoise_var | adaptive | robust> [extra hipcc flags ...]" >&2; exit 2; }
pat=$1; unit=$2; shift 2
src=rs_kernels.hip
[ "$unit" = denoise ] && src=rs_denoise.hip
[ "$unit" = denoise_var ] && src=rs_denoise_var.hip
[ "$unit" = adaptive ] && src=rs_adaptive.hip
[ "$unit" = robust ] && src=rs_robust.hip
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
flags=$(make -s --no-print-directory -C "$R/raysnail_amd/csrc" unit-flags-$unit)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
$HIPCC $flags "$@" -c "$R/raysnail_amd/csrc/$src" -o "$tmp/regs.o" -Rpass-analysis=kernel-resource-usage > "$tmp/log" 2>&1 \
  || { cat "$tmp/log" >&2; exit 1; }
grep -E "remark: +(Function Name|VGPRs|ScratchSize|Occupancy)" "$tmp/log" | sed -E 's/.*remark: +//; s/ \[-Rpass.*//' \
  | awk -v p="$pat" '/Function Name/{n=$3; next} /^VGPRs:/{v=$NF} /^ScratchSize/{s=$NF} /^Occupancy/{if (n ~ p) print v, s, $NF, n}'
