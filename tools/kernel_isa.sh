#!/bin/bash
# dev: the machine code of the kernels of one unit of rs_kernels.hip whose names match a pattern, as text that can be
# compared across trees: the unit compiled for the device alone with exactly the flags raysnail_amd/csrc/Makefile gives
# it (its unit-flags-<unit> target), each matching function's instructions with comments, debug directives and the
# function's index in its local labels removed, then its kernel descriptor.
# usage: tools/kernel_isa.sh <pattern> <unit: common | 0 .. 6> [--sum]     (--sum: lines and sha256 per function only)
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
[ $# -ge 2 ] || { echo "usage: $0 <pattern> <unit: common | 0 .. 6> [--sum]" >&2; exit 2; }
pat=$1; unit=$2; sum=${3:-}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
flags=$(make -s --no-print-directory -C "$R/raysnail_amd/csrc" unit-flags-$unit)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
$HIPCC $flags --offload-device-only -S "$R/raysnail_amd/csrc/rs_kernels.hip" -o "$tmp/unit.s" 2> "$tmp/log" \
  || { cat "$tmp/log" >&2; exit 1; }
python3 - "$tmp/unit.s" "$pat" "$sum" <<'PY'
import hashlib, re, sys
text, pat, only_sum = open(sys.argv[1]).read(), sys.argv[2], sys.argv[3] == "--sum"
desc = {m.group(1): m.group(2) for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, flags=re.S | re.M)}
for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
    name, body = m.group(1), m.group(2)
    if not re.search(pat, name):
        continue
    lines = [re.sub(r"\s*;.*$", "", l).rstrip() for l in body.splitlines()]
    lines = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines if l.strip() and not l.strip().startswith((".loc", ".file", ".cfi"))]
    lines += [l.rstrip() for l in desc.get(name, "").splitlines()]
    out = "\n".join(lines) + "\n"
    if only_sum:
        print(len(lines), hashlib.sha256(out.encode()).hexdigest(), name)
    else:
        print(name + ":")
        sys.stdout.write(out)
PY
