#!/bin/bash
# dev: the machine code of the kernels of one kernel unit whose names match a pattern, as text that can be compared
# across trees: the unit compiled for the device alone with exactly the flags raysnail_amd/csrc/Makefile gives it (its
# unit-flags-<unit> target), each matching function's instructions with comments, debug directives and the function's
# index in its local labels removed, then its kernel descriptor. A function is shown under its base name (the
# demangled name without namespaces and argument types, template arguments kept), and its own mangled name is replaced
# by that wherever it occurs: a kernel whose argument type was renamed compares equal.
# usage: tools/kernel_isa.sh <pattern> <unit> [--sum]     (--sum: lines, sha256 and base name per function only)
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
. "$R/tools/unit_src.sh"
[ $# -ge 2 ] || { echo "usage: $0 <pattern> <unit: $UNITS_USAGE> [--sum]" >&2; exit 2; }
pat=$1; unit=$2; sum=${3:-}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
flags=$(make -s --no-print-directory -C "$R/raysnail_amd/csrc" unit-flags-$unit)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
$HIPCC $flags --offload-device-only -S "$R/raysnail_amd/csrc/$(unit_src "$unit")" -o "$tmp/unit.s" 2> "$tmp/log" \
  || { cat "$tmp/log" >&2; exit 1; }
python3 - "$tmp/unit.s" "$pat" "$sum" <<'PY'
import hashlib, re, subprocess, sys
text, pat, only_sum = open(sys.argv[1]).read(), sys.argv[2], sys.argv[3] == "--sum"
desc = {m.group(1): m.group(2) for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, flags=re.S | re.M)}
funcs = [(m.group(1), m.group(2)) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M)
         if re.search(pat, m.group(1))]
def base_names(names):
    if not names:
        return []
    full = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = []
    for s in full[:len(names)]:
        s = s.replace("(anonymous namespace)::", "")
        depth = 0
        for i, ch in enumerate(s):  # cut the argument list: the first "(" outside the template arguments
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                s = s[:i]
                break
        out.append(re.sub(r"^(\w+ )?(\w+::)*", "", s).replace(" ", ""))
    return out
for (name, body), base in sorted(zip(funcs, base_names([f[0] for f in funcs])), key=lambda t: t[1]):
    lines = [re.sub(r"\s*;.*$", "", l).rstrip() for l in body.splitlines()]
    lines = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines if l.strip() and not l.strip().startswith((".loc", ".file", ".cfi"))]
    lines += [l.rstrip() for l in desc.get(name, "").splitlines()]
    out = "\n".join(lines).replace(name, base) + "\n"
    if only_sum:
        print(len(lines), hashlib.sha256(out.encode()).hexdigest(), base)
    else:
        print(base + ":")
        sys.stdout.write(out)
PY
