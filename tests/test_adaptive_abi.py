"""include/raysnail_adaptive.h (the adaptive-sampling part of the C-ABI, a header of its own that raysnail_hip.h
includes) against the library, the ctypes mirror, the committed layout table and INTEGRATION.md's Rust block: what
tests/test_abi.py checks for raysnail_hip.h, for this header. CPU only (no compute calls)."""
import ctypes as C
import json
import os
import re
import subprocess

from raysnail_amd import _abi as A
from test_abi import RUST_SIZE, _c_param_type, _rust_type  # the same C <-> Rust type rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raysnail_adaptive.h")
LAYOUT = os.path.join(ROOT, "tests", "golden", "abi_layout_adaptive.json")
C_OF_RUST = {"RsAdaptiveStats": "rs_adaptive_stats", "RsAdaptiveSettings": "rs_adaptive_settings",
             "RsAdaptivePass": "rs_adaptive_pass"}
CTYPES = {"rs_adaptive_stats": A.rs_adaptive_stats, "rs_adaptive_settings": A.rs_adaptive_settings,
          "rs_adaptive_pass": A.rs_adaptive_pass}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_functions():
    return {m.group(2): (m.group(1).strip(), m.group(3)) for m in
            re.finditer(r"([\w\s\*]+?)\b(rs_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header_text())}


def header_structs():
    out = {}
    for body, name in re.findall(r"typedef struct \w+ \{(.*?)\} (\w+);", header_text(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            fields += [n.strip() for n in decl[len(decl.split()[0]):].split(",")]
        out[name] = fields
    return out


def rust_block():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index("```rust\n// src/gpu/ffi_adaptive.rs"):]
    return block[:block.index("```", 7)]


def test_header_library_and_ctypes_agree(hip_lib):
    assert sorted(header_functions()) == sorted(A.ADAPTIVE_SYMBOLS)
    for name in A.ADAPTIVE_SYMBOLS:
        assert hasattr(hip_lib, name), name
        assert name not in A.EXPORTED_SYMBOLS
    assert hip_lib.rs_abi_version() == 6
    assert set(header_structs()) == set(CTYPES)
    # raysnail_hip.h includes this header: one include gives the whole boundary
    assert '#include "raysnail_adaptive.h"' in open(os.path.join(ROOT, "include", "raysnail_hip.h")).read()


def test_c_layout_matches_committed_table_and_ctypes(tmp_path):
    """offsetof / sizeof of every field, measured by gcc through raysnail_hip.h alone, equal the committed table
    (tests/golden/abi_layout_adaptive.json) and the ctypes structures"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "raysnail_hip.h"', "int main(void) {"]
    for name, fields in header_structs().items():
        lines.append(f'printf("S {name} %zu %zu\\n", sizeof({name}), _Alignof({name}));')
        for f in fields:
            lines.append(f'printf("F {name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        k = line.split()
        if k[0] == "S":
            got.setdefault(k[1], {"fields": []}).update(size=int(k[2]), align=int(k[3]))
        else:
            got[k[1]]["fields"].append([k[2], int(k[3]), int(k[4])])
    if os.environ.get("RS_WRITE_ABI_LAYOUT"):
        json.dump(got, open(LAYOUT, "w"), indent=1)
    assert got == json.load(open(LAYOUT))
    for name, cls in CTYPES.items():
        assert (C.sizeof(cls), C.alignment(cls)) == (got[name]["size"], got[name]["align"]), name
        assert [[f, getattr(cls, f).offset, getattr(cls, f).size] for f, _ in cls._fields_] == got[name]["fields"], name


def test_integration_rust_block_matches_c():
    """INTEGRATION.md's adaptive FFI block: every struct has the C struct's size, alignment and field offsets, and
    every function the header's parameter and return types in order"""
    c = json.load(open(LAYOUT))
    stats = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_layout.json")))["rs_render_stats"]
    block = rust_block()
    structs = {}
    for name, body in re.findall(r"pub struct (\w+) \{(.*?)\}", block, flags=re.S):
        structs[name] = [(f, t.strip()) for f, t in re.findall(r"pub (\w+): ([^,]+?)(?:,|$)", body.strip())]
    assert set(structs) == set(C_OF_RUST)
    for rname, cname in C_OF_RUST.items():
        off, align, fields = 0, 1, []
        for f, t in structs[rname]:
            sz, al = (stats["size"], stats["align"]) if t == "RsStats" else RUST_SIZE[t]
            off = (off + al - 1) // al * al
            fields.append([off, sz])
            off += sz
            align = max(align, al)
        assert ((off + align - 1) // align * align, align) == (c[cname]["size"], c[cname]["align"]), rname
        assert fields == [f[1:] for f in c[cname]["fields"]], rname
    rust = {m.group(1): (m.group(2), m.group(3)) for m in
            re.finditer(r"pub fn (rs_\w+)\((.*?)\)\s*(?:->\s*([^;]*))?;", block, flags=re.S)}
    funcs = header_functions()
    assert set(rust) == set(funcs)
    names = {"rs_adaptive_stats": "RsAdaptiveStats", "rs_adaptive_settings": "RsAdaptiveSettings",
             "rs_adaptive_pass": "RsAdaptivePass"}

    def c_type(decl):
        # (test_abi's table knows raysnail_hip.h's structs only: these go through it as a stand-in type)
        toks = decl.replace("*", " * ").split()
        base = next((t for t in toks if t in names), None)
        if base is None:
            return _c_param_type(decl)
        return _c_param_type(decl.replace(base, "uint8_t")).replace("u8", names[base])
    for name, (ret, args) in funcs.items():
        c_params = [c_type(a.rsplit(None, 1)[0]) for a in args.split(",")]
        r_args, r_ret = rust[name]
        r_params = [_rust_type(a.split(":", 1)[1]) for a in r_args.split(",") if a.strip()]
        assert c_params == r_params, (name, c_params, r_params)
        assert ret == "int" and _rust_type(r_ret or "") == "i32", name
