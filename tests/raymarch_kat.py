"""Shared by the RayMarcher tests: tests/golden/raymarch_kat.json as doubles, and tests/cpp/raymarch_shim.cpp
(raysnail_amd/csrc/rs_raymarch.h behind C entry points) built by g++."""
import ctypes as C
import json
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "raymarch_kat.json")
TMIN = 0.0001


def dbl(h):
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


def hexd(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def same(a, b):
    """bit equality of two doubles; a NaN equals any NaN"""
    return (a != a and b != b) or hexd(a) == hexd(b)


def load():
    """{"rays": [{g, ray[7], tmin, exp[13], obj_t1}], "points": [{g, p[3], contains, dist}]}"""
    doc = json.load(open(KAT))
    for r in doc["rays"]:
        r["ray"] = [dbl(h) for h in r["ray"]]
        r["exp"] = [dbl(h) for h in r["exp"]]
        r["tmin"], r["obj_t1"] = dbl(r["tmin"]), dbl(r["obj_t1"])
    for q in doc["points"]:
        q["p"] = [dbl(h) for h in q["p"]]
        q["dist"] = dbl(q["dist"])
    return doc


def build_shim(tmp_path):
    so = tmp_path / "raymarch_shim.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-std=c++17",
                    os.path.join(ROOT, "tests", "cpp", "raymarch_shim.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.rm_hit.argtypes = [C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(C.c_double)]
    lib.rm_hit_t.argtypes = [C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]
    lib.rm_contains.argtypes = [C.POINTER(C.c_double)]
    lib.rm_distance_est.argtypes = [C.POINTER(C.c_double)]
    lib.rm_distance_est.restype = C.c_double
    return lib
