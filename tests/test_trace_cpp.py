"""The C++ host layer's ray queries (World::trace_closest, World::trace_occluded, World::object_ids) without a GPU:
tests/cpp/test_trace_api.cpp, built against include/raysnail.hpp and run here. tests/test_gpu_trace.py runs the same
driver's `gpu` mode against the Python layer, on the world and rays below."""
import os
import subprocess

import numpy as np

from raysnail_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    """compile tests/cpp/test_trace_api.cpp against the built libraries; returns the program's path"""
    lib_dir = os.path.join(ROOT, "raysnail_amd", "lib")
    exe = tmp_path / "test_trace_api"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_trace_api.cpp"), "-L", lib_dir, "-lraysnail_host",
                    "-lraysnail_hip", "-Wl,-rpath," + lib_dir, "-ldl"], check=True)
    return exe


def world():
    """the driver's world in the Python layer: (world, [ball, crate, ground])"""
    grey = api.Lambertian(api.Color(0.5, 0.5, 0.5))
    ball = api.Sphere((0.0, 0.0, 0.0), 1.0, grey)
    crate = api.Box((1.5, -1.0, -1.0), (2.5, 0.5, 1.0), grey)
    ground = api.AARect.new_xz(api.AARectMetrics(-1.0, (-8.0, 8.0), (-8.0, 8.0)), grey)
    sun = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    h, lights = api.HittableList(), api.HittableList()
    for o in (ball, crate, ground, sun):
        h.add(o)
    lights.add(sun)
    return api.World(h, lights), [ball, crate, ground]


def rays() -> np.ndarray:
    """300 rays from a ring around the objects towards points near them, tmax cycling through +inf, 6.0 and 3.0"""
    rng = np.random.default_rng(18)
    a = rng.uniform(0.0, 2.0 * np.pi, 300)
    o = np.stack([6.0 * np.cos(a), rng.uniform(-0.5, 3.0, 300), 6.0 * np.sin(a)], axis=1)
    d = rng.uniform(-2.5, 2.5, (300, 3)) * np.array([1.0, 0.6, 1.0]) - o
    tmax = np.array([np.inf, 6.0, 3.0])[np.arange(300) % 3]
    return np.ascontiguousarray(np.concatenate([o, d, np.zeros((300, 1)), tmax[:, None]], axis=1))


def test_cpp_trace_api(hip_lib, tmp_path):
    """World::device_scene({}) is a host-only build: valid trace calls throw raysnail::Error with RS_E_STATE; a ray
    table that is not 8 doubles per ray, null outputs, misaligned device pointers and a replica beyond the list with
    RS_E_INVALID; object_ids gives the export handles and RS_E_INVALID for a stranger"""
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
