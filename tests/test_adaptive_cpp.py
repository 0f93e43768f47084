"""The C++ host layer's AdaptiveSettings and TakePhotoSettings::shot_adaptive: tests/cpp/test_adaptive_api.cpp, built
against include/raysnail.hpp and run here without a GPU, and once on the GPU against the Python layer."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    lib_dir = os.path.join(ROOT, "raysnail_amd", "lib")
    exe = tmp_path / "test_adaptive_api"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_adaptive_api.cpp"), "-L", lib_dir, "-lraysnail_host",
                    "-lraysnail_hip", "-Wl,-rpath," + lib_dir, "-ldl"], check=True)
    return exe


def test_cpp_adaptive_api(hip_lib, tmp_path):
    """AdaptiveSettings' defaults are the header's; every invalid setting throws raysnail::Error with RS_E_INVALID and
    the C entry leaves its buffers alone; shot_adaptive throws RS_E_STATE on a host-only build"""
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])


@pytest.mark.gpu
def test_cpp_shot_adaptive_on_the_gpu(gpu, tmp_path):
    """the driver's `gpu` mode: raysnail::TakePhotoSettings::shot_adaptive (8 x 6, 4 samples per pass, seed 3, from pass
    1, at most 6 passes, every other pixel masked) writes the frames and reports the Python layer computes of the same
    world"""
    from raysnail_amd import api
    exe, out = build_driver(tmp_path), tmp_path / "frames.f32"
    r = subprocess.run([str(exe), "gpu", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
    got = np.fromfile(out, np.float32).reshape(2, 6, 8, 4)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("passes ")][0].split()
    hl, lights = api.HittableList(), api.HittableList()
    sun = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    hl.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    hl.add(sun)
    lights.add(sun)
    world = api.World(hl, lights)
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(8).height(6).build()

    class EveryOther(api.PixelController):
        def calculate_pixel(self, x, y):
            return (x + y) % 2 == 0
    mean, var, passes, reports = cam.take_photo().samples(4).seed(3).pass_index(1).shot_adaptive(
        world, api.AdaptiveSettings(max_passes=6), EveryOther())
    assert (mean[1::2, 0::2] == 0.0).all() and (var[1::2, 0::2] == 0.0).all() and (passes[0::2, 0::2] >= 2).all()
    assert [int(v) for v in line[1:]] == [len(reports)] + [r.active for r in reports]
    for g, e in zip(got, (mean, var)):
        assert np.array_equal(g.view(np.uint32), e.view(np.uint32))
