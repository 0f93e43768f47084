"""The C++ host layer's pass_robust and the `robust` argument of TakePhotoSettings::shot_denoised_passes:
tests/cpp/test_robust_api.cpp, built against include/raysnail.hpp and run here without a GPU, and once on the GPU
against the Python layer."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    lib_dir = os.path.join(ROOT, "raysnail_amd", "lib")
    exe = tmp_path / "test_robust_api"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_robust_api.cpp"), "-L", lib_dir, "-lraysnail_host",
                    "-lraysnail_hip", "-Wl,-rpath," + lib_dir, "-ldl"], check=True)
    return exe


def test_cpp_robust_api(hip_lib, tmp_path):
    """ROBUST_AUTO is the header's; every invalid trim and frame list throws raysnail::Error with RS_E_INVALID, from
    pass_robust and, before anything renders, from shot_denoised_passes; the default and every valid value go on to the
    first pass"""
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])


@pytest.mark.gpu
def test_cpp_robust_on_the_gpu(gpu, tmp_path):
    """the driver's `gpu` mode: shot_denoised_passes (8 x 6, 4 passes of 4 samples, seed 3, from pass 1, every other
    pixel masked, robust = ROBUST_AUTO) and pass_robust (trim 0.25) over the same four passes write the frames the Python
    layer computes of the same world"""
    from raysnail_amd import api
    exe, out = build_driver(tmp_path), tmp_path / "frames.bin"
    r = subprocess.run([str(exe), "gpu", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
    raw = np.fromfile(out, np.uint8)
    got = raw[:5 * 6 * 8 * 16].view(np.float32).reshape(5, 6, 8, 4)
    got_trimmed = raw[5 * 6 * 8 * 16:].reshape(6, 8)
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
    den, mean, var = cam.take_photo().samples(4).seed(3).pass_index(1).shot_denoised_passes(
        world, 4, EveryOther(), robust="auto")
    frames = [cam.take_photo().samples(4).seed(3).pass_index(1 + k).shot_to_target(None, world, None, None, EveryOther())
              for k in range(4)]
    rmean, rvar, trimmed = api.pass_robust(frames, True, 0.25)
    for f in (den, mean, var, rmean, rvar):
        assert (f[1::2, 0::2] == 0.0).all()  # masked pixels stay [0,0,0,0]
    assert (var[0::2, 0::2, 3] == 4.0).all() and (trimmed[0::2, 0::2] == 1).all() and (trimmed[1::2, 0::2] == 0).all()
    for g, e in zip(got, (den, mean, var, rmean, rvar)):
        assert np.array_equal(g.view(np.uint32), e.view(np.uint32))
    assert np.array_equal(got_trimmed, trimmed)
