"""The C++ host layer's TakePhotoSettings::shot_features without a GPU: tests/cpp/test_features_api.cpp, built
against include/raysnail.hpp and run here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_shot_features(hip_lib, tmp_path):
    """tests/cpp/test_features_api.cpp: World::device_scene({}) is a host-only build, and shot_features on it throws
    raysnail::Error with RS_E_STATE, with and without a PixelController"""
    lib_dir = os.path.join(ROOT, "raysnail_amd", "lib")
    exe = tmp_path / "test_features_api"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_features_api.cpp"), "-L", lib_dir, "-lraysnail_host",
                    "-lraysnail_hip", "-Wl,-rpath," + lib_dir, "-ldl"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
