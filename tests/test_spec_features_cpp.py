"""The C++ host layer's specular-chain parameters (shot_features' max_specular, shot_denoised and
shot_denoised_passes' guide_specular) without a GPU: tests/cpp/test_spec_features_api.cpp, built against
include/raysnail.hpp and run here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    """compile tests/cpp/test_spec_features_api.cpp against the built libraries; returns the program's path"""
    lib_dir = os.path.join(ROOT, "raysnail_amd", "lib")
    exe = tmp_path / "test_spec_features_api"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_spec_features_api.cpp"), "-L", lib_dir, "-lraysnail_host",
                    "-lraysnail_hip", "-Wl,-rpath," + lib_dir, "-ldl"], check=True)
    return exe


def test_cpp_specular_parameters(hip_lib, tmp_path):
    """World::device_scene({}) is a host-only build: the defaulted calls and the calls with a budget up to 16 throw
    raysnail::Error with RS_E_STATE, a budget of 17 with RS_E_INVALID, with and without a PixelController"""
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
