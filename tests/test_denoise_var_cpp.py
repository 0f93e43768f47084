"""The C++ host layer's pass_moments, denoise_var and TakePhotoSettings::shot_denoised_passes without a GPU:
tests/cpp/test_denoise_var_api.cpp, built against include/raysnail.hpp and run here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    lib_dir = os.path.join(ROOT, "raysnail_amd", "lib")
    exe = tmp_path / "test_denoise_var_api"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_denoise_var_api.cpp"), "-L", lib_dir, "-lraysnail_host",
                    "-lraysnail_hip", "-Wl,-rpath," + lib_dir, "-ldl"], check=True)
    return exe


def test_cpp_denoise_var_api(hip_lib, tmp_path):
    """tests/cpp/test_denoise_var_api.cpp: DenoiseVarSettings' defaults are the header's; every invalid argument of
    raysnail::denoise_var and raysnail::pass_moments throws raysnail::Error with RS_E_INVALID and leaves the frames
    alone; shot_denoised_passes throws RS_E_INVALID below 2 passes and RS_E_STATE on a host-only build"""
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
