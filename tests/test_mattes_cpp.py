"""The C++ host layer's material-id mattes (TakePhotoSettings::shot_mattes, matte_extract, World::material_id) without
a GPU: tests/cpp/test_mattes_api.cpp, built against include/raysnail.hpp and run here. tests/test_gpu_mattes.py runs the
same driver's `gpu` mode against the Python layer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    """compile tests/cpp/test_mattes_api.cpp against the built libraries; returns the program's path"""
    lib_dir = os.path.join(ROOT, "raysnail_amd", "lib")
    exe = tmp_path / "test_mattes_api"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_mattes_api.cpp"), "-L", lib_dir, "-lraysnail_host",
                    "-lraysnail_hip", "-Wl,-rpath," + lib_dir, "-ldl"], check=True)
    return exe


def test_cpp_mattes_api(hip_lib, tmp_path):
    """World::device_scene({}) is a host-only build: valid shot_mattes calls throw raysnail::Error with RS_E_STATE;
    ranks 0 and 9 and a budget of 17 with RS_E_INVALID; material_id gives the export handles, RS_NO_MATERIAL for a null
    reference and RS_E_INVALID for a stranger; matte_extract refuses every invalid argument"""
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
