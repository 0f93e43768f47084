"""The camera samples' trace order (raysnail_amd/csrc/rs_gen_perm.h) without a GPU: tests/cpp/test_gen_perm.cpp runs
the shared function on the CPU and checks that it is a bijection of every batch for frame widths 1 .. 20, 1 .. 12
lattice rows, 1 .. 70 sample planes, three batch origins and seven row steps, that a wave's 64 consecutive samples of
a group hold exactly 64 / SP pixels of one tile, and that a batch which is not whole planes keeps the identity."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gen_perm_is_a_bijection(tmp_path):
    exe = tmp_path / "test_gen_perm"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_gen_perm.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-500:])
    assert "117600 cases" in r.stdout
