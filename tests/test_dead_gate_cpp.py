"""The gate of the zero-throughput rule (raysnail_amd/csrc/rs_dead_gate.h: which scenes, and which cameras, let a
streaming frame rendered without statistics end the paths whose throughput is exactly zero) without a GPU:
tests/cpp/test_dead_gate.cpp states each case -- the bench scene with one change -- and what the gate must say."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases the gate was specified with (name -> the gate's answer); the program checks more
NAMED = {
    "bench scene": 1,
    "light strictly inside a large glass sphere": 1,
    "sphere cutting the light's ball": 0,
    "sphere inside the light": 0,
    "sphere tangent to the light (outside)": 0,
    "sphere apart by half the margin": 0,
    "light tangent to its enclosing sphere (inside)": 0,
    "moving sphere (speed set)": 0,
    "moving scene (DScene::moving)": 0,
    "NaN colour (even)": 0,
    "+inf colour (even)": 0,
    "NaN multiplier": 0,
    "-inf multiplier": 0,
    "NaN background (low)": 0,
    "infinite background (high)": 0,
    "not the spheres mode": 0,
}


def test_dead_gate_cases(tmp_path):
    exe = tmp_path / "test_dead_gate"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_dead_gate.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-500:])
    assert "FAILED" not in r.stdout
    cases = {m.group(1).strip(): (int(m.group(2)), int(m.group(3)))
             for m in re.finditer(r"^case (.+?) +want (\d) got (\d)$", r.stdout, flags=re.M)}
    assert len(cases) >= 50, len(cases)
    for name, want in NAMED.items():
        assert cases.get(name) == (want, want), (name, cases.get(name))
    cams = re.findall(r"^camera (.+?) +want (\d) got (\d)$", r.stdout, flags=re.M)
    assert len(cams) == 6 and all(w == g for _, w, g in cams), cams
