"""The per-cell candidate lists of the spheres mode's light-sample rays (raysnail_amd/csrc/rs_light_cand.h) without a
GPU: tests/cpp/test_light_cand.cpp restates the list build by brute force with the shared functions (the cell index,
the cell's ball, the membership check, the criterion) and checks it against rays drawn from the exact family -- every
sphere a ray hits is in the record of the cell its origin maps to, or the record is marked overflow -- for the bench
scene (the RTIOW scene's own spheres, handed over in a file, and an RTIOW-shaped field), a huge light one cell from the
grid (every cell overflows), a light inside the grid, a 0.01-radius sphere 1,000 units along a beam, and two identical
spheres; lists built for 0.7 of the light's radius or of the cell ball must miss hits; non-finite and out-of-box
origins map to "outside"."""
import os
import subprocess

from raysnail_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_light_cand_criterion(tmp_path):
    exe = tmp_path / "test_light_cand"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_light_cand.cpp")], check=True)
    _, world, _, _ = scenes.rtow_13_1(96, 60)
    objs = world.hittables.objects
    assert len(objs) > 400 and len(world.lights.objects) == 1
    light = [i for i, o in enumerate(objs) if o is world.lights.objects[0]]
    assert len(light) == 1
    spheres = tmp_path / "rtiow_spheres.txt"
    with open(spheres, "w") as f:
        for o in objs:
            f.write("%r %r %r %r\n" % (o.center[0], o.center[1], o.center[2], o.radius))
    r = subprocess.run([str(exe), str(spheres), str(light[0])], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-500:])
    for name in ("bench (file)", "bench ", "huge light", "light inside", "far small sphere", "twins", "rho x 0.7", "ball x 0.7"):
        assert name in r.stdout, name
