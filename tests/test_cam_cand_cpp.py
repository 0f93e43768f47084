"""The candidate criterion of the spheres mode's camera launch (raysnail_amd/csrc/rs_cam_cand.h) without a GPU:
tests/cpp/test_cam_cand.cpp restates the per-pixel list build with the shared function and checks it against rays
drawn from the camera's exact ray family (every sphere a ray hits is in its pixel's record, or the record is marked
overflow), for the bench camera, a wide lens, a pinhole and a camera inside a sphere; the bench camera also over the
RTIOW scene's own spheres, handed over in a file, where at most 6 % of the pixels with candidates may overflow; and
for cameras at the edges of the criterion's own code (the `wide` threshold from both sides on either piece, a lens
below a pixel's footprint, focus negative and 0, fov 180, spheres centred on O, on a pixel's axis and of radius 0) and
the bench scene scaled by 1e-6 and 1e6, whose overflow share is capped at the bench camera's plus one point."""
import os
import subprocess

from raysnail_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cam_cand_criterion(tmp_path):
    exe = tmp_path / "test_cam_cand"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_cam_cand.cpp")], check=True)
    _, world, _, _ = scenes.rtow_13_1(96, 60)
    spheres = tmp_path / "rtiow_spheres.txt"
    with open(spheres, "w") as f:
        for o in world.hittables.objects:
            f.write("%r %r %r %r\n" % (o.center[0], o.center[1], o.center[2], o.radius))
    assert len(world.hittables.objects) > 400
    r = subprocess.run([str(exe), str(spheres)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-500:])
    assert "bench (file)" in r.stdout
    for name in ("bench x 1e-6", "bench x 1e6", "lens below", "lens above", "pinhole below", "pinhole above", "small lens",
                 "all wide", "focus 0", "focus -4", "fov 180", "special"):
        assert name in r.stdout, name
