# dev: the light-sample candidate lists of the bench scene on the CPU (tests/cpp/test_light_cand.cpp --lists): the
# grid, the histogram of list lengths over the cells a sphere's surface passes through, their overflow share, and how
# many of the 96 x 60 frame's first hits (the CPU oracle's world_hit of four camera samples per pixel) lie outside the
# grid or in overflow cells.
# usage: python tools/light_cand_lists.py [max_cells ...]  > profiles/light_cand/lists.txt
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raysnail_amd import scenes
from oracle.binding import OracleScene, camera_sample

tmp = tempfile.mkdtemp()
exe = os.path.join(tmp, "light_cand")
subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_light_cand.cpp")], check=True)
cam, world, _, _ = scenes.rtow_13_1(96, 60)
objs = world.hittables.objects
light = [i for i, o in enumerate(objs) if o is world.lights.objects[0]][0]
sph = os.path.join(tmp, "spheres.txt")
with open(sph, "w") as f:
    for o in objs:
        f.write("%r %r %r %r\n" % (o.center[0], o.center[1], o.center[2], o.radius))
st = cam.take_photo().samples(4).depth(8).seed(1).settings()
xys = np.array([(x, y, s) for y in range(60) for x in range(96) for s in range(4)], dtype=np.uint32)
rays = camera_sample(cam.desc, st, xys, False)
orc = OracleScene(world)
hits = os.path.join(tmp, "hits.txt")
n_sky = 0
with open(hits, "w") as f:
    for r in rays:
        h = orc.world_hit(r[0:3], r[3:6], r[6])
        if h[0]:
            f.write("%r %r %r\n" % (h[3], h[4], h[5]))
        else:
            n_sky += 1
print("bench scene (RTIOW, seed 7): %d spheres, the light is sphere %d; 96 x 60 x 4 camera samples, %d miss everything" %
      (len(objs), light, n_sky))
for mc in (sys.argv[1:] or ["0"]):
    print("== at most %s cells" % (mc if mc != "0" else "2^17 (the product's)"), flush=True)
    subprocess.run([exe, "--lists", sph, str(light), hits, mc], check=True)
