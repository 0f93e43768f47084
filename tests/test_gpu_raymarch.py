"""RayMarcher (the Mandelbulb object, raysnail src/hittable/geometry/raymarching.rs) on the GPU: World::hit records
against tests/golden/raymarch_kat.json bit for bit (the known answers of the pure-Python restatement
tests/raymarch_ref.py), the object under a TfFacade and an Intersection, and frames of the preview scene and of a
marcher used as a light in both render modes."""
import ctypes as C
import math

import numpy as np
import pytest

import raymarch_kat as K
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

pytestmark = pytest.mark.gpu

GREY = lambda: api.Lambertian(api.Color(0.5, 0.5, 0.5))  # noqa: E731  (material id 0 of every probe world)


@pytest.fixture(scope="module")
def kat():
    return K.load()


def _world(obj):
    """obj alone in the world; a light sphere in the lights list only (a pdf material needs one, list.rs:51)"""
    h, lights = api.HittableList(), api.HittableList()
    h.add(obj)
    lights.add(api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)).multiplier(1.5)))
    return api.World(h, lights)


def _probe(world, rays, tmin):
    ds = world.device_scene()
    rays = np.ascontiguousarray(np.array(rays, dtype=np.float64).reshape(-1, 7))
    out = np.full((len(rays), 13), -7.0)
    assert ds.lib.rs_probe_world_hit(ds.handle, rays.ctypes.data, len(rays), tmin, float("inf"), out.ctypes.data) == 0
    return out


def _rows_differ(got, exp):
    return [k for k in range(len(exp)) if not all(K.same(float(a), float(b)) for a, b in zip(got[k], exp[k]))]


def test_probe_matches_kat(gpu, kat):
    """the marcher alone in the world: rs_probe_world_hit on groups A-F and H, one call per distinct tmin, all 13
    doubles bit for bit"""
    world = _world(api.RayMarcher(GREY()))
    info = world.device_scene().info()
    assert info.scene_mode == 0 and info.ref_order == 1
    seen = 0
    for tmin in sorted({r["tmin"] for r in kat["rays"]}):
        recs = [r for r in kat["rays"] if r["tmin"] == tmin]
        out = _probe(world, [r["ray"] for r in recs], tmin)
        bad = _rows_differ(out, [r["exp"] for r in recs])
        assert not bad, (tmin, [(recs[k]["g"], [K.hexd(float(x)) for x in out[k]], [K.hexd(x) for x in recs[k]["exp"]])
                                for k in bad[:3]])
        seen += len(recs)
    assert seen == 100


def test_translated_marcher(gpu, kat):
    """TfFacade(translate(4, 0, -2)) of the marcher, group H with the origins shifted by the offset (exact on H's
    2^-10 grid): hit, t1, t2, the object-space normal and outside as in H, the point mapped forward
    (tf_facade.rs:41-55): p = fl((o + d t1) + offset)"""
    off = (4.0, 0.0, -2.0)
    st = api.TransformStack()
    st.push(api.Transform.translate(off))
    world = _world(api.TfFacade(api.RayMarcher(GREY()), st))
    recs = [r for r in kat["rays"] if r["g"] == "H"]
    assert len(recs) == 16 and 2 <= sum(1 for r in recs if r["exp"][0] == 1.0)
    rays = []
    for r in recs:
        o = [r["ray"][i] + off[i] for i in range(3)]
        assert all(o[i] - off[i] == r["ray"][i] for i in range(3))
        rays.append(o + r["ray"][3:7])
    exp = []
    for r in recs:
        e = list(r["exp"])
        if e[0] == 1.0:
            for i in range(3):
                e[3 + i] = e[3 + i] + off[i]
        exp.append(e)
    out = _probe(world, rays, K.TMIN)
    bad = _rows_differ(out, exp)
    assert not bad, [(k, list(out[k]), exp[k]) for k in bad[:3]]


def _project(cam, p, W, H):
    """pixel (x, y) of world point p through the pinhole of camera.rs:36-70 (row 0 is the top: painter.rs:133-139)"""
    f, a, up = np.array(cam.look_from[:]), np.array(cam.look_at[:]), np.array(cam.vup[:])
    w = (f - a) / np.linalg.norm(f - a)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    q = np.array(p) - f
    z = -np.dot(q, w)
    half = math.tan(math.radians(cam.fov) / 2.0)
    nx, ny = np.dot(q, u) / (z * half * W / H), np.dot(q, v) / (z * half)
    return (nx + 1.0) * 0.5 * W, (1.0 - ny) * 0.5 * H


def test_modes_agree_on_preview_scene(gpu):
    """raymarching_test(32, 20), 4 samples, depth 4, two seeds: the megakernel and the wavefront frames are
    bit-equal, two row_step = 2 halves assemble to the frame, every pixel is finite, and the bulb is in the
    picture: at least 10 % of the pixels inside its bbox's projection differ from the world without it (45 % of
    the known-answer camera rays into that box hit)."""
    W, H = 32, 20
    cam, world, _, _ = scenes.raymarching_test(W, H)
    cam0, world0, _, _ = scenes.raymarching_test(W, H)
    world0.hittables.objects = [o for o in world0.hittables.objects if not isinstance(o, api.RayMarcher)]
    assert len(world0.hittables.objects) == 2 and len(world.hittables.objects) == 3
    info = world.device_scene().info()
    assert info.scene_mode == 0 and info.ref_order == 1 and info.n_world == 3
    corners = [_project(cam.desc, (sx * 1.3, sy * 1.3, sz * 1.3), W, H) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    x0, x1 = max(0, int(min(c[0] for c in corners))), min(W, int(math.ceil(max(c[0] for c in corners))))
    y0, y1 = max(0, int(min(c[1] for c in corners))), min(H, int(math.ceil(max(c[1] for c in corners))))
    assert (x1 - x0) * (y1 - y0) >= 100, (x0, x1, y0, y1)
    for seed in (1, 2):
        photo = cam.take_photo().samples(4).depth(4).seed(seed)
        mega = photo.mode(A.RS_MODE_MEGAKERNEL).shot(None, world)
        wave = photo.mode(A.RS_MODE_WAVEFRONT).shot(None, world)
        assert np.isfinite(mega).all()
        assert np.array_equal(mega, wave)
        halves = np.zeros_like(wave)
        for r in range(2):
            world.device_scene().render(cam.desc, photo.rows(r, 0, 2).settings(), out=halves)
        photo.rows(0, 0, 1)
        assert np.array_equal(halves, wave)
        bare = cam0.take_photo().samples(4).depth(4).seed(seed).mode(A.RS_MODE_WAVEFRONT).shot(None, world0)
        box = np.any(wave[y0:y1, x0:x1] != bare[y0:y1, x0:x1], axis=-1)
        print(f"seed {seed}: {int(box.sum())} of {box.size} pixels of the projected box differ")
        assert box.sum() * 10 >= box.size, (int(box.sum()), box.size)


def test_cut_bulb(gpu, kat, tmp_path):
    """Intersection(RayMarcher, Box((-2, -2, -2), (2, 0, 2))), group A (camera rays, the camera outside the box).
    intersection.rs:58-100 as Obj::composite_t_calls restates it: both children are hit over the same range, the
    nearer hit wins if the OTHER object contains its point, else the farther one if the nearer object contains
    its point. A bulb hit below y = 0 lies in the box the ray entered before it, and the box's entry point is not
    in the bulb: the farther hit, the bulb's own record, is returned. Above y = 0 the bulb's point is outside the
    box; the result is the box's entry point if the bulb contains it (the cut face y = 0), else a miss."""
    shim = K.build_shim(tmp_path)
    cut = api.Intersection(api.RayMarcher(GREY()), api.Box((-2.0, -2.0, -2.0), (2.0, 0.0, 2.0), None), None)
    recs = [r for r in kat["rays"] if r["g"] == "A"]
    out = _probe(_world(cut), [r["ray"] for r in recs], K.TMIN)
    below = [k for k, r in enumerate(recs) if r["exp"][0] == 1.0 and r["exp"][4] < -0.05]
    above = [k for k, r in enumerate(recs) if r["exp"][0] == 1.0 and r["exp"][4] > 0.05]
    assert len(below) >= 4 and len(above) >= 4, (len(below), len(above))
    for k in range(len(recs)):
        assert out[k][0] in (0.0, 1.0)
        if out[k][0] == 1.0:
            assert out[k][4] <= 1e-9, (k, list(out[k]))
    bad = [k for k in below if not all(K.same(float(a), b) for a, b in zip(out[k], recs[k]["exp"]))]
    assert not bad, [(k, list(out[k]), recs[k]["exp"]) for k in bad[:3]]
    faces = 0
    for k in above:
        if out[k][0] == 1.0:
            assert abs(out[k][4]) <= 1e-9, (k, list(out[k]))
            assert shim.rm_contains((C.c_double * 3)(*out[k][3:6])) == 1, (k, list(out[k]))
            faces += 1
    print(f"cut bulb: {len(below)} hits below the cut, {len(above)} above it of which {faces} show the cut face")


def test_marcher_as_light(gpu):
    """the marcher carries a DiffuseLight and is the only entry of the lights list (Hittable::random is
    Vec3::random_unit, raymarching.rs:183-185), above a Lambertian ground: 16 x 16, 4 samples, depth 3; the frame
    is finite and not black, and both modes give it bit for bit"""
    bulb = api.RayMarcher(api.DiffuseLight(api.Color(1.0, 0.9, 0.8)).multiplier(3.0))
    h, lights = api.HittableList(), api.HittableList()
    h.add(bulb)
    h.add(api.Sphere((0.0, -1001.5, 0.0), 1000.0, api.Lambertian(api.Color(0.6, 0.6, 0.6))))
    lights.add(bulb)
    world = api.World(h, lights, api.Gradient(api.Color(0.0, 0.0, 0.0), api.Color(0.0, 0.0, 0.0)))
    cam = api.CameraBuilder().look_from(api.Point3(13.0 * 0.7, -1.7 * 0.7, 3.0 * 0.7)).look_at(api.Point3(0.0, -0.4, 0.0)) \
        .fov(20.0).aperture(0.01).focus(10.0).width(16).height(16).build()
    photo = cam.take_photo().samples(4).depth(3).seed(9)
    mega = photo.mode(A.RS_MODE_MEGAKERNEL).shot(None, world)
    wave = photo.mode(A.RS_MODE_WAVEFRONT).shot(None, world)
    assert np.isfinite(mega).all() and mega[..., :3].max() > 0.0
    assert np.array_equal(mega, wave)
    # the ground is lit by the bulb alone (black sky): some pixel below the bulb's bbox is not black
    assert mega[13:, :, :3].max() > 0.0
