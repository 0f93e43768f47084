"""The spheres mode's camera launch finds a sample's hit among its lattice pixel's candidate spheres (a 16-byte
record per pixel, raysnail_amd/csrc/rs_cam_cand.h, built once per camera, lattice and scene on the frame slot) instead
of walking the tree; a pixel with more than 8 candidates, an exact tie of two spheres' t and a launch without records
fall back to the walk. Pure scheduling: every frame below equals the CPU oracle's bit for bit, segment count included.
A scene cycles through three frame slots, each with its own records, so a frame is rendered four times: the fourth
runs on the first one's slot, with the records that frame built."""
import numpy as np
import pytest

from raysnail_amd import scenes
from raysnail_amd.api import CameraBuilder, Color, Dielectric, DiffuseLight, Glass, Gradient, HittableList, \
    Lambertian, Metal, Point3, Sphere, World

pytestmark = pytest.mark.gpu
W, H = 96, 60
SKY = Gradient(Color(0.3, 0.4, 0.5, 1.0), Color(0.7, 0.89, 1.0, 1.0))


def _oracle(world):
    from oracle.binding import OracleScene
    return OracleScene(world)


def _photo(cam, spp=16, depth=8, seed=5):
    return cam.take_photo().samples(spp).depth(depth).seed(seed)


def _check(ds, cam, st, want, rs, times=4, mask=None, sel=slice(None), what=None):
    for k in range(times):
        img, stats = ds.render(cam.desc, st, mask)
        assert stats.segments == rs.segments, (what, k, stats.segments, rs.segments)
        assert np.array_equal(img[sel], want[sel]), (what, k)


def _device_frame(torch, ds, cam, st):
    out = torch.full((cam.desc.height, cam.desc.width, 4), -1.0, dtype=torch.float32, device="cuda")
    assert ds.render_device(cam.desc, st, out.data_ptr(), torch.cuda.current_stream().cuda_stream, stats=False) is None
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def rtow():
    """The 96 x 60 RTIOW scene, its oracle, and the oracle's (frame, stats) per settings key, computed once."""
    cam, world, _, _ = scenes.rtow_13_1(W, H)
    orc = _oracle(world)
    cache = {}

    def ref(key, photo, mask=None):
        if key not in cache:
            img, st = orc.render(cam.desc, photo.settings(), threads=16, mask=mask)
            img.setflags(write=False)
            cache[key] = (img, st)
        return cache[key]

    return cam, world, ref


@pytest.mark.parametrize("depth", [8, 1])
def test_rtiow_96x60(gpu, rtow, depth):
    cam, world, ref = rtow
    photo = _photo(cam, depth=depth)
    want, rs = ref(("depth", depth), photo)
    ds = world.device_scene()
    _check(ds, cam, photo.settings(), want, rs, what=depth)
    for _ in range(4):  # asynchronous frames on the same slots
        assert np.array_equal(_device_frame(gpu, ds, cam, photo.settings()), want), depth


def test_rtiow_64x40x9_partial_waves_and_overflow_pixels(gpu):
    """23,040 samples in groups of 8 + 1 planes; at this size a visible share of the pixels has over 8 candidates."""
    cam, world, _, _ = scenes.rtow_13_1(64, 40)
    photo = _photo(cam, spp=9, seed=7)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    _check(world.device_scene(), cam, photo.settings(), want, rs)


def _lit(h):
    """the scene's light, in both lists"""
    lights = HittableList()
    light = Sphere((0.0, 30.0, 10.0), 6.0, DiffuseLight(Color(1.0, 0.9, 0.8, 1.0)).multiplier(3.0))
    h.add(light)
    lights.add(light)
    return World(h, lights, SKY, (0.0, 0.0))


def _materials():
    return [Lambertian(Color(0.7, 0.3, 0.2, 1.0)), Metal(Color(0.7, 0.6, 0.5, 1.0)),
            Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass()), Lambertian(Color(0.2, 0.5, 0.7, 1.0))]


def test_wide_aperture(gpu):
    """Aperture 2, focus 4, spheres 0.5 - 3 units from the lens: the beams are as wide as the spheres' spacing."""
    g = np.random.default_rng(11)
    mats = _materials()
    h = HittableList()
    for i in range(16):
        r = 0.1 + 0.2 * g.random()
        dist = 0.5 + 2.5 * g.random() + r
        th, ph = (g.random() - 0.5) * 2.4, (g.random() - 0.5) * 1.6
        h.add(Sphere((dist * np.sin(th), dist * np.sin(ph), -dist * np.cos(th) * np.cos(ph)), r, mats[i % 4]))
    h.add(Sphere((0.0, -1003.0, 0.0), 1000.0, Lambertian(Color(0.5, 0.5, 0.5, 1.0))))
    world = _lit(h)
    cam = CameraBuilder().look_from(Point3(0.0, 0.0, 0.0)).look_at(Point3(0.0, 0.0, -1.0)).fov(40.0) \
        .aperture(2.0).focus(4.0).width(64).height(40).build()
    photo = _photo(cam, spp=9, depth=3, seed=2)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    _check(world.device_scene(), cam, photo.settings(), want, rs)


def test_line_of_spheres_behind_a_glass_sphere_around_the_lens(gpu):
    """Twenty small spheres along the central line of sight: every centre pixel has more than 8 candidates (its rays
    walk). The glass sphere holds the lens: the ray origin is inside a candidate of every pixel."""
    mats = _materials()
    h = HittableList()
    h.add(Sphere((0.0, 0.0, 6.0), 0.5, mats[2]))
    for i in range(20):
        h.add(Sphere((0.0, 0.0, 4.5 - 0.45 * i), 0.12, mats[i % 4]))
    h.add(Sphere((0.0, -1001.0, 0.0), 1000.0, Lambertian(Color(0.5, 0.5, 0.5, 1.0))))
    world = _lit(h)
    cam = CameraBuilder().look_from(Point3(0.0, 0.0, 6.0)).look_at(Point3(0.0, 0.0, 0.0)).fov(30.0) \
        .aperture(0.05).focus(4.0).width(64).height(40).build()
    photo = _photo(cam, spp=9, depth=4, seed=3)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    _check(world.device_scene(), cam, photo.settings(), want, rs)


def test_two_identical_spheres_tie(gpu):
    """Two spheres at one place with different materials: every ray that hits them finds the same t twice, and the
    one the walk meets first wins. The list's order is another one, so these lanes must walk."""
    h = HittableList()
    h.add(Sphere((0.0, 1.0, 0.0), 1.0, Lambertian(Color(0.8, 0.1, 0.1, 1.0))))
    h.add(Sphere((0.0, 1.0, 0.0), 1.0, Metal(Color(0.2, 0.9, 0.2, 1.0))))
    h.add(Sphere((2.1, 0.6, 0.4), 0.6, Lambertian(Color(0.2, 0.3, 0.8, 1.0))))
    h.add(Sphere((-2.0, 0.7, 0.3), 0.7, Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass())))
    h.add(Sphere((0.0, -1000.0, 0.0), 1000.0, Lambertian(Color(0.5, 0.5, 0.5, 1.0))))
    world = _lit(h)
    cam = CameraBuilder().look_from(Point3(0.0, 2.0, 8.0)).look_at(Point3(0.0, 1.0, 0.0)).fov(35.0) \
        .aperture(0.05).focus(8.0).width(64).height(40).build()
    photo = _photo(cam, spp=9, depth=4, seed=4)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    _check(world.device_scene(), cam, photo.settings(), want, rs)


@pytest.mark.parametrize("rows", [(1, 0, 3), (0, 0, 8)])
def test_row_shares_with_half_mask(gpu, rtow, rows):
    """A row share's lattice has its own records (the key holds the lattice); about half the pixels masked."""
    cam, world, ref = rtow
    yy, xx = np.indices((H, W))
    mask = (((xx // 3) + (yy // 2)) % 2 == 0).astype(np.uint8)
    photo = _photo(cam).rows(*rows)
    want, rs = ref(("mask", rows), photo, mask)
    sel = slice(rows[0], None, rows[2])
    ds = world.device_scene()
    _check(ds, cam, photo.settings(), want, rs, mask=mask, sel=sel, what=rows)
    # ... and the whole frame on the slots that hold the share's records
    full = _photo(cam)
    fwant, frs = ref(("depth", 8), full)
    _check(ds, cam, full.settings(), fwant, frs, times=3, what="full after share")


def test_pass_1_and_two_pass_stream(gpu, rtow):
    """Pass 1 is pass 1 of the oracle; as the second pass of one sample stream it equals its one-pass frame (the
    records do not depend on the pass)."""
    torch = gpu
    cam, world, ref = rtow
    ds = world.device_scene()
    singles = []
    for k in range(2):
        photo = _photo(cam).pass_index(k)
        want, rs = ref(("pass", k), photo)
        _check(ds, cam, photo.settings(), want, rs, times=2, what=("pass", k))
        singles.append(want)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        outs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        ds.render_device_passes(cam.desc, _photo(cam).settings(), [o.data_ptr() for o in outs], s)
        for k in range(2):
            assert np.array_equal(outs[k].cpu().numpy(), singles[k]), k


def test_camera_a_b_a(gpu, rtow):
    """Two cameras alternating on one scene object: every change of camera rebuilds the slot's records."""
    cam_a, world, ref = rtow
    cam_b = CameraBuilder().look_from(Point3(-6.0, 3.0, 9.0)).look_at(Point3(0.0, 0.5, 0.0)).fov(30.0) \
        .aperture(0.1).focus(9.0).width(W).height(H).build()
    orc = _oracle(world)
    pa, pb = _photo(cam_a), _photo(cam_b)
    want_a, rs_a = ref(("depth", 8), pa)
    want_b, rs_b = orc.render(cam_b.desc, pb.settings(), threads=16)
    ds = world.device_scene()
    for cam, photo, want, rs in ((cam_a, pa, want_a, rs_a), (cam_b, pb, want_b, rs_b), (cam_a, pa, want_a, rs_a),
                                 (cam_b, pb, want_b, rs_b)):
        _check(ds, cam, photo.settings(), want, rs, times=2, what="a/b")   # (slots 0 1, 2 0, 1 2, 0 1)
    _check(ds, cam_a, pa.settings(), want_a, rs_a, times=4, what="a again")


def test_commit_between_frames(gpu):
    """A second scene, one sphere moved, committed between the first one's frames: each keeps its own records."""
    def build(x):
        h = HittableList()
        h.add(Sphere((0.0, -1000.0, 0.0), 1000.0, Lambertian(Color(0.5, 0.5, 0.5, 1.0))))
        h.add(Sphere((x, 1.0, 0.0), 1.0, Lambertian(Color(0.7, 0.3, 0.2, 1.0))))
        h.add(Sphere((2.2, 0.8, 0.5), 0.8, Metal(Color(0.7, 0.6, 0.5, 1.0))))
        h.add(Sphere((-2.0, 0.7, 0.3), 0.7, Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass())))
        return _lit(h)
    cam = CameraBuilder().look_from(Point3(0.0, 2.0, 8.0)).look_at(Point3(0.0, 1.0, 0.0)).fov(35.0) \
        .aperture(0.05).focus(8.0).width(64).height(40).build()
    photo = _photo(cam, spp=9, depth=4, seed=6)
    w0, w1 = build(0.0), build(0.4)
    want0, rs0 = _oracle(w0).render(cam.desc, photo.settings(), threads=16)
    want1, rs1 = _oracle(w1).render(cam.desc, photo.settings(), threads=16)
    assert not np.array_equal(want0, want1)
    ds0 = w0.device_scene()
    _check(ds0, cam, photo.settings(), want0, rs0, what="scene 0")
    ds1 = w1.device_scene()  # the commit
    _check(ds1, cam, photo.settings(), want1, rs1, what="scene 1")
    _check(ds0, cam, photo.settings(), want0, rs0, what="scene 0 again")


def test_moving_sphere_scene_has_no_lists(gpu):
    """A moving sphere: the scene gets no records (its camera rays walk) and still matches."""
    h, lights = HittableList(), HittableList()
    h.add(Sphere((0.0, -1000.0, 0.0), 1000.0, Lambertian(Color(0.5, 0.5, 0.5, 1.0))))
    h.add(Sphere((0.0, 1.0, 0.0), 1.0, Lambertian(Color(0.7, 0.3, 0.2, 1.0))).with_speed((0.6, 0.0, 0.2)))
    h.add(Sphere((2.2, 0.8, 0.5), 0.8, Metal(Color(0.7, 0.6, 0.5, 1.0))))
    light = Sphere((0.0, 6.0, 2.0), 1.0, DiffuseLight(Color(1.0, 0.9, 0.8, 1.0)).multiplier(4.0))
    h.add(light)
    lights.add(light)
    cam = CameraBuilder().look_from(Point3(0.0, 2.0, 8.0)).look_at(Point3(0.0, 1.0, 0.0)).fov(35.0) \
        .shutter_speed(1.0).width(64).height(40).build()
    world = World(h, lights, SKY, (0.0, 1.0))
    photo = _photo(cam, spp=9, depth=4, seed=3)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    _check(world.device_scene(), cam, photo.settings(), want, rs)
