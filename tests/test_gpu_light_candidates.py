"""The spheres mode's carried launch finds the hit of a light-sample ray (the front run of a carried set) among the
candidate spheres of the cell of space it starts in (a 16-byte record per cell of a uniform grid,
raysnail_amd/csrc/rs_light_cand.h, built once per scene commit) instead of walking the tree; a ray from outside the
grid, one that fails the membership check, one from a cell with more than 8 candidates and an exact tie of two
spheres' t fall back to the walk, and a scene with two lights or a moving sphere gets no records. Pure scheduling:
every frame below equals the CPU oracle's bit for bit, segment count included."""
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


def _check(ds, cam, st, want, rs, times=2, mask=None, sel=slice(None), what=None):
    for k in range(times):
        img, stats = ds.render(cam.desc, st, mask)
        assert stats.segments == rs.segments, (what, k, stats.segments, rs.segments)
        assert np.array_equal(img[sel], want[sel]), (what, k)


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


@pytest.mark.parametrize("depth", [8, 2])
def test_rtiow_96x60(gpu, rtow, depth):
    """Depth 2: the light-sample rays of the first scatter are the only carried front run."""
    cam, world, ref = rtow
    photo = _photo(cam, depth=depth)
    want, rs = ref(("depth", depth), photo)
    ds = world.device_scene()
    _check(ds, cam, photo.settings(), want, rs, times=4, what=depth)   # (three frame slots: the fourth reuses the first)
    out = gpu.full((H, W, 4), -1.0, dtype=gpu.float32, device="cuda")
    assert ds.render_device(cam.desc, photo.settings(), out.data_ptr(), gpu.cuda.current_stream().cuda_stream, stats=False) is None
    gpu.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want), depth


def test_rtiow_64x40x9_partial_waves(gpu):
    cam, world, _, _ = scenes.rtow_13_1(64, 40)
    photo = _photo(cam, spp=9, seed=7)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    _check(world.device_scene(), cam, photo.settings(), want, rs)


def _materials():
    return [Lambertian(Color(0.7, 0.3, 0.2, 1.0)), Metal(Color(0.7, 0.6, 0.5, 1.0)),
            Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass()), Lambertian(Color(0.2, 0.5, 0.7, 1.0))]


def _field(g, n=6, extra=()):
    """n x n balls of radius 0.2 on a ground sphere, three larger spheres, and `extra`"""
    mats = _materials()
    h = HittableList()
    h.add(Sphere((0.0, -1000.0, 0.0), 1000.0, Lambertian(Color(0.5, 0.5, 0.5, 1.0))))
    k = 0
    for a in range(-n // 2, n - n // 2):
        for b in range(-n // 2, n - n // 2):
            h.add(Sphere((a + 0.9 * g.random(), 0.2, b + 0.9 * g.random()), 0.2, mats[k % 4]))
            k += 1
    h.add(Sphere((0.0, 1.0, 0.0), 1.0, mats[2]))
    h.add(Sphere((-2.2, 0.7, 0.6), 0.7, mats[0]))
    h.add(Sphere((2.1, 0.6, -0.4), 0.6, mats[1]))
    for s in extra:
        h.add(s)
    return h


def _world(h, lights_at, times=(0.0, 0.0)):
    lights = HittableList()
    for c, r in lights_at:
        light = Sphere(c, r, DiffuseLight(Color(1.0, 0.9, 0.8, 1.0)).multiplier(3.0))
        h.add(light)
        lights.add(light)
    return World(h, lights, SKY, times)


def _cam(w=64, h=40):
    return CameraBuilder().look_from(Point3(0.5, 2.5, 9.0)).look_at(Point3(0.0, 0.6, 0.0)).fov(35.0) \
        .aperture(0.05).focus(9.0).width(w).height(h).build()


def _render_and_check(world, cam, spp=9, depth=4, seed=3, times=2):
    photo = _photo(cam, spp=spp, depth=depth, seed=seed)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    _check(world.device_scene(), cam, photo.settings(), want, rs, times=times)


def test_light_just_above_the_ball_layer(gpu):
    """A light of radius 0.5 at height 1.6 over the field: it lies inside the grid, the beams of the cells around it are
    wide (their records overflow), beams from farther cells run along the layer through many balls (overflow as
    well), others have short lists: walking and list lanes mix in one wave."""
    world = _world(_field(np.random.default_rng(21), n=8), [((0.4, 1.6, 1.3), 0.5)])
    _render_and_check(world, _cam())


def test_two_identical_spheres_between_the_scatter_points_and_the_light(gpu):
    """Two spheres at one place with different materials, between the field and the light: a light-sample ray that
    hits them finds the same t twice, and the one the walk meets first wins. The list's order is another one, so
    these lanes must walk."""
    twins = [Sphere((1.5, 2.2, 0.5), 0.8, Lambertian(Color(0.8, 0.1, 0.1, 1.0))),
             Sphere((1.5, 2.2, 0.5), 0.8, Metal(Color(0.2, 0.9, 0.2, 1.0)))]
    world = _world(_field(np.random.default_rng(22), extra=twins), [((30.0, 40.0, 10.0), 4.0)])
    _render_and_check(world, _cam())


def test_two_lights_scene_has_no_lists(gpu):
    world = _world(_field(np.random.default_rng(23)), [((30.0, 40.0, 10.0), 4.0), ((-20.0, 30.0, -5.0), 3.0)])
    _render_and_check(world, _cam())


def test_moving_sphere_scene_has_no_lists(gpu):
    g = np.random.default_rng(24)
    mover = Sphere((1.0, 1.6, 1.5), 0.4, Lambertian(Color(0.7, 0.3, 0.2, 1.0))).with_speed((0.6, 0.0, 0.2))
    world = _world(_field(g, extra=[mover]), [((30.0, 40.0, 10.0), 4.0)], times=(0.0, 1.0))
    cam = CameraBuilder().look_from(Point3(0.5, 2.5, 9.0)).look_at(Point3(0.0, 0.6, 0.0)).fov(35.0) \
        .shutter_speed(1.0).width(64).height(40).build()
    _render_and_check(world, cam)


def test_commit_between_frames(gpu):
    """A second scene, its light elsewhere (other cells, other lists), committed between the first one's frames: each
    keeps its own records."""
    cam = _cam()
    photo = _photo(cam, spp=9, depth=4, seed=6)
    w0 = _world(_field(np.random.default_rng(25)), [((30.0, 40.0, 10.0), 4.0)])
    w1 = _world(_field(np.random.default_rng(25)), [((-25.0, 35.0, 15.0), 4.0)])
    want0, rs0 = _oracle(w0).render(cam.desc, photo.settings(), threads=16)
    want1, rs1 = _oracle(w1).render(cam.desc, photo.settings(), threads=16)
    assert not np.array_equal(want0, want1)
    ds0 = w0.device_scene()
    _check(ds0, cam, photo.settings(), want0, rs0, what="scene 0")
    ds1 = w1.device_scene()  # the commit
    _check(ds1, cam, photo.settings(), want1, rs1, what="scene 1")
    _check(ds0, cam, photo.settings(), want0, rs0, what="scene 0 again")


def test_row_share_with_half_mask(gpu, rtow):
    cam, world, ref = rtow
    rows = (1, 0, 3)
    yy, xx = np.indices((H, W))
    mask = (((xx // 3) + (yy // 2)) % 2 == 0).astype(np.uint8)
    photo = _photo(cam).rows(*rows)
    want, rs = ref(("mask", rows), photo, mask)
    _check(world.device_scene(), cam, photo.settings(), want, rs, mask=mask, sel=slice(rows[0], None, rows[2]), what=rows)


def test_pass_1_of_a_two_pass_stream(gpu, rtow):
    """Pass 1 as the second pass of one sample stream equals the oracle's pass 1 (the records depend on no pass)."""
    torch = gpu
    cam, world, ref = rtow
    ds = world.device_scene()
    singles = [ref(("pass", k), _photo(cam).pass_index(k))[0] for k in range(2)]
    photo1 = _photo(cam).pass_index(1)
    _check(ds, cam, photo1.settings(), singles[1], ref(("pass", 1), photo1)[1], what="pass 1")
    outs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    ds.render_device_passes(cam.desc, _photo(cam).settings(), [o.data_ptr() for o in outs], torch.cuda.current_stream().cuda_stream)
    for k in range(2):
        assert np.array_equal(outs[k].cpu().numpy(), singles[k]), k
