"""A streaming frame rendered without statistics ends the paths whose throughput is exactly zero at the scatter that
zeroes them (raysnail_amd/csrc/rs_dead_gate.h, WfState::end_dead): such a path can only add +0.0 to its sample, which is
what it is closed with. A frame that reports rs_render_stats traces them to their ends, because `segments` is the
reference's count. Both frames equal the CPU oracle's bit for bit, on scenes that do contain dead paths, and the
statistics frame's segments and samples equal the oracle's.

The scenes' dead paths, counted on the oracle's side. The issue asked for the count of samples whose radiance is exactly
(0, 0, 0) at depth 8 to be well above that count at depth 1. As worded that cannot hold on any scene: at depth 1 every
sample whose camera ray hits a surface is exactly zero (the next level returns 0), and a sample that is zero at depth 8
hit a surface first, so the depth-8 set is a subset of the depth-1 set (RTIOW 96 x 60 x 16: 63 % of the samples at
depth 1). What the check is for is kept, and made exact: a sample whose path ended BEFORE the depth limit (the oracle's
segment count of the sample < depth) ended at the sky, at the light, or absorbed; sky and light colours are positive in
every scene here and nothing absorbs on the outside of a sphere, so such a sample is exactly (0, 0, 0) only if its
throughput was zero when it got there -- a dead path, traced to its end by the oracle. That count is 0 at depth 1 by
construction and must be at least 1 % of the samples at the scene's depth (the issue's own CPU count has 3.2 % of the
samples die at their first scatter alone, 12,872 of 400,000); measured per scene on the oracle: see DEAD_MEASURED."""
import numpy as np
import pytest

from raysnail_amd import scenes
from raysnail_amd.api import CameraBuilder, Checker, Color, Dielectric, DiffuseLight, DiffuseMetal, Glass, Gradient, \
    HittableList, Lambertian, Metal, Point3, Sphere, World

pytestmark = pytest.mark.gpu
W, H = 96, 60
SKY = Gradient(Color(0.3, 0.4, 0.5, 1.0), Color(0.7, 0.89, 1.0, 1.0))
# oracle-side shares of dead samples (see the module docstring) on every fourth pixel, as measured when the test was
# written (printed by every run): scene -> share at the scene's depth
DEAD_MEASURED = {"rtiow depth 8": 0.0566, "rtiow depth 50": 0.0771, "black ball": 0.1203, "diffuse metal": 0.0317,
                 "ball cutting the light": 0.0112}


def _oracle(world):
    from oracle.binding import OracleScene
    return OracleScene(world)


def _photo(cam, spp=16, depth=8, seed=5):
    return cam.take_photo().samples(spp).depth(depth).seed(seed)


def dead_share(orc, cam, photo, depth, stride=4):
    """The share of the samples of every stride-th pixel that are exactly (0, 0, 0) although their path ended before
    the depth limit: dead paths (module docstring)."""
    st = photo.depth(depth).settings()
    n_s = int(np.floor(np.sqrt(st.samples))) ** 2
    pix = [(x, y) for y in range(cam.desc.height) for x in range(cam.desc.width) if (x + 2 * y) % stride == 0]
    dead = total = 0
    for x, y in pix:
        for s in range(n_s):
            rad, seg = orc.sample_radiance(cam.desc, st, x, y, s)
            total += 1
            dead += int(seg < depth and not rad.any())
    return dead / total


def _field(g, n=6, extra=()):
    """n x n balls of radius 0.2 on a ground sphere, three larger spheres, and `extra`"""
    mats = [Lambertian(Color(0.7, 0.3, 0.2, 1.0)), Metal(Color(0.7, 0.6, 0.5, 1.0)),
            Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass()), Lambertian(Color(0.2, 0.5, 0.7, 1.0))]
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


def _world(h, light_at=((30.0, 40.0, 10.0), 4.0)):
    lights = HittableList()
    light = Sphere(light_at[0], light_at[1], DiffuseLight(Color(1.0, 0.9, 0.8, 1.0)).multiplier(3.0))
    h.add(light)
    lights.add(light)
    return World(h, lights, SKY, (0.0, 0.0))


def _cam(w=64, h=40):
    return CameraBuilder().look_from(Point3(0.5, 2.5, 9.0)).look_at(Point3(0.0, 0.6, 0.0)).fov(35.0) \
        .aperture(0.05).focus(9.0).width(w).height(h).build()


def _plain(torch, ds, cam, st, mask=None):
    """The frame rendered without statistics (render_device, stats=False), from device memory prefilled with -1"""
    out = torch.full((cam.desc.height, cam.desc.width, 4), -1.0, dtype=torch.float32, device="cuda")
    d_mask = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).cuda() if mask is not None else None
    assert ds.render_device(cam.desc, st, out.data_ptr(), torch.cuda.current_stream().cuda_stream,
                            d_mask.data_ptr() if d_mask is not None else 0, stats=False) is None
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_scene(torch, world, cam, photo, depth, name, dead_expected=True):
    """plain == statistics == oracle, the statistics frame's counts == the oracle's, and the scene has dead paths"""
    orc = _oracle(world)
    st = photo.depth(depth).settings()
    want, rs = orc.render(cam.desc, st, threads=16)
    share0, share = dead_share(orc, cam, photo, 1), dead_share(orc, cam, photo, depth)
    print(f"{name}: dead share at depth 1 {share0:.4f}, at depth {depth} {share:.4f}; oracle segments {rs.segments}")
    assert share0 == 0.0, (name, share0)
    if dead_expected:
        assert share >= 0.01, (name, share)
    ds = world.device_scene()
    plain = _plain(torch, ds, cam, st)
    img, stats = ds.render(cam.desc, st)
    assert np.array_equal(img, want), name
    assert np.array_equal(plain, want), name
    assert (stats.segments, stats.samples) == (rs.segments, rs.samples), (name, stats.segments, rs.segments)
    assert np.array_equal(_plain(torch, ds, cam, st), want), (name, "plain after statistics")


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


@pytest.mark.parametrize("depth", [8, 50])
def test_rtiow_96x60(gpu, depth):
    """Depth 50: the frame's last iteration is the streaming finish (k_wfs_finish), which ends dead paths in its loop."""
    cam, world, _, _ = scenes.rtow_13_1(W, H)
    _check_scene(gpu, world, cam, _photo(cam), depth, f"rtiow depth {depth}")


def test_black_lambertian_ball(gpu):
    """A black Lambertian ball (and black small balls): its scatters zero the throughput by colour, whatever mult is,
    at the first hit of camera rays too (the camera launch's in-place shading)."""
    g = np.random.default_rng(31)
    black = Lambertian(Color(0.0, 0.0, 0.0, 1.0))
    extra = [Sphere((1.2, 0.8, 2.0), 0.8, black)] + [Sphere((-1.5 + 0.7 * k, 0.25, 3.0), 0.25, black) for k in range(4)]
    cam = _cam()
    _check_scene(gpu, _world(_field(g, extra=extra)), cam, _photo(cam, seed=3), 8, "black ball")


def test_diffuse_metal_ball(gpu):
    """DiffuseMetal balls (the heavy shading launch; a checker among them): light samples behind the reflected
    direction's hemisphere get mult == 0."""
    g = np.random.default_rng(32)
    extra = [Sphere((1.2, 0.8, 2.0), 0.8, DiffuseMetal(20.0, Color(0.8, 0.7, 0.3, 1.0))),
             Sphere((-1.6, 0.5, 2.6), 0.5, DiffuseMetal(4.0, Checker(Color(0.9, 0.9, 0.9, 1.0), Color(0.2, 0.3, 0.1, 1.0), 10.0)))]
    cam = _cam()
    _check_scene(gpu, _world(_field(g, extra=extra)), cam, _photo(cam, seed=4), 8, "diffuse metal")


def test_gate_false_ball_cutting_the_light(gpu):
    """A ball whose surface passes through the light's ball: the gate is false, the frame without statistics traces
    every path as before (and still equals the oracle's)."""
    g = np.random.default_rng(33)
    extra = [Sphere((30.0, 40.0, 13.0), 2.0, Lambertian(Color(0.6, 0.6, 0.2, 1.0)))]
    cam = _cam()
    _check_scene(gpu, _world(_field(g, extra=extra)), cam, _photo(cam, seed=6), 8, "ball cutting the light")


def test_masked_row_share(gpu, rtow):
    """Rows 1, 9, 17, ... with a checkered sample mask"""
    cam, world, ref = rtow
    rows = (1, 0, 8)
    yy, xx = np.indices((H, W))
    mask = (((xx // 3) + (yy // 2)) % 2 == 0).astype(np.uint8)
    photo = _photo(cam).rows(*rows)
    want, rs = ref(("mask", rows), photo, mask)
    sel = slice(rows[0], None, rows[2])
    ds = world.device_scene()
    assert np.array_equal(_plain(gpu, ds, cam, photo.settings(), mask)[sel], want[sel])
    img, stats = ds.render(cam.desc, photo.settings(), mask)
    assert np.array_equal(img[sel], want[sel])
    assert stats.segments == rs.segments
    assert np.array_equal(_plain(gpu, ds, cam, photo.settings(), mask)[sel], want[sel])


def test_pass_1_of_a_two_pass_stream(gpu, rtow):
    """Both passes of one sample stream, without and with statistics, equal the oracle's single passes."""
    torch = gpu
    cam, world, ref = rtow
    ds = world.device_scene()
    singles = [ref(("pass", k), _photo(cam).pass_index(k)) for k in range(2)]
    for with_stats in (False, True, False):
        outs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        stats = ds.render_device_passes(cam.desc, _photo(cam).settings(), [o.data_ptr() for o in outs],
                                        torch.cuda.current_stream().cuda_stream, stats=with_stats)
        torch.cuda.synchronize()
        for k in range(2):
            assert np.array_equal(outs[k].cpu().numpy(), singles[k][0]), (with_stats, k)
        if with_stats:
            assert stats.segments == singles[0][1].segments + singles[1][1].segments


def test_plain_statistics_plain(gpu, rtow):
    """A plain frame, a statistics frame and a plain frame on one device scene: three equal frames (the grids of each
    kind are sized from frames of its own kind)."""
    cam, world, ref = rtow
    photo = _photo(cam)
    want, rs = ref(("depth", 8), photo)
    ds = world.device_scene()
    a = _plain(gpu, ds, cam, photo.settings())
    b, stats = ds.render(cam.desc, photo.settings())
    c = _plain(gpu, ds, cam, photo.settings())
    assert np.array_equal(a, want) and np.array_equal(b, want) and np.array_equal(c, want)
    assert (stats.segments, stats.samples) == (rs.segments, rs.samples)
    # and through the slots again (three frame slots: the fourth plain frame reuses the first one's)
    for k in range(4):
        assert np.array_equal(_plain(gpu, ds, cam, photo.settings()), want), k
