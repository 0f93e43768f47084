"""Specular-chain feature buffers (rs_render_features_specular / _device) on the GPU against the CPU oracle, bit for
bit on all 8 channels of every rendered pixel: the features scene at several bounce budgets, one scene per tree kind,
the hall of mirrors, the eye inside a glass sphere, more than 64 samples, a Metal RayMarcher (against the library's
pinned World::hit probe), the scheduling invariances of the call, its argument checks and the layers above it.
Expected frames are built by tests/spec_features_ref.py from oracle calls alone; tests/test_spec_features_cpu.py
checks from the oracle alone that these fixtures reach every ending of a chain."""
import ctypes as C

import numpy as np
import pytest

import features_ref as F
import spec_features_ref as R
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-123.25)


def _assert_frames(got_a, got_n, exp_a, exp_n, where=None):
    """bitwise on every pixel of `where` (all when None), both frames; NaNs compare equal"""
    for name, got, exp in (("albedo", got_a, exp_a), ("normal", got_n, exp_n)):
        ok = F.same_bits(got, exp).all(axis=-1)
        if where is not None:
            ok = ok | ~where
        bad = np.argwhere(~ok)
        assert len(bad) == 0, (name, len(bad), [(int(y), int(x), got[y, x].tolist(), exp[y, x].tolist()) for y, x in bad[:3]])


def _expected(name, m):
    """(expected albedo, expected normal, the restatement's chains) of a fixture: computed once, read only"""
    ch = R.fixture_chains(name, m)
    return ch.frames() + (ch,)


@pytest.mark.parametrize("m", [0, 1, 4])
def test_features_scene(gpu, m):
    """48 x 30, N = 9, aperture 0.1, shutter 1.0: Metal, Dielectric and MixedMaterial(Metal, ..) spheres among every
    other way a hit gets its material. segments is the restatement's World::hit count; max_specular = 0 is also
    rs_render_features' own frame, through the first-hit kernel"""
    cam, world, photo, _, _, _ = R.fixture("features")
    exp_a, exp_n, ch = _expected("features", m)
    ds = world.device_scene()
    got_a, got_n, stats = ds.render_features(cam.desc, photo.settings(), max_specular=m)
    _assert_frames(got_a, got_n, exp_a, exp_n)
    assert stats.samples == 48 * 30 * 9 and stats.segments == int(ch.calls.sum())
    assert stats.kernel_id == 4 and stats.kernel_launches == 1  # RS_KERNEL_FEATURES
    if m == 0:
        own_a, own_n, _ = ds.render_features(cam.desc, photo.settings())
        a, n = np.zeros_like(own_a), np.zeros_like(own_n)  # (the new entry point itself, not the wrapper's shortcut)
        st = photo.settings()
        assert ds.lib.rs_render_features_specular(ds.handle, C.byref(cam.desc), C.byref(st), None, 0, a.ctypes.data,
                                                  n.ctypes.data, None) == 0
        assert F.same_bits(a, own_a).all() and F.same_bits(n, own_n).all() and F.same_bits(a, got_a).all()


@pytest.mark.parametrize("name", ["spheres", "mesh", "rich"])
def test_tree_kinds(gpu, name):
    """32 x 20, N = 4, max_specular 3: RTIOW 13.1 (the spheres-only 4-wide tree, mode 1: glass, hollow glass, metal), a
    Dielectric triangle mesh (flat mesh tree, mode 2) and the rich generic mode, where the chain through the glass
    sphere ends on the medium's Isotropic boundary hit at its key-0 distance"""
    cam, world, photo, _, _, _ = R.fixture(name)
    ds = world.device_scene()
    assert ds.info().scene_mode == R.FIXTURES[name][5]
    exp_a, exp_n, ch = _expected(name, 3)
    got_a, got_n, stats = ds.render_features(cam.desc, photo.settings(), max_specular=3)
    _assert_frames(got_a, got_n, exp_a, exp_n)
    assert stats.segments == int(ch.calls.sum())


@pytest.mark.parametrize("m", [1, 2, 16])
def test_hall_of_mirrors(gpu, m):
    """16 x 10, N = 4, the eye between two facing Metal rects: every sample runs to the limit, segments is exactly
    samples x (max_specular + 1), and the depth is the whole path's length"""
    cam, world, photo, _, _, _ = R.fixture("hall")
    exp_a, exp_n, ch = _expected("hall", m)
    assert (ch.ending == R.LIMIT).all()
    got_a, got_n, stats = world.device_scene().render_features(cam.desc, photo.settings(), max_specular=m)
    _assert_frames(got_a, got_n, exp_a, exp_n)
    assert stats.segments == 16 * 10 * 4 * (m + 1)
    assert (got_a[..., 3] == 1.0).all() and (got_n[..., 3] >= 2.0 + 5.0 * m).all()  # m + 1 legs


def test_inside_a_glass_sphere(gpu):
    """16 x 10, N = 4, max_specular 8, the eye off-centre inside glass: total internal reflection to the limit, chains
    that leave for the sky (escape: albedo = the tint, the last normal) and chains that end on the diffuse sphere"""
    cam, world, photo, _, _, _ = R.fixture("tir")
    exp_a, exp_n, ch = _expected("tir", 8)
    assert min(ch.count(R.LIMIT), ch.count(R.ESCAPE), ch.count(R.TERMINAL_AFTER)) > 0 and int(ch.tir.sum()) > 0
    got_a, got_n, stats = world.device_scene().render_features(cam.desc, photo.settings(), max_specular=8)
    _assert_frames(got_a, got_n, exp_a, exp_n)
    assert stats.segments == int(ch.calls.sum())


def test_more_than_64_samples(gpu):
    """the features scene at 8 x 5 with samples = 100: a pixel's samples span two chunks of the wave's reduction (64 +
    36) and the running carry; max_specular 2"""
    cam, world = scenes.features_scene(8, 5)
    photo = cam.take_photo().samples(100).seed(5).pass_index(1)
    orc, rec = R.oracle_scene(world)
    ch = R.chains(cam.desc, photo.settings(), F.oracle_hits(orc), F.Albedo(rec), 2)
    assert (ch.bounces >= 1).sum() > 40 and ch.count(R.MISS) > 0
    exp_a, exp_n = ch.frames()
    got_a, got_n, stats = world.device_scene().render_features(cam.desc, photo.settings(), max_specular=2)
    _assert_frames(got_a, got_n, exp_a, exp_n)
    assert stats.segments == int(ch.calls.sum())


def test_metal_raymarcher(gpu):
    """raymarching_test with a Metal Mandelbulb at 16 x 10, N = 1, max_specular 2, through the marcher unit's kernel.
    The oracle has no marcher: the hit records come from rs_probe_world_hit (pinned against tests/raymarch_ref.py by
    tests/test_gpu_raymarch.py), the bounces from the oracle's Metal as everywhere"""
    cam, world = R.marcher_metal(16, 10)
    photo = cam.take_photo().samples(1).seed(3).pass_index(0)
    ds, rec = F.device_scene(world)
    assert ds.info().scene_mode == 0 and ds.info().ref_order == 1
    ch = R.chains(cam.desc, photo.settings(), F.probe_hits(ds), F.Albedo(rec), 2)
    assert (ch.bounces >= 1).sum() >= 10, int((ch.bounces >= 1).sum())
    exp_a, exp_n = ch.frames()
    got_a, got_n, stats = ds.render_features(cam.desc, photo.settings(), max_specular=2)
    _assert_frames(got_a, got_n, exp_a, exp_n)
    assert stats.segments == int(ch.calls.sum())


def test_lattice_and_mask(gpu):
    """row_begin = 1, row_step = 3 and a checkerboard mask over sentinel-filled frames: masked pixels are zero in both
    frames, the other lattice pixels are the full frame's, rows off the lattice keep the caller's values"""
    W, H = 48, 30
    cam, world, photo, _, _, _ = R.fixture("features")
    exp_a, exp_n, ch = _expected("features", 4)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = ((xx + yy) % 2).astype(np.uint8)
    on_lattice = (yy >= 1) & ((yy - 1) % 3 == 0)
    a = np.full((H, W, 4), SENTINEL, np.float32)
    n = np.full((H, W, 4), SENTINEL, np.float32)
    st = photo.settings()
    st.row_begin, st.row_end, st.row_step = 1, 0, 3
    _, _, stats = world.device_scene().render_features(cam.desc, st, mask, albedo=a, normal=n, max_specular=4)
    for got in (a, n):
        assert (got[~on_lattice] == SENTINEL).all()
        assert (got[on_lattice & (mask == 0)] == 0.0).all()
    live = on_lattice & (mask == 1)
    _assert_frames(a, n, exp_a, exp_n, where=live)
    assert stats.samples == int(on_lattice[:, 0].sum()) * W * 9
    assert stats.segments == int(ch.calls.reshape(H, W, 9)[live].sum())  # masked pixels trace nothing


def test_three_virtual_devices(gpu):
    """devices = [0, 0, 0]: the row lattice split over three replicas and gathered, host and device call, bitwise the
    one-device frames"""
    torch = gpu
    W, H = 48, 30
    cam, world, photo, _, _, _ = R.fixture("features")
    exp_a, exp_n, ch = _expected("features", 4)
    ds3 = api.DeviceScene(world, devices=[0, 0, 0])
    assert ds3.info().n_devices == 3
    got_a, got_n, stats = ds3.render_features(cam.desc, photo.settings(), max_specular=4)
    _assert_frames(got_a, got_n, exp_a, exp_n)
    assert stats.segments == int(ch.calls.sum())
    ta = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    tn = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    ds3.render_features_device(cam.desc, photo.settings(), ta.data_ptr(), tn.data_ptr(),
                               torch.cuda.current_stream().cuda_stream, max_specular=4)
    _assert_frames(ta.cpu().numpy(), tn.cpu().numpy(), exp_a, exp_n)


def test_device_call_on_side_stream_between_guard_zones(gpu):
    """rs_render_features_specular_device on a non-default stream with stats = NULL (asynchronous), the two frames in
    the middle of one sentinel-filled allocation: after a stream sync the frames are the host call's and the guard
    zones before, between and after them are untouched; with one output NULL the other frame is the same and nothing
    else is written"""
    torch = gpu
    W, H = 48, 30
    cam, world, photo, _, _, _ = R.fixture("features")
    exp_a, exp_n, _ = _expected("features", 4)
    ds = world.device_scene()
    side = torch.cuda.Stream()
    n_f, guard = H * W * 4, 4096
    buf = torch.full((3 * guard + 2 * n_f,), float(SENTINEL), dtype=torch.float32, device="cuda")
    ta, tn = buf[guard:guard + n_f], buf[2 * guard + n_f:2 * guard + 2 * n_f]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert ds.render_features_device(cam.desc, photo.settings(), ta.data_ptr(), tn.data_ptr(), side.cuda_stream,
                                         stats=False, max_specular=4) is None
    side.synchronize()
    host = buf.cpu().numpy()
    _assert_frames(host[guard:guard + n_f].reshape(H, W, 4), host[2 * guard + n_f:2 * guard + 2 * n_f].reshape(H, W, 4),
                   exp_a, exp_n)
    for lo in (0, guard + n_f, 2 * guard + 2 * n_f):
        assert (host[lo:lo + guard] == SENTINEL).all()
    # albedo only, then normal only
    ua = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    un = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_features_device(cam.desc, photo.settings(), ua.data_ptr(), 0, side.cuda_stream, stats=False, max_specular=4)
    side.synchronize()
    assert torch.equal(ua.view(-1).view(torch.int32), ta.view(torch.int32)) and bool((un == float(SENTINEL)).all())
    ds.render_features_device(cam.desc, photo.settings(), 0, un.data_ptr(), side.cuda_stream, stats=False, max_specular=4)
    side.synchronize()
    assert torch.equal(un.view(-1).view(torch.int32), tn.view(torch.int32))
    assert torch.equal(ua.view(-1).view(torch.int32), ta.view(torch.int32))
    # the host call with one output
    only_a, none_n, _ = ds.render_features(cam.desc, photo.settings(), want=(True, False), max_specular=4)
    assert none_n is None and F.same_bits(only_a, exp_a).all()
    none_a, only_n, _ = ds.render_features(cam.desc, photo.settings(), want=(False, True), max_specular=4)
    assert none_a is None and F.same_bits(only_n, exp_n).all()


def test_invalid_arguments(gpu):
    """on a committed scene with a device: max_specular = 17 and both outputs NULL are RS_E_INVALID and write nothing;
    before commit a valid call is RS_E_STATE"""
    cam, world, photo, _, _, _ = R.fixture("hall")
    ds = world.device_scene()
    st = photo.settings()
    a = np.full((10, 16, 4), SENTINEL, np.float32)
    lib = ds.lib
    assert lib.rs_render_features_specular(ds.handle, C.byref(cam.desc), C.byref(st), None, 17, a.ctypes.data, None,
                                           None) == A.RS_E_INVALID
    assert lib.rs_render_features_specular(ds.handle, C.byref(cam.desc), C.byref(st), None, 2, None, None,
                                           None) == A.RS_E_INVALID
    assert lib.rs_render_features_specular_device(ds.handle, C.byref(cam.desc), C.byref(st), None, 17, None, None, None,
                                                  None) == A.RS_E_INVALID
    with pytest.raises(api.RaysnailError) as e:
        ds.render_features(cam.desc, st, max_specular=17)
    assert e.value.code == A.RS_E_INVALID
    assert (a == SENTINEL).all()
    fresh = C.c_void_p()
    assert lib.rs_scene_create(C.byref(fresh)) == 0
    assert lib.rs_render_features_specular(fresh, C.byref(cam.desc), C.byref(st), None, 2, a.ctypes.data, None,
                                           None) == A.RS_E_STATE
    lib.rs_scene_destroy(fresh)


def test_layers_above(gpu):
    """shot_features(max_specular=2) is the explicit call; shot_denoised(guide_specular=2) and
    shot_denoised_passes(.., guide_specular=2) are the compositions by hand over the chain guides, and with the default
    they are what they were: the compositions over the first-hit guides"""
    cam, world, _, _, _, _ = R.fixture("features")
    photo = cam.take_photo().samples(4).depth(4).seed(9).pass_index(1)
    ds = world.device_scene()
    a2, n2 = photo.shot_features(world, max_specular=2)
    assert photo.last_stats.segments > 48 * 30 * 4
    ea, en, _ = ds.render_features(cam.desc, photo.settings(), max_specular=2)
    assert F.same_bits(a2, ea).all() and F.same_bits(n2, en).all()
    a0, n0 = photo.shot_features(world)
    assert not F.same_bits(a0, a2).all()
    den2, beauty = photo.shot_denoised(world, guide_specular=2)
    assert F.same_bits(den2, api.denoise(beauty, a2, n2, None, photo._gamma)).all()
    den0, beauty0 = photo.shot_denoised(world)
    assert F.same_bits(beauty0, beauty).all()
    assert F.same_bits(den0, api.denoise(beauty, a0, n0, None, photo._gamma)).all()
    assert not F.same_bits(den0, den2).all()
    dv2, mean, var = photo.shot_denoised_passes(world, 2, guide_specular=2)
    assert F.same_bits(dv2, api.denoise_var(mean, var, a2, n2, None, photo._gamma)).all()
    dv0, mean0, var0 = photo.shot_denoised_passes(world, 2)
    assert F.same_bits(mean0, mean).all() and F.same_bits(dv0, api.denoise_var(mean, var, a0, n0, None, photo._gamma)).all()


def test_cpp_layer_on_the_gpu(gpu, tmp_path):
    """tests/cpp/test_spec_features_api.cpp in its `gpu` mode: shot_features(world, mask, 2) and shot_features(world,
    mask) of the C++ host layer (8 x 6, 4 samples, seed 3, pass 1, every other pixel masked) write the frames the
    Python layer renders of the same world"""
    import test_spec_features_cpp as T
    exe, frames = T.build(tmp_path), tmp_path / "frames.f32"
    import subprocess
    r = subprocess.run([str(exe), "gpu", str(frames)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
    got = np.fromfile(frames, np.float32).reshape(4, 6, 8, 4)
    h, lights = api.HittableList(), api.HittableList()
    sun = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    h.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Metal(api.Color(0.5, 0.75, 0.25))))
    h.add(api.Sphere((0.0, -101.0, 0.0), 100.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    h.add(sun)
    lights.add(sun)
    world = api.World(h, lights)
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(8).height(6).build()

    class EveryOther(api.PixelController):
        def calculate_pixel(self, x, y):
            return (x + y) % 2 == 0
    photo = cam.take_photo().samples(4).seed(3).pass_index(1)
    a2, n2 = photo.shot_features(world, EveryOther(), 2)
    a0, n0 = photo.shot_features(world, EveryOther())
    assert not F.same_bits(a0, a2).all()
    for k, exp in enumerate((a2, n2, a0, n0)):
        assert F.same_bits(got[k], exp).all(), k
