"""GPU parity: libraysnail_hip (gfx950) against the CPU oracle on the same seeded inputs.

North-star tolerance (BASELINE.json): per-pixel RMSE < 1e-4 against the reference semantics at a
fixed seed. The GPU path computes in f64 with the reference's operation order, so in practice the
frames are bit-identical; the tests assert the RMSE bound and, more strictly, >= 99.9 % bitwise
identical pixels (the remainder would be ocml-vs-glibc ulp differences in sin/cos/pow).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from raysnail_amd import _abi as A
from raysnail_amd import scenes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _oracle(world):
    from oracle.binding import OracleScene
    return OracleScene(world)


def _cmp(gpu_img, ref_img):
    g = gpu_img[..., :3].astype(np.float64)
    r = ref_img[..., :3].astype(np.float64)
    d = np.abs(g - r)
    rmse = float(np.sqrt(np.mean(d * d)))
    exact = float(np.mean(np.all(gpu_img == ref_img, axis=-1)))
    return rmse, exact, float(d.max())


def _load_make_golden():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


@pytest.mark.parametrize("name", ["rtow", "example_sdl", "quadric_sdl", "cornell", "rtow_depth50", "rtow_c1"])
def test_golden_frames(gpu, name):
    mg = _load_make_golden()
    build, spp, depth, seed = mg.FRAMES[name]
    cam, world = build()
    photo = cam.take_photo().samples(spp).depth(depth).seed(seed)
    img = photo.shot(None, world)
    ref = np.load(os.path.join(GOLDEN, "oracle_frames.npz"))[name]
    rmse, exact, mx = _cmp(img, ref)
    kat = json.load(open(os.path.join(GOLDEN, "kat.json")))
    assert photo.last_stats.segments == kat["frames"][name]["segments"]
    assert rmse < 1e-4 and exact >= 0.999, (name, rmse, exact, mx)


SCENES = {
    "rtow": lambda: scenes.rtow_13_1(96, 60)[:2],
    "example_sdl": lambda: scenes.example_sdl(96, 60),
    "quadric_sdl": lambda: scenes.quadric_sdl(80, 80),
    "cornell": lambda: scenes.cornell_box(64, 64),
    "cornell_axis_aligned": lambda: scenes.cornell_box(64, 64, rotated=False),
    "mesh": lambda: scenes.mesh_scene(96, 54, 24, 60),
    # §8(f)3: BlinnPhong, Perlin (all types / smoothings), Image (u, v), Isotropic media, Difference
    "materials": lambda: scenes.materials_scene(96, 64),
    "cornell_smoke": lambda: scenes.cornell_smoke(48, 48),
    "all_feature": lambda: scenes.all_feature_scene(48, 48, earth=scenes.synthetic_image()),
    "box_field": lambda: _box_field(64, 48),
}


def _box_field(w, h, n=400):
    """A reference-order scene with a deep tree: n random boxes, a translated quadric-box intersection
    and a Difference (non-monotone objects), a sphere light -- the in-order 4-wide tree's walk
    (collapse4_inorder) against the oracle's recursive BVH::hit."""
    from raysnail_amd.api import (Box, CameraBuilder, Color, Difference, DiffuseLight, Gradient, HittableList,
                                  Intersection, Lambertian, Metal, Point3, Sphere, World)
    C32 = Color
    rng = np.random.default_rng(3)
    hl = HittableList()
    for i in range(n):
        c = rng.uniform(-6, 6, 3) * np.array([1.0, 0.3, 1.0])
        e = rng.uniform(0.05, 0.6, 3)
        mat = Lambertian(C32(*rng.uniform(0.1, 0.9, 3))) if i % 3 else Metal(C32(0.8, 0.8, 0.8))
        hl.add(Box(tuple(c - e), tuple(c + e), mat))
    q = scenes._quad((1.0, -1.0, 1.0), (0, 0, 0), (0, 0, 0), 0.0)
    hl.add(scenes._translated(Intersection(q, Box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), None),
                                           Lambertian(C32(0.7, 0.8, 0.5))), (0.5, 1.5, 0.5)))
    hl.add(Difference(Box((-2.0, 2.0, -2.0), (-1.0, 3.0, -1.0), Lambertian(C32(0.4, 0.6, 0.8))),
                      Sphere((-1.5, 2.5, -1.5), 0.6, Lambertian(C32(0.9, 0.2, 0.2))), None))
    lights = HittableList()
    lamp = Sphere((0.0, 30.0, 10.0), 4.0, DiffuseLight(C32(1.0, 0.9, 0.8)).multiplier(4.0))
    lights.add(lamp)
    hl.add(lamp)
    cam = CameraBuilder().look_from(Point3(9.0, 4.0, 11.0)).look_at(Point3(0.0, 0.0, 0.0)).fov(50.0) \
        .width(w).height(h).build()
    return cam, World(hl, lights, Gradient(C32(0.3, 0.4, 0.5), C32(0.7, 0.89, 1.0)), (0.0, 0.0))


@pytest.mark.parametrize("mode", [A.RS_MODE_MEGAKERNEL, A.RS_MODE_WAVEFRONT])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_frames_match_oracle(gpu, name, mode):
    cam, world = SCENES[name]()
    photo = cam.take_photo().samples(16).depth(8).seed(11).mode(mode)
    img = photo.shot(None, world)
    ref, rstats = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    rmse, exact, mx = _cmp(img, ref)
    assert photo.last_stats.segments == rstats.segments
    assert rmse < 1e-4 and exact >= 0.999, (name, rmse, exact, mx)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_world_hit_random_rays(gpu, name):
    """World::hit records (t1, t2, point, normal, outside, material) on random rays, bit for bit."""
    cam, world = SCENES[name]()
    ds = world.device_scene()
    orc = _oracle(world)
    rng = np.random.default_rng(5)
    n = 4096
    eye = np.array(cam.desc.look_from[:])
    o = eye + rng.normal(0, 1.0, (n, 3))
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.ascontiguousarray(np.concatenate([o, d, np.zeros((n, 1))], 1))
    out = np.zeros((n, 13))
    assert ds.lib.rs_probe_world_hit(ds.handle, rays.ctypes.data, n, 1e-4, float("inf"), out.ctypes.data) == 0
    bad = 0
    for i in range(n):
        r = np.array(orc.world_hit(o[i], d[i]))
        g = out[i]
        same = r[0] == g[0] and (r[0] == 0 or (np.array_equal(r[1:13], g[1:13])))
        bad += 0 if same else 1
    assert bad == 0, f"{bad}/{n} world-hit mismatches"


@pytest.mark.parametrize("mode", [A.RS_MODE_MEGAKERNEL, A.RS_MODE_WAVEFRONT])
def test_determinism_batching_and_rows(gpu, monkeypatch, mode):
    cam, world, _, _ = scenes.rtow_13_1(120, 75)
    photo = cam.take_photo().samples(9).depth(8).seed(3).mode(mode)
    a = photo.shot(None, world)
    b = photo.shot(None, world)
    assert np.array_equal(a, b)
    # tiny batches: samples split over many launches, accumulated in sample order
    cam2, world2, _, _ = scenes.rtow_13_1(120, 75)
    world2.device_scene().set_workspace(max_batch_items=5000)
    c = cam2.take_photo().samples(9).depth(8).seed(3).mode(mode).shot(None, world2)
    assert np.array_equal(a, c)
    # tiny path sets: many chunks per batch (bounce-synchronous) / a small streaming pool with many
    # injections per batch
    cam3, world3, _, _ = scenes.rtow_13_1(120, 75)
    world3.device_scene().set_workspace(pool_paths=3000)
    d = cam3.take_photo().samples(9).depth(8).seed(3).mode(mode).shot(None, world3)
    assert np.array_equal(a, d)
    # rows interleaved over 3 "ranks" into one buffer == full frame (painter.rs:248)
    ds = world.device_scene()
    out = np.zeros_like(a)
    for r in range(3):
        st = photo.rows(r, 0, 3).settings()
        ds.render(cam.desc, st, out=out)
    assert np.array_equal(a, out)


def test_camera_order_plane_groups(gpu):
    """gen_perm (rs_kernels.hip): a wave traces 32 samples of each of 2 pixels, a batch's sample planes cut into
    groups of 32 and then of decreasing powers of two (49 planes: 32 + 16 + 1). Pure scheduling: the frame equals
    the one rendered one plane per batch (single-plane groups, the old one-plane-per-wave order), and a row share at
    N = 8 (2 x 1 pixel tiles) renders its rows as the full frame does."""
    cam, world, _, _ = scenes.rtow_13_1(72, 45)
    photo = cam.take_photo().samples(49).depth(8).seed(5)
    a = photo.shot(None, world)
    cam2, world2, _, _ = scenes.rtow_13_1(72, 45)
    world2.device_scene().set_workspace(max_batch_items=72 * 45)
    b = cam2.take_photo().samples(49).depth(8).seed(5).shot(None, world2)
    assert np.array_equal(a, b)
    ds = world.device_scene()
    out = np.zeros_like(a)
    ds.render(cam.desc, photo.rows(1, 0, 8).settings(), out=out)
    assert np.array_equal(a[1::8], out[1::8])
    ref, _ = _oracle(world).render(cam.desc, photo.rows(0, 0, 9).settings())
    rmse, exact, mx = _cmp(a[0::9], ref[0::9])
    assert rmse < 1e-4 and exact >= 0.999, (rmse, exact, mx)


def test_pixel_mask_and_untouched_rows(gpu):
    """painter.rs:204-210: pixels the PixelController rejects come back [0,0,0,0]."""
    cam, world = scenes.example_sdl(64, 40)
    photo = cam.take_photo().samples(4).depth(8).seed(2)
    full = photo.shot(None, world)
    mask = (np.indices((40, 64)).sum(0) % 3 != 0).astype(np.uint8)
    out, _ = world.device_scene().render(cam.desc, photo.settings(), mask)
    assert np.all(out[mask == 0] == 0.0)
    assert np.array_equal(out[mask == 1], full[mask == 1])
    ref, _ = _oracle(world).render(cam.desc, photo.settings(), threads=8, mask=mask)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("name", ["mesh", "mesh_metal", "smoke"])
def test_pixel_mask_bounce_synchronous(gpu, name):
    """The bounce-synchronous wavefront (a flat mesh scene -- Lambertian only, k_wf_shade<kSmFlat, true>, or
    with Metal / Dielectric spheres, the generic shading -- and a rich media scene) under a pixel mask:
    k_wf_gen compacts the live samples into set 0's shards (rs_kernels.hip Segs); masked pixels come back 0,
    the frame equals the oracle's and the unmasked pixels the maskless frame's."""
    if name.startswith("mesh"):
        cam, world = scenes.mesh_scene(48, 32, n_theta=20, n_phi=40)
        if name == "mesh_metal":
            from raysnail_amd.api import Color, Dielectric, Glass, Metal, Sphere
            world.hittables.add(Sphere((1.4, 0.6, 0.3), 0.5, Metal(Color(0.7, 0.6, 0.5, 1.0))))
            world.hittables.add(Sphere((-1.3, 0.5, 0.8), 0.45, Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass())))
    else:
        cam, world = scenes.cornell_smoke(48, 32)
    photo = cam.take_photo().samples(4).depth(8).seed(5)
    full = photo.shot(None, world)
    mask = (np.indices((32, 48)).sum(0) % 5 != 0).astype(np.uint8)
    out, _ = world.device_scene().render(cam.desc, photo.settings(), mask)
    assert np.all(out[mask == 0] == 0.0)
    assert np.array_equal(out[mask == 1], full[mask == 1])
    ref, _ = _oracle(world).render(cam.desc, photo.settings(), threads=8, mask=mask)
    assert np.array_equal(out, ref)


def test_streaming_moving_sphere_records(gpu):
    """A spheres-only scene with a moving sphere and a nonzero shutter runs the streaming wavefront with the
    path's time in its record (WfState::tagw = 0: the (item, level) tag in its own array) and every sphere's
    centre at the ray's time (sphere.rs center_at); the frame equals the oracle's. Its static twin (no speed)
    carries the tag in ray_o.w and must differ only where the moving sphere is seen."""
    from raysnail_amd.api import CameraBuilder, Color, Dielectric, DiffuseLight, Glass, Gradient, HittableList, \
        Lambertian, Metal, Point3, Sphere, World
    frames = []
    for speed in ((0.6, 0.0, 0.2), None):
        h, lights = HittableList(), HittableList()
        h.add(Sphere((0.0, -1000.0, 0.0), 1000.0, Lambertian(Color(0.5, 0.5, 0.5, 1.0))))
        s = Sphere((0.0, 1.0, 0.0), 1.0, Lambertian(Color(0.7, 0.3, 0.2, 1.0)))
        h.add(s.with_speed(speed) if speed else s)
        h.add(Sphere((2.2, 0.8, 0.5), 0.8, Metal(Color(0.7, 0.6, 0.5, 1.0))))
        h.add(Sphere((-2.0, 0.7, 0.3), 0.7, Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass())))
        light = Sphere((0.0, 6.0, 2.0), 1.0, DiffuseLight(Color(1.0, 0.9, 0.8, 1.0)).multiplier(4.0))
        h.add(light)
        lights.add(light)
        cam = CameraBuilder().look_from(Point3(0.0, 2.0, 8.0)).look_at(Point3(0.0, 1.0, 0.0)).fov(35.0) \
            .shutter_speed(1.0).width(64).height(40).build()
        world = World(h, lights, Gradient(Color(0.3, 0.4, 0.5, 1.0), Color(0.7, 0.89, 1.0, 1.0)), (0.0, 1.0))
        photo = cam.take_photo().samples(9).depth(12).seed(3)
        img = photo.shot(None, world)
        ref, _ = _oracle(world).render(cam.desc, photo.settings(), threads=8)
        assert np.array_equal(img, ref)
        frames.append(img)
    assert not np.array_equal(frames[0], frames[1])


def test_deep_paths_depth50(gpu):
    """Depth-50 recursion (configs 2-5): wavefront keeps bouncing until every queue drains."""
    for build in (lambda: scenes.rtow_13_1(40, 25)[:2], lambda: scenes.cornell_box(32, 32)):
        cam, world = build()
        photo = cam.take_photo().samples(4).depth(50).seed(8)
        img = photo.shot(None, world)
        ref, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
        assert photo.last_stats.segments == rs.segments
        assert np.array_equal(img, ref)


def test_samples_rule_and_zero_samples(gpu):
    """painter.rs:110-118: N = floor(sqrt(requested))^2; N = 0 gives NaN (0/0) like the reference."""
    cam, world = scenes.example_sdl(32, 20)
    p5 = cam.take_photo().samples(5).depth(4).seed(1)
    p4 = cam.take_photo().samples(4).depth(4).seed(1)
    assert np.array_equal(p5.shot(None, world), p4.shot(None, world))
    z = cam.take_photo().samples(0).depth(4).seed(1).shot(None, world)
    assert np.isnan(z[..., :3]).all() and (z[..., 3] == 1.0).all()


def test_render_device_into_torch(gpu):
    torch = gpu
    cam, world, _, _ = scenes.rtow_13_1(64, 40)
    photo = cam.take_photo().samples(4).depth(8).seed(9)
    host = photo.shot(None, world)
    t = torch.zeros((40, 64, 4), dtype=torch.float32, device="cuda")
    st = world.device_scene().render_device(cam.desc, photo.settings(), t.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    assert st.launches >= 1 and st.path_ms > 0
    assert np.array_equal(t.cpu().numpy(), host)


def test_bench_config_rows_match_oracle(gpu):
    """Full bench size (800x500, 64 spp, depth 8): the oracle re-renders every 50th row and those
    rows must match; size-independent properties on the whole frame; both GPU modes agree bitwise."""
    cam, world, _, _ = scenes.rtow_13_1(800, 500)
    photo = cam.take_photo().samples(64).depth(8).seed(1)
    img = photo.shot(None, world)
    mega = cam.take_photo().samples(64).depth(8).seed(1).mode(A.RS_MODE_MEGAKERNEL).shot(None, world)
    assert np.array_equal(img, mega)
    assert np.isfinite(img).all() and (img[..., 3] == 1.0).all()
    assert photo.last_stats.samples == 800 * 500 * 64
    st = photo.rows(0, 0, 50).settings()
    ref, _ = _oracle(world).render(cam.desc, st, threads=16)
    rmse, exact, mx = _cmp(img[::50], ref[::50])
    assert rmse < 1e-4 and exact >= 0.999, (rmse, exact, mx)


def test_passes_combine_like_cli(gpu):
    """raysnail.rs:379-427 passes folded with combine_pixel: GPU passes via render_sharded on one
    device (virtual ranks) == oracle passes folded in numpy."""
    torch = gpu
    from raysnail_amd.distributed import combine_pixels
    cam, world = scenes.example_sdl(48, 30)
    photo = cam.take_photo().samples(4).depth(8).seed(4)
    ds = world.device_scene()
    orc = _oracle(world)
    acc_t = torch.zeros((30, 48, 4), dtype=torch.float32, device="cuda")
    acc_t[..., 3] = 1
    acc_n = np.zeros((30, 48, 4), np.float32)
    acc_n[..., 3] = 1
    for p in range(3):
        st = photo.pass_index(p).settings()
        g, _ = ds.render(cam.desc, st)
        r, _ = orc.render(cam.desc, st, threads=8)
        assert np.array_equal(g, r)
        acc_t = combine_pixels(acc_t, torch.from_numpy(g).cuda(), float(p))
        acc_n = (acc_n * np.float32(p) + r) / np.float32(p + 1)
    assert np.allclose(acc_t.cpu().numpy(), acc_n, rtol=0, atol=1e-6)


def test_obj_mesh_scene_matches_oracle(gpu, tmp_path):
    """§8(f)4: TriangleMesh::load (OBJ, quads triangulated, averaged vertex normals) rendered on
    the GPU against the oracle fed the same triangles."""
    from raysnail_amd import api
    lines = []
    n = 24
    for i in range(n + 1):  # a bumpy height field of quads
        for j in range(n + 1):
            x, z = i / n * 2 - 1, j / n * 2 - 1
            lines.append(f"v {x:.6f} {0.3 * np.sin(3 * x) * np.cos(2 * z) + 0.5:.6f} {z:.6f}")
    for i in range(n):
        for j in range(n):
            a = i * (n + 1) + j + 1
            lines.append(f"f {a} {a + 1} {a + n + 2} {a + n + 1}")
    path = tmp_path / "field.obj"
    path.write_text("\n".join(lines) + "\n")
    mesh = api.TriangleMesh.load(str(path), 1.5, (0.0, 0.0, 0.0), 30.0, 1, api.Lambertian(api.Color(0.8, 0.6, 0.4)))
    assert mesh.positions.shape == (2 * n * n, 9)
    h = api.HittableList().add(mesh).add(api.Sphere((0, -1000, 0), 1000.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    light = api.Sphere((30, 40, 10), 5.0, api.DiffuseLight(api.Color(1, 0.9, 0.7)).multiplier(3.0))
    h.add(light)
    world = api.World(h, api.HittableList().add(light))
    cam = api.CameraBuilder().look_from((0, 2.5, 4)).look_at((0, 0.5, 0)).fov(40).width(64).height(48).build()
    photo = cam.take_photo().samples(16).depth(8).seed(5)
    img = photo.shot(None, world)
    ref, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    assert photo.last_stats.segments == rs.segments
    assert np.array_equal(img, ref)


def test_rich_scene_deep_paths_and_batching(gpu, monkeypatch):
    """Media / Perlin / Image scenes at depth 50 with tiny wavefront chunks: still bit-identical."""
    cam, world = scenes.materials_scene(40, 28)
    world.device_scene().set_workspace(pool_paths=2000)
    photo = cam.take_photo().samples(9).depth(50).seed(12)
    img = photo.shot(None, world)
    ref, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    assert photo.last_stats.segments == rs.segments
    assert np.array_equal(img, ref)


@pytest.mark.parametrize("name", ["rtow", "cornell", "quadric_sdl", "mesh"])
def test_per_sample_radiance_vs_oracle(gpu, name):
    """Per-sample f64 radiance (rs_probe_samples, the GPU's forward form of ray_color) against the
    oracle's recursion (orc_sample_radiance, camera.rs:156-255) for every sample of a few pixels.

    The forward form multiplies the throughput level by level, T = (c * (lm * T)) * mult, where the
    recursion nests the same factors the other way round, so the f64 products may differ in their
    last bits. Stated tolerance: |gpu - oracle| <= 2^-40 * max(|oracle|, 1) per channel (far below
    one f32 ulp of a pixel); world.hit counts must be equal (same path, same decisions)."""
    cam, world = SCENES[name]()
    photo = cam.take_photo().samples(64).depth(50).seed(13)
    st = photo.settings()
    ds = world.device_scene()
    orc = _oracle(world)
    W, H = cam.desc.width, cam.desc.height
    n = 64
    exact = total = 0
    worst = 0.0
    for (x, y) in [(W // 2, H // 2), (W // 5, H // 3), (W - 3, H - 2), (2, 1)]:
        g = np.zeros((n, 4))
        assert ds.lib.rs_probe_samples(ds.handle, C.byref(cam.desc), C.byref(st), x, y, 0, n,
                                       g.ctypes.data) == 0, ds.lib.rs_last_error()
        for s in range(n):
            o, seg = orc.sample_radiance(cam.desc, st, x, y, s)
            assert g[s, 3] == seg, (x, y, s, g[s, 3], seg)
            fin = np.isfinite(o)
            assert np.array_equal(np.isfinite(g[s, :3]), fin), (x, y, s, g[s, :3], o)
            d = np.abs(g[s, :3][fin] - o[fin]) / np.maximum(np.abs(o[fin]), 1.0)
            worst = max(worst, float(d.max()) if d.size else 0.0)
            exact += int(np.array_equal(g[s, :3][fin], o[fin]))
            total += 1
    print(f"{name}: {exact}/{total} samples bit-identical, worst relative difference {worst:.3e}")
    assert worst <= 2.0 ** -40, worst


@pytest.mark.parametrize("name", ["rtow", "example_sdl", "quadric_sdl"])
def test_streaming_pool_and_async_bit_identical(gpu, name):
    """Scheduling only. The streaming wavefront (spheres / nest-0 / nest-2 scenes: a pool of paths in
    flight, camera samples injected per iteration as paths finish) with pools from 20 iterations'
    worth down to 256 samples per iteration and radiance batches of 1-2 sample planes (several
    batches in the ring, accumulated while later samples are still traced); chunk lanes; 1-4 frames in
    flight with asynchronous rs_render_device frames overlapping on one stream -- two frame settings
    alternating into two buffers, and the row shares r::4 of one frame (a strong-scaled rank's work)
    into one buffer. Every frame equals the oracle's bit for bit, with the oracle's world.hit count."""
    import torch
    build = {"rtow": lambda: scenes.rtow_13_1(96, 60)[:2], "example_sdl": lambda: scenes.example_sdl(96, 60),
             "quadric_sdl": lambda: scenes.quadric_sdl(96, 60)}[name]
    cam, world = build()
    ds = world.device_scene()
    st = cam.take_photo().samples(16).depth(12).seed(5).settings()
    st2 = cam.take_photo().samples(9).depth(7).seed(6).settings()
    orc = _oracle(world)
    ref, rstats = orc.render(cam.desc, st)
    ref2, _ = orc.render(cam.desc, st2)
    npx = 96 * 60
    for batch, pool in ((32 << 20, 16 << 20), (32 << 20, 20000), (2 * npx, 5000), (npx, 256 * 12)):
        ds.set_workspace(batch, pool)
        for lanes in (1, 2):
            ds.set_lanes(lanes)
            img, stats = ds.render(cam.desc, st)
            assert stats.segments == rstats.segments, (batch, pool, lanes)
            assert np.array_equal(img, ref), (batch, pool, lanes)
    ds.set_workspace(32 << 20, 16 << 20)
    s = torch.cuda.current_stream().cuda_stream
    for frames in (1, 2, 3, 4):
        ds.set_frames_in_flight(frames)
        outs = [torch.full((60, 96, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        for k in range(6):  # two settings alternating, asynchronous, back to back on one stream
            assert ds.render_device(cam.desc, st if k % 2 == 0 else st2, outs[k % 2].data_ptr(), s, stats=False) is None
        torch.cuda.synchronize()
        assert np.array_equal(outs[0].cpu().numpy(), ref), frames
        assert np.array_equal(outs[1].cpu().numpy(), ref2), frames
        share = torch.zeros((60, 96, 4), dtype=torch.float32, device="cuda")
        for r in range(4):  # the row shares of N = 4 ranks, overlapping, into one frame
            sh = cam.take_photo().samples(16).depth(12).seed(5).rows(r, 0, 4).settings()
            ds.render_device(cam.desc, sh, share.data_ptr(), s, stats=False)
        torch.cuda.synchronize()
        assert np.array_equal(share.cpu().numpy(), ref), frames
        # the two settings on two streams at once: a slot is reused only after its previous frame
        # (whatever stream it ran on), and each frame orders itself after its caller's stream
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        for o in outs:
            o.fill_(-1.0)
        sa.wait_stream(torch.cuda.current_stream())
        sb.wait_stream(torch.cuda.current_stream())
        for k in range(4):
            ds.render_device(cam.desc, st if k % 2 == 0 else st2, outs[k % 2].data_ptr(),
                             (sa if k % 2 == 0 else sb).cuda_stream, stats=False)
        torch.cuda.synchronize()
        assert np.array_equal(outs[0].cpu().numpy(), ref), frames
        assert np.array_equal(outs[1].cpu().numpy(), ref2), frames
    ds.set_frames_in_flight(2)


def test_queue_counter_reset_across_frames(gpu):
    """The last accumulate of an asynchronous frame zeroes the frame's queue counters for the next
    one (no memset, rs_host.cpp counts_clean); frames with statistics keep them for the readback and
    the next frame zeroes them itself. Mixed sequences -- asynchronous, with statistics, a row share
    (fewer counters), the full frame again, a longer depth (more counters) -- must each give the
    oracle's frame and, with statistics, its world.hit count."""
    import torch
    cam, world = scenes.rtow_13_1(96, 60)[:2]
    ds = world.device_scene()
    s = torch.cuda.current_stream().cuda_stream
    out = torch.zeros((60, 96, 4), dtype=torch.float32, device="cuda")
    orc = _oracle(world)
    cases = {}
    for key, photo in (("d8", cam.take_photo().samples(16).depth(8).seed(5)),
                       ("d8_share", cam.take_photo().samples(16).depth(8).seed(5).rows(0, 0, 4)),
                       ("d20", cam.take_photo().samples(16).depth(20).seed(5))):
        st = photo.settings()
        ref, rstats = orc.render(cam.desc, st)
        cases[key] = (st, ref, rstats)
    for key, with_stats in (("d8", False), ("d8", False), ("d8", True), ("d8_share", False), ("d8", False),
                            ("d20", False), ("d20", True), ("d8", False), ("d8_share", True), ("d8", False)):
        st, ref, rstats = cases[key]
        out.zero_()
        stats = ds.render_device(cam.desc, st, out.data_ptr(), s, stats=with_stats)
        torch.cuda.synchronize()
        img = out.cpu().numpy()
        if key == "d8_share":
            assert np.array_equal(img[0::4], ref[0::4]), key
        else:
            assert np.array_equal(img, ref), key
        if with_stats:
            assert stats.segments == rstats.segments, (key, stats.segments, rstats.segments)


def _emissive_csg_scene(w=80, h=60):
    """Composite prims whose records carry a DiffuseLight (an Intersection with the light on the
    CSG, a TfFacade of it) next to Lambertian CSG: the material-sorted wavefront must emit for them
    (camera.rs:172-176, 250) from the generic class 4, which every composite prim gets -- Lambertian-only
    CSG included (its records take the material through set_material_if_none, hit.rs:69-78)."""
    from raysnail_amd.api import (Box, CameraBuilder, DiffuseLight, Gradient, HittableList, Intersection,
                                  Lambertian, Sphere, TfFacade, Transform, TransformStack, World)
    from raysnail_amd.scenes import C32
    hl, lights = HittableList(), HittableList()
    lamp = DiffuseLight(C32(1.0, 0.9, 0.7)).multiplier(4.0)
    glow = Intersection(Sphere((0.0, 0.0, 0.0), 1.0, None), Box((-0.7, -0.7, -0.7), (0.7, 0.7, 0.7), None), lamp)
    st = TransformStack()
    st.push(Transform.translate((0.0, 2.5, 0.0)))
    lit = TfFacade(glow, st)
    hl.add(lit)
    lights.add(lit)
    lam = Lambertian(C32(0.7, 0.6, 0.5))
    st2 = TransformStack()
    st2.push(Transform.translate((1.5, 0.0, 0.0)))
    hl.add(TfFacade(Intersection(Sphere((0.0, 0.0, 0.0), 1.0, None), Box((-0.8, -0.8, -0.8), (0.8, 0.8, 0.8), None), lam), st2))
    # one child with its own (light) material, one with none: mixed classes -> generic
    hl.add(Intersection(Sphere((-1.5, 0.0, 0.0), 1.0, DiffuseLight(C32(0.2, 0.4, 0.9))),
                        Box((-2.3, -0.8, -0.8), (-0.7, 0.8, 0.8), None), lam))
    hl.add(Sphere((0.0, -1001.0, 0.0), 1000.0, Lambertian(C32(0.5, 0.5, 0.5))))
    world = World(hl, lights, Gradient(C32(0.05, 0.05, 0.1), C32(0.1, 0.1, 0.2)), (0.0, 0.0))
    cam = CameraBuilder().look_from((0.0, 2.0, 9.0)).look_at((0.0, 0.5, 0.0)).fov(40.0).width(w).height(h).build()
    return cam, world


def test_emissive_and_lambertian_csg_classes(gpu):
    cam, world = _emissive_csg_scene()
    photo = cam.take_photo().samples(16).depth(10).seed(7)
    img = photo.shot(None, world)
    info = world.device_scene().info()
    assert info.scene_mode in (3, 4)  # a nest mode: the material-sorted wavefront
    ref, rs = _oracle(world).render(cam.desc, photo.settings())
    assert photo.last_stats.segments == rs.segments
    assert np.array_equal(img, ref)
    assert img[..., :3].max() > 1.0  # the lamp is seen directly


@pytest.mark.parametrize("frames", [1, 2, 3])
def test_render_rows_progressive(gpu, frames):
    """rs_render_rows (Painter::draw + PainterTarget::register_pixels, painter.rs:214, 332): every lattice
    row once, in lattice order, its pixels final when reported, then the (H) sentinel; the frame equals
    the one-call frame bitwise -- with 1-3 bands in flight, a strided lattice and a pixel mask."""
    cam, world = scenes.example_sdl(160, 100)
    ds = world.device_scene()
    ds.set_frames_in_flight(frames)
    photo = cam.take_photo().samples(9).depth(8).seed(2)
    ref, _ = ds.render(cam.desc, photo.settings())
    for lattice, mask in (((0, 0, 1), None), ((1, 0, 3), (np.arange(160 * 100).reshape(100, 160) % 7 != 0))):
        st = photo.rows(*lattice).settings()
        one, _ = ds.render(cam.desc, st, mask)
        seen = []

        def on_row(y, out):
            seen.append(y)
            if y < 100:
                assert np.array_equal(out[y], one[y]), y
        for stats in (False, True):
            seen.clear()
            img, _ = ds.render_rows(cam.desc, st, on_row, mask, bands=7, stats=stats)
            assert seen == list(range(lattice[0], 100, lattice[2])) + [100]
            assert np.array_equal(img[lattice[0]::lattice[2]], one[lattice[0]::lattice[2]])
    ds.set_frames_in_flight(2)


def test_render_rows_stats_on_spilling_mesh(gpu):
    """rs_render_rows with statistics on a tree whose traversal stack spills to HBM (one frame slot per replica):
    every band's counters are its own (a band is not enqueued into a slot whose previous band's counters are still
    to be read), so the summed segments and samples equal rs_render's for the same frame, and the frame is the same."""
    cam, world = scenes.mesh_scene(96, 54)
    ds = world.device_scene()
    inf = ds.info()
    assert inf.stack_need > inf.stack_lds, (inf.stack_need, inf.stack_lds)  # the spilling case
    ds.set_frames_in_flight(2)
    st = cam.take_photo().samples(4).depth(8).seed(3).settings()
    ref, rst = ds.render(cam.desc, st)
    rows = []
    img, bst = ds.render_rows(cam.desc, st, lambda y, out: rows.append(y), None, bands=5, stats=True)
    assert rows == list(range(54)) + [54]
    assert np.array_equal(img, ref)
    assert (bst.samples, bst.segments) == (rst.samples, rst.segments)
    assert bst.kernel_bytes == rst.kernel_bytes


def test_deep_spheres_stack_spill_matches_oracle(gpu):
    """A spheres-mode scene whose 4-wide tree needs a 22-entry traversal stack (40k spheres): the entries past
    the LDS part spill to the HBM overflow array, the replica runs one frame slot, and the frame still equals
    the oracle's bit for bit with the same world.hit count."""
    cam, world = scenes.deep_spheres(48, 32, 40000)
    ds = world.device_scene()
    info = ds.info()
    assert info.scene_mode == 1 and info.stack_need > info.stack_lds
    st = cam.take_photo().samples(9).depth(8).seed(3).settings()
    img, stats = ds.render(cam.desc, st)
    ref, rs = _oracle(world).render(cam.desc, st)
    assert stats.segments == rs.segments
    assert np.array_equal(img, ref)


def _leaf_row_scene(w=32, h=20):
    """Twelve leaf objects (boxes, which make the scene reference-order, and spheres off the axis) in a row along
    the view axis, growing with distance, and a sphere light above: the central rays reach every object's box,
    the outer ones only the far boxes."""
    from raysnail_amd.api import (Box, CameraBuilder, DiffuseLight, Gradient, HittableList, Lambertian, Metal,
                                  Sphere, World)
    from raysnail_amd.scenes import C32
    hl, lights = HittableList(), HittableList()
    for i in range(12):
        z = -1.5 * i
        mat = Lambertian(C32(0.2 + 0.06 * i, 0.7 - 0.04 * i, 0.5)) if i % 2 else Metal(C32(0.8, 0.8, 0.7))
        if i % 3 == 2:
            hl.add(Sphere((0.15 * ((i % 4) - 1.5), 0.1 * (i % 3), z), 0.45 + 0.02 * i, mat))
        else:
            hl.add(Box((-0.4 - 0.03 * i, -0.4, z - 0.3), (0.4 + 0.03 * i, 0.4 + 0.02 * i, z + 0.3), mat))
    lamp = Sphere((0.0, 6.0, -8.0), 2.0, DiffuseLight(C32(1.0, 0.9, 0.8)).multiplier(4.0))
    lights.add(lamp)
    hl.add(lamp)
    world = World(hl, lights, Gradient(C32(0.3, 0.4, 0.5), C32(0.7, 0.89, 1.0)), (0.0, 0.0))
    cam = CameraBuilder().look_from((0.05, 0.1, 6.0)).look_at((0.0, 0.0, -8.0)).fov(20.0).width(w).height(h).build()
    return cam, world


def test_deferred_walk_second_window_matches_oracle(gpu):
    """A nest-0 reference-order scene with its LDS image whose central rays reach more than kLeafBatch (8) leaf
    boxes: the deferred walk (rs_kernels.hip traverse_deferred) lists its leaves in two windows, walking the tree
    again for the second. The frame equals the oracle's bit for bit."""
    cam, world = _leaf_row_scene()
    info = world.device_scene().info()
    assert info.scene_mode == 3  # nest-0
    assert info.ref_order == 1 and info.tree_arity == 4
    assert info.stack_need + 8 <= info.stack_lds  # the condition for the scene's LDS image (build_limg)
    photo = cam.take_photo().samples(4).depth(4).seed(5).mode(A.RS_MODE_WAVEFRONT)
    img = photo.shot(None, world)
    ref, rs = _oracle(world).render(cam.desc, photo.settings())
    assert photo.last_stats.segments == rs.segments
    assert np.array_equal(img, ref)


@pytest.mark.parametrize("name", ["rtow", "example_sdl", "quadric_sdl", "mesh"])
def test_render_device_passes_stream(gpu, name):
    """rs_render_device_passes: n progressive passes of one frame (raysnail.rs:379-427's pass loop) as one sample
    stream -- pass k + 1's camera samples enter the pool while pass k's paths drain -- equal, frame by frame, the
    passes rendered one call each, and pass 0 equals the oracle's. Pools from whole passes down to 256 samples per
    iteration and radiance batches of 1-16 sample planes (a pass is several batches; several passes' batches in the
    ring at once), one and two lanes, repeated output pointers, a row share (rows 1::4), and the statistics summed
    over the passes. `mesh` (bounce-synchronous) takes the one-call-per-pass fallback."""
    torch = gpu
    build = {"rtow": lambda: scenes.rtow_13_1(64, 40)[:2], "example_sdl": lambda: scenes.example_sdl(64, 40),
             "quadric_sdl": lambda: scenes.quadric_sdl(48, 48), "mesh": lambda: scenes.mesh_scene(64, 36, 24, 60)}[name]
    cam, world = build()
    H, W = cam.desc.height, cam.desc.width
    ds = world.device_scene()
    s = torch.cuda.current_stream().cuda_stream
    n = 5
    for rows in ((0, 0, 1), (1, 0, 4)):
        photo = cam.take_photo().samples(16).depth(10).seed(8).pass_index(3).rows(*rows)
        st = photo.settings()
        singles = []
        one_stats = []
        for k in range(n):
            o = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda")
            one_stats.append(ds.render_device(cam.desc, cam.take_photo().samples(16).depth(10).seed(8)
                                              .pass_index(3 + k).rows(*rows).settings(), o.data_ptr(), s))
            singles.append(o.cpu().numpy())
        if rows == (0, 0, 1):
            ref, rs = _oracle(world).render(cam.desc, st, threads=16)
            assert np.array_equal(singles[0], ref)
        npx = W * len(range(rows[0], H, rows[2]))
        for batch, pool in ((32 << 20, 16 << 20), (npx, 256 * 10), (4 * npx, 7000), (16 * npx, 3 * 16 * npx)):
            ds.set_workspace(batch, pool)
            for lanes in (1, 2):
                ds.set_lanes(lanes)
                outs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(n)]
                stats = ds.render_device_passes(cam.desc, st, [o.data_ptr() for o in outs], s)
                for k in range(n):
                    assert np.array_equal(outs[k].cpu().numpy(), singles[k]), (name, rows, batch, pool, lanes, k)
                assert stats.samples == sum(x.samples for x in one_stats)
                assert stats.segments == sum(x.segments for x in one_stats), (name, rows, batch, pool, lanes)
                # asynchronous, two outputs reused (later passes overwrite), back to back with a one-pass call
                pair = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
                assert ds.render_device_passes(cam.desc, st, [pair[k % 2].data_ptr() for k in range(n)], s,
                                               stats=False) is None
                last = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda")
                ds.render_device_passes(cam.desc, st, [last.data_ptr()], s, stats=False)
                torch.cuda.synchronize()
                assert np.array_equal(pair[(n - 1) % 2].cpu().numpy(), singles[n - 1])
                assert np.array_equal(pair[(n - 2) % 2].cpu().numpy(), singles[n - 2])
                assert np.array_equal(last.cpu().numpy(), singles[0])
        ds.set_workspace(32 << 20, 256 << 20)
        ds.set_lanes(0)


def test_carried_grid_hint_from_a_lighter_frame(gpu):
    """The carried-extend and shading grids of a streaming frame are sized from the carried counts of the last
    completed frame of the same shape (rs_host.cpp Replica::hist); where the frame carries more paths than that
    estimate the blocks grid-stride over the rest. A frame looking at the sky (almost nothing carried) then one of
    the same shape looking at the balls (most paths carried): the second equals the oracle's frame bit for bit, and
    so does a third with a history of its own shape."""
    torch = gpu
    from raysnail_amd.api import CameraBuilder, Point3
    cam, world, _, _ = scenes.rtow_13_1(96, 60)
    sky = CameraBuilder().look_from(Point3(13.0, 2.0, 3.0)).look_at(Point3(13.0, 50.0, 3.0)).vup((1.0, 0.0, 0.0)) \
        .fov(20.0).width(96).height(60).build()
    ds = world.device_scene()
    ds.set_workspace(96 * 60, 96 * 60 * 16)  # several batches and iterations per frame
    s = torch.cuda.current_stream().cuda_stream
    st = cam.take_photo().samples(16).depth(12).seed(3).settings()
    ref, rs = _oracle(world).render(cam.desc, st, threads=16)
    out = torch.zeros((60, 96, 4), dtype=torch.float32, device="cuda")
    for _ in range(3):
        ds.render_device(sky.desc, st, out.data_ptr(), s, stats=False)
    torch.cuda.synchronize()
    for _ in range(2):
        stats = ds.render_device(cam.desc, st, out.data_ptr(), s)
        assert stats.segments == rs.segments
        assert np.array_equal(out.cpu().numpy(), ref)
