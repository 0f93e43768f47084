"""The spheres mode's camera launch shades its Lambertian / Metal / Dielectric hits itself (k_wfs_extend kFuse,
rs_kernels.hip): no level-0 record, no queue entry; the survivors enter the next set at level 1 through the next
iteration's front / back counters, the others write their radiance there and then. Pure scheduling: every frame
below equals the CPU oracle's bit for bit, and where statistics are on the segment count is the oracle's
world.hit count (the fused samples sit on a counter of their own, rs_host.cpp's byte model)."""
import numpy as np
import pytest

from raysnail_amd import scenes

pytestmark = pytest.mark.gpu
W, H = 96, 60
NPX = W * H


def _oracle(world):
    from oracle.binding import OracleScene
    return OracleScene(world)


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


def _photo(cam, spp=16, depth=8, seed=5):
    return cam.take_photo().samples(spp).depth(depth).seed(seed)


def _device_frame(torch, ds, cam, st, stats=False, mask=None):
    out = torch.full((cam.desc.height, cam.desc.width, 4), -1.0, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    r = ds.render_device(cam.desc, st, out.data_ptr(), s, mask.data_ptr() if mask is not None else 0, stats=stats)
    torch.cuda.synchronize()
    return out.cpu().numpy(), r


def test_render_and_async_device_frame(gpu, rtow):
    cam, world, ref = rtow
    photo = _photo(cam)
    want, rs = ref("d8", photo)
    ds = world.device_scene()
    for _ in range(2):  # the second frame's grids come from the first one's counts
        img, stats = ds.render(cam.desc, photo.settings())
        assert stats.segments == rs.segments, (stats.segments, rs.segments)
        assert np.array_equal(img, want)
    for _ in range(2):
        img, none = _device_frame(gpu, ds, cam, photo.settings())
        assert none is None
        assert np.array_equal(img, want)


@pytest.mark.parametrize("depth", [1, 2])
def test_depth_1_and_2(gpu, rtow, depth):
    """Depth 1: every fused sample ends at close_path, the next set stays empty (a path left there would be traced
    and counted by the next iteration: the segment count is the number of live camera samples). Depth 2: one carried
    bounce, whose paths all come from the camera launch's own stores."""
    cam, world, ref = rtow
    photo = _photo(cam, depth=depth)
    want, rs = ref(("depth", depth), photo)
    ds = world.device_scene()
    for _ in range(2):
        img, stats = ds.render(cam.desc, photo.settings())
        assert stats.segments == rs.segments, (depth, stats.segments, rs.segments)
        assert np.array_equal(img, want), depth
    if depth == 1:
        assert rs.segments == NPX * 16  # every camera sample of the unmasked frame is live and traced once
    img, _ = _device_frame(gpu, ds, cam, photo.settings())
    assert np.array_equal(img, want), depth


def test_partial_blocks_50x30x9(gpu):
    """13,500 samples: no multiple of 256 or 64 (partial last block and wave), gen_perm groups of 8 + 1 planes."""
    cam, world, _, _ = scenes.rtow_13_1(50, 30)
    photo = _photo(cam, spp=9, seed=7)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    ds = world.device_scene()
    for _ in range(2):
        img, stats = ds.render(cam.desc, photo.settings())
        assert stats.segments == rs.segments
        assert np.array_equal(img, want)
    img, _ = _device_frame(gpu, ds, cam, photo.settings())
    assert np.array_equal(img, want)


@pytest.mark.parametrize("rows", [(1, 0, 3), (0, 0, 8)])
def test_pixel_mask_on_row_shares(gpu, rtow, rows):
    """About half the pixels masked (dead camera samples in every wave), on a row share; (0, 0, 8) is the share whose
    waves take the 16 x 4 pixel tile."""
    cam, world, ref = rtow
    yy, xx = np.indices((H, W))
    mask = (((xx // 3) + (yy // 2)) % 2 == 0).astype(np.uint8)
    assert 0.4 < mask.mean() < 0.6
    photo = _photo(cam).rows(*rows)
    want, rs = ref(("mask", rows), photo, mask)
    ds = world.device_scene()
    sel = slice(rows[0], None, rows[2])
    for _ in range(2):
        img, stats = ds.render(cam.desc, photo.settings(), mask)
        assert stats.segments == rs.segments, (rows, stats.segments, rs.segments)
        assert np.array_equal(img[sel], want[sel]), rows
        assert np.all(img[sel][mask[sel] == 0] == 0.0)
    dmask = gpu.from_numpy(mask).cuda()
    img, _ = _device_frame(gpu, ds, cam, photo.settings(), mask=dmask)
    assert np.array_equal(img[sel], want[sel]), rows


def test_small_pools_carry_and_inject(gpu, rtow):
    """Pools of a few thousand paths: most iterations carry paths and inject camera samples, so the camera launch's
    survivors and the shading launches' share the next set's runs and counters; one and two lanes, one and three
    frames in flight (asynchronous frames back to back)."""
    torch = gpu
    cam, world, ref = rtow
    photo = _photo(cam)
    want, rs = ref("d8", photo)
    ds = world.device_scene()
    s = torch.cuda.current_stream().cuda_stream
    try:
        for batch, pool in ((2 * NPX, 5000), (NPX, 256 * 12)):
            ds.set_workspace(batch, pool)
            for lanes in (1, 2):
                ds.set_lanes(lanes)
                img, stats = ds.render(cam.desc, photo.settings())
                assert stats.segments == rs.segments, (batch, pool, lanes)
                assert np.array_equal(img, want), (batch, pool, lanes)
                for frames in (1, 3):
                    ds.set_frames_in_flight(frames)
                    outs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(3)]
                    for o in outs:
                        assert ds.render_device(cam.desc, photo.settings(), o.data_ptr(), s, stats=False) is None
                    torch.cuda.synchronize()
                    for o in outs:
                        assert np.array_equal(o.cpu().numpy(), want), (batch, pool, lanes, frames)
    finally:
        ds.set_workspace(32 << 20, 256 << 20)
        ds.set_lanes(0)
        ds.set_frames_in_flight(2)


@pytest.mark.parametrize("depth", [2, 8])
def test_moving_sphere_records(gpu, depth):
    """A moving sphere: the records carry the ray's time and the (item, level) tag in its own array (WfState::tagw
    = 0); the fused samples' level-1 records must carry both as the shading launch's would."""
    from raysnail_amd.api import CameraBuilder, Color, Dielectric, DiffuseLight, Glass, Gradient, HittableList, \
        Lambertian, Metal, Point3, Sphere, World
    h, lights = HittableList(), HittableList()
    h.add(Sphere((0.0, -1000.0, 0.0), 1000.0, Lambertian(Color(0.5, 0.5, 0.5, 1.0))))
    h.add(Sphere((0.0, 1.0, 0.0), 1.0, Lambertian(Color(0.7, 0.3, 0.2, 1.0))).with_speed((0.6, 0.0, 0.2)))
    h.add(Sphere((2.2, 0.8, 0.5), 0.8, Metal(Color(0.7, 0.6, 0.5, 1.0))))
    h.add(Sphere((-2.0, 0.7, 0.3), 0.7, Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass())))
    light = Sphere((0.0, 6.0, 2.0), 1.0, DiffuseLight(Color(1.0, 0.9, 0.8, 1.0)).multiplier(4.0))
    h.add(light)
    lights.add(light)
    cam = CameraBuilder().look_from(Point3(0.0, 2.0, 8.0)).look_at(Point3(0.0, 1.0, 0.0)).fov(35.0) \
        .shutter_speed(1.0).width(64).height(40).build()
    world = World(h, lights, Gradient(Color(0.3, 0.4, 0.5, 1.0), Color(0.7, 0.89, 1.0, 1.0)), (0.0, 1.0))
    photo = cam.take_photo().samples(9).depth(depth).seed(3)
    want, rs = _oracle(world).render(cam.desc, photo.settings(), threads=8)
    ds = world.device_scene()
    for _ in range(2):
        img, stats = ds.render(cam.desc, photo.settings())
        assert stats.segments == rs.segments, depth
        assert np.array_equal(img, want), depth
    img, _ = _device_frame(gpu, ds, cam, photo.settings())
    assert np.array_equal(img, want), depth


def test_frame_sequence_counter_reset_and_history(gpu, rtow):
    """Depth 1, depth 8, a row share and statistics frames alternating on one scene: the fused-sample counter is
    zeroed with the frame's other counters (by the last accumulate, or by the next frame after a statistics
    readback), and the grid history (carried and queued counts per iteration) follows the frame's shape."""
    torch = gpu
    cam, world, ref = rtow
    cases = {"d1": (_photo(cam, depth=1), ("depth", 1)), "d8": (_photo(cam), "d8"),
             "share": (_photo(cam).rows(0, 0, 4), "share4")}
    ds = world.device_scene()
    for key, with_stats in (("d1", False), ("d8", False), ("d8", True), ("share", False), ("d1", True), ("d8", False),
                            ("share", True), ("d8", True), ("d1", False), ("d8", False)):
        photo, rkey = cases[key]
        want, rs = ref(rkey, photo)
        img, stats = _device_frame(torch, ds, cam, photo.settings(), stats=with_stats)
        sel = slice(0, None, 4) if key == "share" else slice(None)
        assert np.array_equal(img[sel], want[sel]), (key, with_stats)
        if with_stats:
            assert stats.segments == rs.segments, (key, stats.segments, rs.segments)


def test_two_passes_stream(gpu, rtow):
    """Two passes as one sample stream (rs_render_device_passes): pass 1's camera samples are injected, and shaded by
    the camera launch, while pass 0's paths are carried. Each pass equals its one-pass frame; pass 0 the oracle's."""
    torch = gpu
    cam, world, ref = rtow
    ds = world.device_scene()
    s = torch.cuda.current_stream().cuda_stream
    singles, seg = [], 0
    for k in range(2):
        img, stats = _device_frame(torch, ds, cam, _photo(cam).pass_index(k).settings(), stats=True)
        singles.append(img)
        seg += stats.segments
    want, rs = ref("d8", _photo(cam))
    assert np.array_equal(singles[0], want)
    try:
        for batch, pool in ((32 << 20, 16 << 20), (4 * NPX, 7000)):
            ds.set_workspace(batch, pool)
            for lanes in (1, 2):
                ds.set_lanes(lanes)
                outs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
                stats = ds.render_device_passes(cam.desc, _photo(cam).settings(), [o.data_ptr() for o in outs], s)
                assert stats.segments == seg, (batch, pool, lanes)
                for k in range(2):
                    assert np.array_equal(outs[k].cpu().numpy(), singles[k]), (batch, pool, lanes, k)
    finally:
        ds.set_workspace(32 << 20, 256 << 20)
        ds.set_lanes(0)
