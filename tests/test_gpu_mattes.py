"""Material-id mattes (rs_render_mattes / _device) and their extraction (rs_matte_extract / _device) on the GPU against
the CPU oracle, bit for bit on integer views: one scene per scene mode and the RayMarcher variant, two frame sizes at
every sample count that takes another path through the kernel's reduction (several pixels per wave, one chunk, several
chunks with a ragged last one), the rank counts, the bounce budgets, masks, lattices, virtual devices, a side stream
between guard zones, an exact tie, more distinct ids than ranks and than the table holds, and the layers above.
Expected layers are built by tests/mattes_ref.py from oracle calls alone (each reference once per process, read only);
tests/test_mattes_cpu.py checks the fixtures from the oracle alone."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import features_ref as F
import mattes_ref as M
import spec_features_ref as R
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

pytestmark = pytest.mark.gpu

BG, EMPTY = A.RS_MATTE_ID_BACKGROUND, A.RS_MATTE_ID_EMPTY
ID_SENTINEL, COV_SENTINEL, OVF_SENTINEL = np.int32(-77777), np.float32(-123.25), np.uint8(0xAB)
SAMPLES = (1, 4, 9, 16, 64, 100, 130)
SIZES = ((37, 23), (11, 7))


def _assert_layers(got, exp, where=None):
    """bitwise on every pixel of `where` (all when None): ids, coverages (as uint32) and overflow"""
    (gi, gc, go), (ei, ec, eo) = got, exp
    ok = (gi == ei).all(axis=-1) & (gc.view(np.uint32) == ec.view(np.uint32)).all(axis=-1)
    if go is not None:
        ok = ok & (go == eo)
    if where is not None:
        ok = ok | ~where
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (len(bad), [(int(y), int(x), gi[y, x].tolist(), ei[y, x].tolist(), gc[y, x].tolist(),
                                       ec[y, x].tolist()) for y, x in bad[:3]])


# ---------------------------------------------------------------- references, once per process ----
@functools.lru_cache(maxsize=None)
def _features(w, h):
    """(camera, world, the oracle's hit function, Bouncer) of the features scene at w x h: every material kind, a
    Metal, a Dielectric and a MixedMaterial(Metal, ..) sphere, an object without a material, aperture and shutter"""
    cam, world = scenes.features_scene(w, h)
    orc, rec = R.oracle_scene(world)
    return cam, world, F.oracle_hits(orc), R.Bouncer(F.Albedo(rec))


@functools.lru_cache(maxsize=None)
def _features_ids(w, h, samples, m):
    cam, world, hit_fn, bouncer = _features(w, h)
    photo = cam.take_photo().samples(samples).seed(5).pass_index(1)
    return M.frame_ids(cam.desc, photo.settings(), hit_fn, bouncer, m) + (photo,)


@functools.lru_cache(maxsize=None)
def _features_layers(w, h, samples, m, ranks):
    ids, _, _ = _features_ids(w, h, samples, m)
    out = M.layers(ids, w, h, ranks)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- sample counts, frame sizes, ranks ----
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_counts(gpu, size, samples):
    """the features scene, max_specular 1, ranks 1, 4 and 8 of the same samples: N = 1 .. 16 (64 .. 4 pixels per wave,
    7 with a lane left over at N = 9), 64 (one pixel, one chunk), 100 (64 + 36) and samples = 130 (N = 121: not a
    square; 64 + 57). segments is the restatement's World::hit count"""
    w, h = size
    cam, world, _, _ = _features(w, h)
    ids, calls, photo = _features_ids(w, h, samples, 1)
    sq = int(np.floor(np.sqrt(samples)))
    assert ids.shape == (w * h, sq * sq)
    ds = world.device_scene()
    for ranks in (1, 4, 8):
        gi, gc, go, stats = ds.render_mattes(cam.desc, photo.settings(), ranks, 1)
        _assert_layers((gi, gc, go), _features_layers(w, h, samples, 1, ranks))
        assert stats.samples == w * h * sq * sq and stats.segments == int(calls.sum())
        assert stats.kernel_id == A.RS_KERNEL_MATTES and stats.kernel_launches == 1
    assert (go == 0).all()


@pytest.mark.parametrize("m", [0, 1, 4])
def test_bounce_budgets(gpu, m):
    """37 x 23, N = 9, ranks 4: at 0 the id is the first hit's (field 12 of the oracle's record, the background on a
    miss); at 1 and 4 chains through the mirror and the glass end elsewhere, and a chain that escapes reports the
    background id where the first hit was a surface"""
    w, h = 37, 23
    cam, world, hit_fn, _ = _features(w, h)
    ids, calls, photo = _features_ids(w, h, 9, m)
    first_ids, _, _ = _features_ids(w, h, 9, 0)
    if m == 0:
        rays = F.camera_rays(cam.desc, photo.settings(), [(x, y) for y in range(h) for x in range(w)]).reshape(-1, 7)
        recs = hit_fn(rays)
        assert (ids.reshape(-1) == np.where(recs[:, 0] == 1.0, recs[:, 12], BG).astype(np.int64)).all()
        assert (calls == 1).all()
    else:
        escaped = (ids == BG) & (first_ids != BG)
        assert escaped.any() and ((ids != first_ids) & (ids != BG)).any()
    gi, gc, go, stats = world.device_scene().render_mattes(cam.desc, photo.settings(), 4, m)
    _assert_layers((gi, gc, go), _features_layers(w, h, 9, m, 4))
    assert stats.segments == int(calls.sum())
    assert (gi == BG).any()


def test_unmaterialed_object_and_coverage_sum(gpu):
    """an object without a material reports RS_NO_MATERIAL; the coverages of a pixel with at most 8 distinct ids and no
    overflow sum to 1 within 8 x 2^-24 at ranks 8 (each is one rounding of an exact fraction below 1)"""
    w, h = 37, 23
    cam, world, _, _ = _features(w, h)
    ids, _, photo = _features_ids(w, h, 16, 1)
    gi, gc, go, _ = world.device_scene().render_mattes(cam.desc, photo.settings(), 8, 1)
    assert (gi == A.RS_NO_MATERIAL).any() and (ids == A.RS_NO_MATERIAL).any()
    distinct = np.array([len(set(r.tolist())) for r in ids]).reshape(h, w)
    small = (distinct <= 8) & (go == 0)
    assert small.sum() > w * h // 2
    total = gc.astype(np.float64).sum(axis=-1)
    assert (np.abs(total[small] - 1.0) <= 8 * 2.0 ** -24).all(), float(np.abs(total[small] - 1.0).max())
    assert ((gi != EMPTY).sum(axis=-1)[small] == distinct[small]).all()
    assert (gc[gi == EMPTY] == 0.0).all() and not np.signbit(gc[gi == EMPTY]).any()


# ---------------------------------------------------------------- scene modes ----
@functools.lru_cache(maxsize=None)
def _mode_scene(name):
    build = {"spheres": lambda: scenes.rtow_13_1(37, 23, seed=7)[:2], "mesh": lambda: R.mesh_glass_scene(37, 23),
             "rich": lambda: R.rich_glass_scene(37, 23)}[name]
    cam, world = build()
    orc, rec = R.oracle_scene(world)
    photo = cam.take_photo().samples(4).seed(11).pass_index(2)
    ids, calls = M.frame_ids(cam.desc, photo.settings(), F.oracle_hits(orc), R.Bouncer(F.Albedo(rec)), 3)
    return cam, world, photo, ids, calls


@pytest.mark.parametrize("name,mode", [("spheres", 1), ("mesh", 2), ("rich", 0)])
def test_scene_modes(gpu, name, mode):
    """37 x 23, N = 4, max_specular 3, ranks 4: RTIOW 13.1 (the spheres-only 4-wide tree), a Dielectric triangle mesh
    (flat mesh tree) and the rich generic mode (the chain through the glass sphere ends on the medium's own Isotropic
    material, which has a handle like any other), each through the one generic kernel"""
    cam, world, photo, ids, calls = _mode_scene(name)
    ds = world.device_scene()
    assert ds.info().scene_mode == mode
    assert len(np.unique(ids)) >= 2  # a surface and the background at least (the glass mesh itself is seen through)
    gi, gc, go, stats = ds.render_mattes(cam.desc, photo.settings(), 4, 3)
    _assert_layers((gi, gc, go), M.layers(ids, 37, 23, 4))
    assert stats.segments == int(calls.sum())


def test_metal_raymarcher(gpu):
    """raymarching_test with a Metal Mandelbulb at 11 x 7, N = 4, max_specular 2, ranks 4, through the marcher unit's
    kernel. The oracle has no marcher: the hit records come from rs_probe_world_hit (pinned against
    tests/raymarch_ref.py by tests/test_gpu_raymarch.py), the bounces from the oracle's Metal as everywhere"""
    cam, world = R.marcher_metal(11, 7)
    photo = cam.take_photo().samples(4).seed(3).pass_index(0)
    ds, rec = F.device_scene(world)
    assert ds.info().scene_mode == 0 and ds.info().ref_order == 1
    ids, calls = M.frame_ids(cam.desc, photo.settings(), F.probe_hits(ds), R.Bouncer(F.Albedo(rec)), 2)
    assert (calls > 1).sum() >= 10 and len(np.unique(ids)) >= 2
    gi, gc, go, stats = ds.render_mattes(cam.desc, photo.settings(), 4, 2)
    _assert_layers((gi, gc, go), M.layers(ids, 11, 7, 4))
    assert stats.segments == int(calls.sum())


# ---------------------------------------------------------------- masks, lattices, devices, streams ----
def _sentinel_layers(h, w, ranks):
    return (np.full((h, w, ranks), ID_SENTINEL, np.int32), np.full((h, w, ranks), COV_SENTINEL, np.float32),
            np.full((h, w), OVF_SENTINEL, np.uint8))


@pytest.mark.parametrize("samples", [9, 100])
def test_lattice_and_mask(gpu, samples):
    """every third row from row 1 and a checkerboard mask over sentinel-filled arrays: masked pixels are empty in every
    rank with overflow 0, the other lattice pixels are the full frame's, rows off the lattice keep the caller's
    values; then a band of rows (row_begin 5, row_end 16, step 1)"""
    w, h = 37, 23
    cam, world, _, _ = _features(w, h)
    _, calls, photo = _features_ids(w, h, samples, 1)
    exp = _features_layers(w, h, samples, 1, 4)
    N = calls.shape[1]
    yy, xx = np.mgrid[0:h, 0:w]
    mask = ((xx + yy) % 2).astype(np.uint8)
    ds = world.device_scene()
    for (begin, end, step) in ((1, 0, 3), (5, 16, 1)):
        on_lattice = (yy >= begin) & ((yy - begin) % step == 0) & ((yy < end) if end else True)
        gi, gc, go = _sentinel_layers(h, w, 4)
        st = photo.settings()
        st.row_begin, st.row_end, st.row_step = begin, end, step
        _, _, _, stats = ds.render_mattes(cam.desc, st, 4, 1, mask, ids=gi, cov=gc, overflow=go)
        assert (gi[~on_lattice] == ID_SENTINEL).all() and (gc[~on_lattice] == COV_SENTINEL).all()
        assert (go[~on_lattice] == OVF_SENTINEL).all()
        off = on_lattice & (mask == 0)
        assert (gi[off] == EMPTY).all() and (gc[off] == 0.0).all() and (go[off] == 0).all()
        live = on_lattice & (mask == 1)
        _assert_layers((gi, gc, go), exp, where=live)
        assert stats.samples == int(on_lattice[:, 0].sum()) * w * N
        assert stats.segments == int(calls.reshape(h, w, N)[live].sum())  # masked pixels trace nothing


def test_two_virtual_devices(gpu):
    """devices = [0, 0]: the row lattice split over two replicas and gathered, host and device call, bitwise the
    one-device layers; the overflow plane may be left out"""
    torch = gpu
    w, h = 37, 23
    cam, world, _, _ = _features(w, h)
    _, calls, photo = _features_ids(w, h, 9, 1)
    exp = _features_layers(w, h, 9, 1, 4)
    ds2 = api.DeviceScene(world, devices=[0, 0])
    assert ds2.info().n_devices == 2
    gi, gc, go, stats = ds2.render_mattes(cam.desc, photo.settings(), 4, 1)
    _assert_layers((gi, gc, go), exp)
    assert stats.segments == int(calls.sum())
    gi, gc, go, _ = ds2.render_mattes(cam.desc, photo.settings(), 4, 1, want_overflow=False)
    assert go is None
    _assert_layers((gi, gc, None), exp)
    ti = torch.full((h, w, 4), int(ID_SENTINEL), dtype=torch.int32, device="cuda")
    tc = torch.full((h, w, 4), float(COV_SENTINEL), dtype=torch.float32, device="cuda")
    to = torch.full((h, w), int(OVF_SENTINEL), dtype=torch.uint8, device="cuda")
    ds2.render_mattes_device(cam.desc, photo.settings(), ti.data_ptr(), tc.data_ptr(), to.data_ptr(), 4, 1,
                             torch.cuda.current_stream().cuda_stream)
    _assert_layers((ti.cpu().numpy(), tc.cpu().numpy(), to.cpu().numpy()), exp)


@pytest.mark.parametrize("samples", [4, 100])
def test_device_call_on_side_stream_between_guard_zones(gpu, samples):
    """rs_render_mattes_device on a non-default stream with stats = NULL (asynchronous) and overflow = NULL, the ids
    and the coverages in the middle of sentinel-filled allocations: after a stream sync the layers are the oracle's
    and the guard zones before, between and after them are untouched"""
    torch = gpu
    w, h, ranks = 37, 23, 8
    cam, world, _, _ = _features(w, h)
    _, _, photo = _features_ids(w, h, samples, 1)
    exp = _features_layers(w, h, samples, 1, ranks)
    ds = world.device_scene()
    side = torch.cuda.Stream()
    n, guard = h * w * ranks, 4096
    buf = torch.full((3 * guard + 2 * n,), float(COV_SENTINEL), dtype=torch.float32, device="cuda")
    sentinel_bits = int(np.array([COV_SENTINEL]).view(np.int32)[0])
    ti, tc = buf[guard:guard + n], buf[2 * guard + n:2 * guard + 2 * n]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert ds.render_mattes_device(cam.desc, photo.settings(), ti.data_ptr(), tc.data_ptr(), 0, ranks, 1,
                                       side.cuda_stream, stats=False) is None
    side.synchronize()
    host = buf.cpu().numpy()
    gi = host[guard:guard + n].view(np.int32).reshape(h, w, ranks)
    gc = host[2 * guard + n:2 * guard + 2 * n].reshape(h, w, ranks)
    _assert_layers((gi, gc, None), exp)
    for lo in (0, guard + n, 2 * guard + 2 * n):
        assert (host[lo:lo + guard].view(np.int32) == sentinel_bits).all()


# ---------------------------------------------------------------- ties and overflow ----
@pytest.mark.parametrize("left_first", [True, False])
def test_exact_tie(gpu, left_first):
    """two coplanar rects meeting on the middle pixel column's centre line, sqrt_spp 2 and 4: both halves are exactly
    N / 2 and rank 0 is the smaller handle, whichever side it is on (tests/test_mattes_cpu.py shows it from the oracle)"""
    cam, world, left, right = M.tie_scene(left_first)
    orc, rec = R.oracle_scene(world)
    ds = world.device_scene()
    assert {ds.material_id(left), ds.material_id(right)} == {0, 1}
    assert ds.material_id(left) == (0 if left_first else 1)
    for samples in (4, 16):
        photo = cam.take_photo().samples(samples).seed(1)
        ids, _ = M.frame_ids(cam.desc, photo.settings(), F.oracle_hits(orc), R.Bouncer(F.Albedo(rec)), 0)
        gi, gc, go, _ = ds.render_mattes(cam.desc, photo.settings(), 2, 0)
        _assert_layers((gi, gc, go), M.layers(ids, 5, 3, 2))
        assert (gi[:, 2] == np.array([0, 1])).all() and (gc[:, 2] == 0.5).all()


@functools.lru_cache(maxsize=None)
def _lattice():
    cam, world, photo, mats = M.lattice_scene()
    orc, rec = R.oracle_scene(world)
    ids, _ = M.frame_ids(cam.desc, photo.settings(), F.oracle_hits(orc), R.Bouncer(F.Albedo(rec)), 0)
    return cam, world, photo, mats, ids


@pytest.mark.parametrize("ranks", [1, 4, 8])
def test_more_ids_than_ranks_and_than_the_table(gpu, ranks):
    """the 10 x 10 sphere lattice under a 3 x 2 frame at 100 spp: pixel (1, 0) has 71 distinct ids (overflow 1: the
    background and the 63 smallest handles survive with their full counts), pixel (0, 0) 31 (overflow 0), the rest the
    background alone"""
    cam, world, photo, mats, ids = _lattice()
    exp = M.layers(ids, 3, 2, ranks)
    assert exp[2].tolist() == [[0, 1, 0], [0, 0, 0]]
    assert [len(set(ids[p].tolist())) for p in range(6)] == [31, 71, 1, 1, 1, 1]
    ds = world.device_scene()
    gi, gc, go, _ = ds.render_mattes(cam.desc, photo.settings(), ranks, 0)
    _assert_layers((gi, gc, go), exp)
    assert go[0, 1] == 1 and go[0, 0] == 0 and go.sum() == 1
    assert gi[0, 1, 0] == BG and gc[0, 1, 0] == np.float32(0.3)
    if ranks == 8:
        assert gi[0, 1, 1:].tolist() == sorted(set(ids[1].tolist()) - {BG})[:7]
        assert gi[0, 1, 1] == ds.material_id(mats[3])


# ---------------------------------------------------------------- extraction ----
def test_matte_extract(gpu):
    """rs_matte_extract_device on rendered layers (37 x 23 x 8 and x 1) against the restatement, bit for bit: one id,
    several, one that is nowhere, the background, the empty id, 64 ids, ranks = 1, a side stream between guard zones,
    and the host entry"""
    torch = gpu
    w, h = 37, 23
    cam, world, _, _ = _features(w, h)
    _, _, photo = _features_ids(w, h, 16, 1)
    present = [int(i) for i in np.unique(_features_ids(w, h, 16, 1)[0]) if i >= 0]
    assert len(present) >= 4
    wanted_sets = ([present[0]], present[1:4], [12345], [BG], [BG, A.RS_NO_MATERIAL] + present, [EMPTY, present[0]],
                   list(range(1000, 1063)) + [present[1]])
    side = torch.cuda.Stream()
    for ranks in (8, 1):
        ei, ec, _ = _features_layers(w, h, 16, 1, ranks)
        ti, tc = torch.from_numpy(np.array(ei)).cuda(), torch.from_numpy(np.array(ec)).cuda()
        guard = 1024
        buf = torch.full((2 * guard + w * h,), float(COV_SENTINEL), dtype=torch.float32, device="cuda")
        out = buf[guard:guard + w * h]
        torch.cuda.synchronize()
        for wanted in wanted_sets:
            exp = M.matte_extract(ei, ec, wanted)
            with torch.cuda.stream(side):
                api.matte_extract_device(ti.data_ptr(), tc.data_ptr(), w, h, ranks, wanted, out.data_ptr(), side.cuda_stream)
            side.synchronize()
            host = buf.cpu().numpy()
            got = host[guard:guard + w * h].reshape(h, w)
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (ranks, wanted)
            assert (host[:guard] == COV_SENTINEL).all() and (host[guard + w * h:] == COV_SENTINEL).all()
            got_host = api.matte_extract(ei, ec, wanted)
            assert np.array_equal(got_host.view(np.uint32), exp.view(np.uint32)), (ranks, wanted)
        assert (M.matte_extract(ei, ec, [12345]) == 0.0).all() and (M.matte_extract(ei, ec, [BG]) > 0.0).any()
    # the background and every surface together: the whole pixel, where 8 ranks hold all of its ids
    ei, ec, _ = _features_layers(w, h, 16, 1, 8)
    everything = api.matte_extract(ei, ec, [BG, A.RS_NO_MATERIAL] + present)
    full = (ei != EMPTY).sum(axis=-1) < 8
    assert (np.abs(everything[full].astype(np.float64) - 1.0) <= 8 * 2.0 ** -24).all()


# ---------------------------------------------------------------- the layers above ----
def test_python_layers(gpu):
    """shot_mattes is the explicit call under the photo's settings, rows and mask; material_id names what the layers
    hold; render_mattes_device with stats gives the host call's layers"""
    torch = gpu
    w, h = 37, 23
    cam, world, _, _ = _features(w, h)
    _, _, photo = _features_ids(w, h, 9, 1)
    exp = _features_layers(w, h, 9, 1, 4)
    ids, cov, ovf = photo.shot_mattes(world, None, 4, 1)
    _assert_layers((ids, cov, ovf), exp)
    assert photo.last_stats.kernel_id == A.RS_KERNEL_MATTES

    class EveryOther(api.PixelController):
        def calculate_pixel(self, x, y):
            return (x + y) % 2 == 0
    ids, cov, ovf = photo.shot_mattes(world, EveryOther(), max_specular=1)
    yy, xx = np.mgrid[0:h, 0:w]
    _assert_layers((ids, cov, ovf), exp, where=(xx + yy) % 2 == 0)
    assert (ids[(xx + yy) % 2 == 1] == EMPTY).all()
    ds = world.device_scene()
    named = {ds.material_id(o.material) for o in world.hittables.objects if hasattr(o, "material")}
    seen = set(np.unique(exp[0]).tolist()) - {BG, EMPTY}
    assert seen & named and A.RS_NO_MATERIAL in named
    ti = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda")
    tc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    to = torch.ones((h, w), dtype=torch.uint8, device="cuda")
    stats = ds.render_mattes_device(cam.desc, photo.settings(), ti.data_ptr(), tc.data_ptr(), to.data_ptr(), 4, 1)
    _assert_layers((ti.cpu().numpy(), tc.cpu().numpy(), to.cpu().numpy()), exp)
    assert stats.kernel_id == A.RS_KERNEL_MATTES and stats.segments == int(_features_ids(w, h, 9, 1)[1].sum())


def test_cpp_layer_on_the_gpu(gpu, tmp_path):
    """tests/cpp/test_mattes_api.cpp in its `gpu` mode: shot_mattes(world, mask, 4, 2), shot_mattes(world, mask, 2),
    matte_extract and material_id of the C++ host layer (8 x 6, 4 samples, seed 3, pass 1, every other pixel masked)
    give what the Python layer gives of the same world"""
    import test_mattes_cpp as T
    exe, path = T.build(tmp_path), tmp_path / "mattes.bin"
    r = subprocess.run([str(exe), "gpu", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
    raw = np.fromfile(path, np.uint8)
    n, pos, got = 6 * 8, 0, []
    for count, dt in ((n * 4, np.int32), (n * 4, np.float32), (n, np.uint8), (n * 2, np.int32), (n * 2, np.float32),
                      (n, np.uint8), (n, np.float32), (3, np.int32)):
        size = count * np.dtype(dt).itemsize
        got.append(raw[pos:pos + size].view(dt))
        pos += size
    assert pos == len(raw)
    h, lights = api.HittableList(), api.HittableList()
    sun = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    mirror, grey = api.Metal(api.Color(0.5, 0.75, 0.25)), api.Lambertian(api.Color(0.5, 0.5, 0.5))
    h.add(api.Sphere((0.0, 0.0, 0.0), 1.0, mirror))
    h.add(api.Sphere((0.0, -101.0, 0.0), 100.0, grey))
    h.add(sun)
    lights.add(sun)
    world = api.World(h, lights)
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(8).height(6).build()

    class EveryOther(api.PixelController):
        def calculate_pixel(self, x, y):
            return (x + y) % 2 == 0
    photo = cam.take_photo().samples(4).seed(3).pass_index(1)
    i2, c2, o2 = photo.shot_mattes(world, EveryOther(), 4, 2)
    i0, c0, o0 = photo.shot_mattes(world, EveryOther(), 2)
    ds = world.device_scene()
    names = [ds.material_id(mirror), ds.material_id(grey), ds.material_id(sun.material)]
    matte = api.matte_extract(i2, c2, [names[1], BG])
    assert not np.array_equal(i2[..., :2], i0)  # the mirror shows what it reflects
    for g, e in zip(got, (i2, c2, o2, i0, c0, o0, matte, np.array(names, np.int32))):
        assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(e).reshape(-1).view(np.uint8))
