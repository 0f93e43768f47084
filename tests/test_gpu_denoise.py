"""rs_denoise_device / rs_denoise on the GPU, bit for bit against the numpy restatement of the header's contract
(tests/denoise_ref.py; NaNs compare equal, as features_ref.same_bits): seeded synthetic frames at two sizes -- 37 x 23,
smaller than any tile and than the level-4 reach (taps leave the frame on both sides at once), and 149 x 67, several
tiles in each direction with a remainder, wider than two tiles plus the LDS halo -- and one rendered frame."""
import numpy as np
import pytest

import denoise_ref as D
import features_ref as F
from raysnail_amd import api, scenes

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (149, 67)]
SENTINEL = -123.25
GUARD = 4096  # floats on each side of the workspace


@pytest.fixture(scope="module")
def frames():
    """the synthetic frames of both sizes (computed once, never modified)"""
    out = {}
    for k, (w, h) in enumerate(SIZES):
        out[(w, h)] = D.synthetic(w, h, 10 + k)
        for a in out[(w, h)]:
            a.setflags(write=False)
    return out


def _kw(st):
    return dict(levels=st.levels, sigma_color=st.sigma_color, sigma_normal=st.sigma_normal, sigma_depth=st.sigma_depth)


def run_device(torch, beauty, albedo, normal, st, gamma, in_place=False, stream=None):
    """rs_denoise_device on copies of the frames; the output frame as numpy. The workspace sits between two guard
    zones that must come back untouched, and the inputs must come back as they went in (the beauty frame too, unless
    in place)."""
    h, w = beauty.shape[:2]
    dev = [None if a is None else torch.from_numpy(np.array(a, np.float32)).cuda() for a in (beauty, albedo, normal)]
    keep = [None if t is None else t.clone() for t in dev]
    n_work = 2 * w * h * 4
    arena = torch.full((n_work + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    work = arena[GUARD:GUARD + n_work]
    out = dev[0] if in_place else torch.full((h, w, 4), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ptr = [0 if t is None else t.data_ptr() for t in dev]
    api.denoise_device(ptr[0], ptr[1], ptr[2], w, h, out.data_ptr(), work.data_ptr(), st, bool(gamma),
                       0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    assert bool((arena[:GUARD] == SENTINEL).all()) and bool((arena[GUARD + n_work:] == SENTINEL).all())
    for t, k in zip(dev[0 if not in_place else 1:], keep[0 if not in_place else 1:]):
        assert t is None or torch.equal(t.view(torch.int32), k.view(torch.int32))
    return out.cpu().numpy()


def assert_same(got, exp):
    ok = F.same_bits(got, exp).all(axis=-1)
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (len(bad), [(int(y), int(x), got[y, x].tolist(), exp[y, x].tolist()) for y, x in bad[:4]])


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("levels", [1, 3, 5, 8])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_levels_and_gamma(gpu, frames, size, levels, gamma):
    """levels 1 (the one launch is first and last), 3, 5 and 8 (step 128: wider than either frame), both gammas"""
    beauty, albedo, normal = frames[size]
    st = api.DenoiseSettings(levels=levels)
    got = run_device(gpu, beauty, albedo, normal, st, gamma)
    assert_same(got, D.denoise(beauty, albedo, normal, gamma=gamma, **_kw(st)))
    assert np.isfinite(got).all()


@pytest.mark.parametrize("which", ["no_albedo", "no_normal", "neither"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_optional_guides(gpu, frames, size, which):
    beauty, albedo, normal = frames[size]
    a = None if which in ("no_albedo", "neither") else albedo
    n = None if which in ("no_normal", "neither") else normal
    st = api.DenoiseSettings()
    for gamma in (0, 1):
        assert_same(run_device(gpu, beauty, a, n, st, gamma), D.denoise(beauty, a, n, gamma=gamma, **_kw(st)))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_and_nan(gpu, frames, size):
    """a masked checkerboard (alpha 0, loud values left in the masked pixels of all three frames) and one NaN pixel
    on a tile edge (x = 31 | 63, y = 7: the last column and row of a 64 x 4 and of a 32 x 8 tile): masked pixels
    and the NaN pixel come back bit for bit, everything else is the restatement's and finite"""
    w, h = size
    beauty, albedo, normal = (a.copy() for a in frames[size])
    yy, xx = np.mgrid[0:h, 0:w]
    masked = (xx + yy) % 2 == 1
    beauty[masked] = [1e6, -3.0, 2.0, 0.0]
    albedo[masked] = [9.0, 9.0, 9.0, 1.0]
    normal[masked] = [5.0, 5.0, 5.0, 1e3]
    nx, ny = (63 if w > 64 else 31), 7
    assert not masked[ny, nx]
    beauty[ny, nx, 1] = np.array([0x7FC00123], np.uint32).view(np.float32)[0]
    st = api.DenoiseSettings()
    got = run_device(gpu, beauty, albedo, normal, st, 1)
    assert_same(got, D.denoise(beauty, albedo, normal, gamma=1, **_kw(st)))
    unusable = masked.copy()
    unusable[ny, nx] = True
    assert (got.view(np.uint32)[unusable] == beauty.view(np.uint32)[unusable]).all()
    assert np.isfinite(got[~unusable]).all()
    # the all-zero mask convention of rs_render
    beauty[masked] = 0.0
    got0 = run_device(gpu, beauty, albedo, normal, st, 1)
    assert (got0.view(np.uint32)[masked] == 0).all()
    assert (got0.view(np.uint32)[~masked] == got.view(np.uint32)[~masked]).all()  # nothing of the masked values leaked


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place(gpu, frames, size):
    """d_out == d_beauty is bitwise the out-of-place result, one level (the launch reads and writes the frame) and five"""
    beauty, albedo, normal = frames[size]
    for levels in (1, 5):
        st = api.DenoiseSettings(levels=levels)
        a = run_device(gpu, beauty, albedo, normal, st, 1)
        b = run_device(gpu, beauty, albedo, normal, st, 1, in_place=True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_side_stream(gpu, frames):
    """enqueued on a non-default stream and read after that stream's synchronise"""
    torch = gpu
    beauty, albedo, normal = frames[SIZES[1]]
    st = api.DenoiseSettings()
    side = torch.cuda.Stream()
    got = run_device(torch, beauty, albedo, normal, st, 1, stream=side)
    assert_same(got, D.denoise(beauty, albedo, normal, gamma=1, **_kw(st)))


def test_host_entry_equals_device_entry(gpu, frames):
    for size in SIZES:
        beauty, albedo, normal = frames[size]
        st = api.DenoiseSettings(levels=4, sigma_color=0.5)
        for a, n, gamma in ((albedo, normal, 1), (None, normal, 0), (None, None, 1)):
            host = api.denoise(beauty, a, n, st, bool(gamma))
            assert np.array_equal(host.view(np.uint32), run_device(gpu, beauty, a, n, st, gamma).view(np.uint32))
    # every guide combination of the host entry's staging, on a 67 x 5 frame: no multiple of the 64 x 4 tile or of the
    # block, two tiles each way
    beauty, albedo, normal = D.synthetic(67, 5, 12)
    for a, n, gamma in ((None, None, 0), (albedo, None, 1), (None, normal, 1), (albedo, normal, 0)):
        host = api.denoise(beauty, a, n, st, bool(gamma))
        assert np.array_equal(host.view(np.uint32), run_device(gpu, beauty, a, n, st, gamma).view(np.uint32))


def test_rendered_frame(gpu):
    """the features scene at 48 x 30, N = 9, depth 4: render + render_features, then the device entry on the GPU's
    own three frames is bitwise the restatement on them, and shot_denoised returns the same pair"""
    torch = gpu
    w, h = 48, 30
    cam, world = scenes.features_scene(w, h)
    photo = cam.take_photo().samples(9).depth(4).seed(5).pass_index(1)
    ds = world.device_scene()
    beauty, _ = ds.render(cam.desc, photo.settings())
    albedo, normal, _ = ds.render_features(cam.desc, photo.settings())
    assert (beauty[..., 3] == 1.0).all() and 0.0 < albedo[..., 3].mean() < 1.0
    st = api.DenoiseSettings()
    got = run_device(torch, beauty, albedo, normal, st, 1)
    assert_same(got, D.denoise(beauty, albedo, normal, gamma=1, **_kw(st)))
    assert not np.array_equal(got, beauty)
    den, raw = photo.shot_denoised(world)
    assert np.array_equal(raw.view(np.uint32), beauty.view(np.uint32))
    assert np.array_equal(den.view(np.uint32), got.view(np.uint32))


def test_cpp_shot_denoised_on_the_gpu(gpu, tmp_path):
    """tests/cpp/test_denoise_api.cpp in its `gpu` mode: raysnail::TakePhotoSettings::shot_denoised (8 x 6, 4 samples,
    seed 3, pass 1, every other pixel masked) writes the frames the Python layer computes of the same world"""
    import subprocess
    from test_denoise_cpp import build_driver
    exe, out = build_driver(tmp_path), tmp_path / "frames.f32"
    r = subprocess.run([str(exe), "gpu", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
    got = np.fromfile(out, np.float32).reshape(2, 6, 8, 4)
    hl, lights = api.HittableList(), api.HittableList()
    sun = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    hl.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    hl.add(sun)
    lights.add(sun)
    world = api.World(hl, lights)
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(8).height(6).build()

    class EveryOther(api.PixelController):
        def calculate_pixel(self, x, y):
            return (x + y) % 2 == 0
    den, raw = cam.take_photo().samples(4).seed(3).pass_index(1).shot_denoised(world, EveryOther())
    assert (raw[1::2, 0::2] == 0.0).all() and (den[1::2, 0::2] == 0.0).all()  # masked pixels stay [0,0,0,0]
    assert F.same_bits(got[0], den).all() and F.same_bits(got[1], raw).all()
