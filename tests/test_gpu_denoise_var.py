"""rs_pass_moments[_device] and rs_denoise_var[_device] on the GPU, bit for bit (uint32 views) against the numpy
restatements of the header's contracts (tests/denoise_var_ref.py): denoise_ref's seeded synthetic frames at 37 x 23
(smaller than any tile and than the level-4 reach) and 149 x 67 (several tiles in each direction with a remainder) plus
a seeded variance frame with exact zeros, a block four orders of magnitude above the rest and coverage-weighted
regions; and one rendered chain."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import denoise_var_ref as V
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (149, 67)]
SENTINEL = -123.25
GUARD = 4096  # floats on each side of a guarded buffer
SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, exp):
    ok = (_bits(got) == _bits(exp)).all(axis=-1)
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (len(bad), [(int(y), int(x), got[y, x].tolist(), exp[y, x].tolist()) for y, x in bad[:4]])


class Guarded:
    """n floats of device memory between two guard zones that must come back untouched"""

    def __init__(self, torch, n):
        self.torch, self.n = torch, n
        self.arena = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.arena[GUARD:GUARD + n]

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        assert bool((self.arena[:GUARD] == SENTINEL).all()) and bool((self.arena[GUARD + self.n:] == SENTINEL).all())

    def numpy(self, shape):
        return self.t.cpu().numpy().reshape(shape)


# ------------------------------------------------------------------------------ pass moments ----
@pytest.fixture(scope="module")
def pass_frames():
    """per size: 64 seeded pass frames; frame k masked on a checkerboard for odd k; one NaN pixel in frame 2 at a tile
    edge (x = 63 | 36: the last column of a 64-wide tile or of the frame; y = 3, the last row of a tile row), one pixel
    masked in all frames; the expected moments per (K, gamma) are computed on demand from these, never modified"""
    out = {}
    for i, (w, h) in enumerate(SIZES):
        rng = np.random.default_rng(40 + i)
        yy, xx = np.mgrid[0:h, 0:w]
        board = (xx + yy) % 2 == 1
        frames = []
        for k in range(64):
            f = np.ones((h, w, 4), np.float32)
            f[..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(3.0)
            if k % 2 == 1:
                f[board] = [5.0, 5.0, 5.0, 0.0] if k % 4 == 1 else 0.0
            f[h - 2, 1] = 0.0
            frames.append(f)
        nx = 63 if w > 64 else w - 1
        frames[2][3, nx, 1] = np.array([0x7FC00321], np.uint32).view(np.float32)[0]
        frames[0][4, min(64, w - 2), 0] = np.inf
        for f in frames:
            f.setflags(write=False)
        out[(w, h)] = frames
    return out


def run_moments(torch, frames, gamma, want=(True, True), alias_mean=False, stream=None):
    """rs_pass_moments_device on copies of the frames: (mean, var) as numpy (None where not asked for). The outputs sit
    between guard zones; the inputs must come back as they went in (but for the frame the mean aliases)."""
    h, w = frames[0].shape[:2]
    dev = [torch.from_numpy(np.array(f, np.float32)).cuda() for f in frames]
    keep = [t.clone() for t in dev]
    mean = Guarded(torch, w * h * 4) if want[0] and not alias_mean else None
    var = Guarded(torch, w * h * 4) if want[1] else None
    torch.cuda.synchronize()
    mean_ptr = dev[0].data_ptr() if alias_mean else (mean.ptr() if mean else 0)
    api.pass_moments_device([t.data_ptr() for t in dev], w, h, mean_ptr, var.ptr() if var else 0, bool(gamma),
                            0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    for g in (mean, var):
        if g is not None:
            g.check()
    for t, k in list(zip(dev, keep))[1 if alias_mean else 0:]:
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    m = dev[0].cpu().numpy() if alias_mean else (mean.numpy((h, w, 4)) if mean else None)
    return m, (var.numpy((h, w, 4)) if var else None)


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 5, 64])
@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_moments(gpu, pass_frames, size, k, gamma):
    frames = pass_frames[size][:k]
    mean, var = run_moments(gpu, frames, gamma)
    exp_mean, exp_var = V.pass_moments(frames, gamma)
    assert_same(mean, exp_mean)
    assert_same(var, exp_var)
    h, w = mean.shape[:2]
    assert (_bits(mean)[h - 2, 1] == 0).all() and (_bits(var)[h - 2, 1] == 0).all()  # masked in all frames
    if k >= 5:
        nx = 63 if w > 64 else w - 1
        assert var[3, nx, 3] == k - 1 - (k // 2 if (nx + 3) % 2 == 1 else 0) and np.isfinite(mean[3, nx]).all()
        assert np.isfinite(mean).all() and np.isfinite(var).all()


def test_moments_one_output_at_a_time_aliasing_and_side_stream(gpu, pass_frames):
    torch = gpu
    for size in SIZES:
        frames = pass_frames[size][:5]
        exp_mean, exp_var = V.pass_moments(frames, 1)
        mean, none = run_moments(torch, frames, 1, want=(True, False))
        assert none is None
        assert_same(mean, exp_mean)
        none, var = run_moments(torch, frames, 1, want=(False, True))
        assert none is None
        assert_same(var, exp_var)
        mean, var = run_moments(torch, frames, 1, alias_mean=True)  # d_mean = frame 0
        assert_same(mean, exp_mean)
        assert_same(var, exp_var)
        mean, var = run_moments(torch, frames, 1, stream=torch.cuda.Stream())
        assert_same(mean, exp_mean)
        assert_same(var, exp_var)


def host_moments(frames, gamma, want):
    """rs_pass_moments with the wanted outputs only (api.pass_moments always asks for both): (mean, var), None where
    not asked for"""
    lib = A.load()
    h, w = frames[0].shape[:2]
    ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    outs = [np.full((h, w, 4), SENTINEL, np.float32) if on else None for on in want]
    rc = lib.rs_pass_moments(ptrs, len(frames), w, h, gamma, *[None if o is None else o.ctypes.data for o in outs])
    assert rc == 0, lib.rs_last_error()
    return outs


def test_moments_host_entry_equals_device_entry(gpu, pass_frames):
    for size in SIZES:
        for k, gamma in ((3, 1), (64, 0)):
            frames = pass_frames[size][:k]
            mean, var = api.pass_moments(frames, bool(gamma))
            dmean, dvar = run_moments(gpu, frames, gamma)
            assert np.array_equal(_bits(mean), _bits(dmean)) and np.array_equal(_bits(var), _bits(dvar))
    # each output alone and both, on the 67 x 5 corner of the frames (no multiple of the block, the NaN and inf pixels
    # inside), K = 3 and 5
    small = [np.ascontiguousarray(f[:5, :67]) for f in pass_frames[SIZES[1]][:5]]
    for k, gamma in ((3, 1), (5, 0)):
        for want in ((True, True), (True, False), (False, True)):
            host, dev = host_moments(small[:k], gamma, want), run_moments(gpu, small[:k], gamma, want)
            for on, a, b in zip(want, host, dev):
                assert (a is None and b is None) if not on else np.array_equal(_bits(a), _bits(b)), (k, want)


# ---------------------------------------------------------------------------------- denoiser ----
@pytest.fixture(scope="module")
def frames():
    """(beauty, var, albedo, normal) of both sizes (computed once, never modified)"""
    out = {}
    for k, (w, h) in enumerate(SIZES):
        beauty, albedo, normal = D.synthetic(w, h, 10 + k)
        out[(w, h)] = (beauty, V.synthetic_variance(w, h, 20 + k, albedo), albedo, normal)
        for a in out[(w, h)]:
            a.setflags(write=False)
    return out


def _kw(st):
    return dict(levels=st.levels, k_color=st.k_color, sigma_normal=st.sigma_normal, sigma_depth=st.sigma_depth)


def run_device(torch, beauty, var, albedo, normal, st, gamma, in_place=False, want_var=True, stream=None):
    """rs_denoise_var_device on copies of the frames: (out, out_var) as numpy. The workspace sits between two guard
    zones that must come back untouched, and the inputs must come back as they went in (beauty and var too, unless in
    place)."""
    h, w = beauty.shape[:2]
    dev = [None if a is None else torch.from_numpy(np.array(a, np.float32)).cuda() for a in (beauty, var, albedo, normal)]
    keep = [None if t is None else t.clone() for t in dev]
    work = Guarded(torch, 4 * w * h * 4)
    out = dev[0] if in_place else torch.full((h, w, 4), SENTINEL, dtype=torch.float32, device="cuda")
    out_var = None if not want_var else (dev[1] if in_place else torch.full((h, w, 4), SENTINEL, dtype=torch.float32,
                                                                            device="cuda"))
    torch.cuda.synchronize()
    ptr = [0 if t is None else t.data_ptr() for t in dev]
    api.denoise_var_device(ptr[0], ptr[1], ptr[2], ptr[3], w, h, out.data_ptr(),
                           0 if out_var is None else out_var.data_ptr(), work.ptr(), st, bool(gamma),
                           0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    work.check()
    written = ([0] if in_place else []) + ([1] if in_place and want_var else [])
    for i, (t, k) in enumerate(zip(dev, keep)):
        assert i in written or t is None or torch.equal(t.view(torch.int32), k.view(torch.int32)), i
    return out.cpu().numpy(), (None if out_var is None else out_var.cpu().numpy())


def check(torch, beauty, var, albedo, normal, st, gamma, **kw):
    out, out_var = run_device(torch, beauty, var, albedo, normal, st, gamma, **kw)
    exp, exp_var = V.denoise_var(beauty, var, albedo, normal, gamma=gamma, **_kw(st))
    assert_same(out, exp)
    if out_var is not None:
        assert_same(out_var, exp_var)
    return out, out_var


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("levels", [1, 3, 5, 8])
@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_levels_and_gamma(gpu, frames, size, levels, gamma):
    """levels 1 (the one launch is first and last), 3, 5 and 8 (step 128: wider than either frame), both gammas"""
    out, out_var = check(gpu, *frames[size], api.DenoiseVarSettings(levels=levels), gamma)
    assert np.isfinite(out).all() and np.isfinite(out_var).all()


@pytest.mark.parametrize("which", ["no_albedo", "no_normal", "neither"])
@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_optional_guides(gpu, frames, size, which):
    beauty, var, albedo, normal = frames[size]
    a = None if which in ("no_albedo", "neither") else albedo
    n = None if which in ("no_normal", "neither") else normal
    for gamma in (0, 1):
        check(gpu, beauty, var, a, n, api.DenoiseVarSettings(), gamma)


@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_mask_nan_and_negative_variance(gpu, frames, size):
    """a masked checkerboard (alpha 0, loud values left in the masked pixels of all four frames), a NaN colour and a
    negative variance on tile edges (x = 63 | 31 and 64 | 32, y = 7 and 4: last / first column and row of a tile): those
    pixels come back bit for bit in both outputs, everything else is the restatement's and finite"""
    w, h = size
    beauty, var, albedo, normal = (a.copy() for a in frames[size])
    yy, xx = np.mgrid[0:h, 0:w]
    masked = (xx + yy) % 2 == 1
    beauty[masked] = [1e6, -3.0, 2.0, 0.0]
    var[masked] = [1e9, 1e9, 1e9, 7.0]
    albedo[masked] = [9.0, 9.0, 9.0, 1.0]
    normal[masked] = [5.0, 5.0, 5.0, 1e3]
    nx, ny = (63 if w > 64 else 31), 7
    vx, vy = (64 if w > 64 else 32), 4
    assert not masked[ny, nx] and not masked[vy, vx]
    beauty[ny, nx, 1] = np.array([0x7FC00123], np.uint32).view(np.float32)[0]
    var[vy, vx, 2] = -1e-4
    st = api.DenoiseVarSettings()
    out, out_var = check(gpu, beauty, var, albedo, normal, st, 1)
    unusable = masked.copy()
    unusable[ny, nx] = unusable[vy, vx] = True
    assert (_bits(out)[unusable] == _bits(beauty)[unusable]).all() and (_bits(out_var)[unusable] == _bits(var)[unusable]).all()
    assert np.isfinite(out[~unusable]).all() and np.isfinite(out_var[~unusable]).all()
    # the all-zero mask convention of rs_render: nothing of the masked values leaked
    beauty[masked] = 0.0
    var[masked] = 0.0
    out0, out_var0 = check(gpu, beauty, var, albedo, normal, st, 1)
    assert (_bits(out0)[masked] == 0).all() and (_bits(out_var0)[masked] == 0).all()
    assert (_bits(out0)[~masked] == _bits(out)[~masked]).all() and (_bits(out_var0)[~masked] == _bits(out_var)[~masked]).all()


@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_in_place_and_no_out_var(gpu, frames, size):
    """d_out == d_beauty with d_out_var == d_var is bitwise the out-of-place result, one level (the launch reads and
    writes the frames) and five; d_out_var NULL leaves the colour as it is"""
    for levels in (1, 5):
        st = api.DenoiseVarSettings(levels=levels)
        a, av = check(gpu, *frames[size], st, 1)
        b, bv = run_device(gpu, *frames[size], st, 1, in_place=True)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(av), _bits(bv))
        c, none = run_device(gpu, *frames[size], st, 1, want_var=False)
        assert none is None and np.array_equal(_bits(a), _bits(c))
        d, none = run_device(gpu, *frames[size], st, 1, in_place=True, want_var=False)
        assert np.array_equal(_bits(a), _bits(d))


def test_side_stream(gpu, frames):
    """enqueued on a non-default stream and read after that stream's synchronise"""
    check(gpu, *frames[SIZES[1]], api.DenoiseVarSettings(), 1, stream=gpu.cuda.Stream())


def test_host_entry_equals_device_entry(gpu, frames):
    for size in SIZES:
        beauty, var, albedo, normal = frames[size]
        st = api.DenoiseVarSettings(levels=4, k_color=1.5)
        for a, n, gamma in ((albedo, normal, 1), (None, normal, 0), (None, None, 1)):
            host, host_var = api.denoise_var(beauty, var, a, n, st, bool(gamma), want_var=True)
            dev, dev_var = run_device(gpu, beauty, var, a, n, st, gamma)
            assert np.array_equal(_bits(host), _bits(dev)) and np.array_equal(_bits(host_var), _bits(dev_var))
            assert np.array_equal(_bits(api.denoise_var(beauty, var, a, n, st, bool(gamma))), _bits(dev))
    # every guide combination with and without out_var, on a 67 x 5 frame: no multiple of the 64 x 4 tile or of the
    # block, two tiles each way
    beauty, albedo, normal = D.synthetic(67, 5, 12)
    var = V.synthetic_variance(67, 5, 22, albedo)
    for a, n, gamma in ((None, None, 0), (albedo, None, 1), (None, normal, 1), (albedo, normal, 0)):
        host, host_var = api.denoise_var(beauty, var, a, n, st, bool(gamma), want_var=True)
        dev, dev_var = run_device(gpu, beauty, var, a, n, st, gamma)
        assert np.array_equal(_bits(host), _bits(dev)) and np.array_equal(_bits(host_var), _bits(dev_var))
        dev, none = run_device(gpu, beauty, var, a, n, st, gamma, want_var=False)
        assert none is None and np.array_equal(_bits(api.denoise_var(beauty, var, a, n, st, bool(gamma))), _bits(dev))


# -------------------------------------------------------------------------------- end to end ----
def test_rendered_passes(gpu):
    """the features scene at 64 x 40, 4 passes of 4 spp, all on the device: render_device_passes into four frames, then
    pass_moments_device, render_features_device and denoise_var_device equal the restatements fed the same GPU pass
    frames; shot_denoised_passes returns the same three frames"""
    torch = gpu
    w, h, passes = 64, 40, 4
    cam, world = scenes.features_scene(w, h)
    photo = cam.take_photo().samples(4).depth(4).seed(5).pass_index(1)
    ds = world.device_scene()

    def frame():
        return torch.full((h, w, 4), SENTINEL, dtype=torch.float32, device="cuda")
    d_pass = [frame() for _ in range(passes)]
    d_mean, d_var, d_albedo, d_normal, d_out = frame(), frame(), frame(), frame(), frame()
    d_work = torch.empty((4 * w * h * 4,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ds.render_device_passes(cam.desc, photo.settings(), [t.data_ptr() for t in d_pass], stream)
    api.pass_moments_device([t.data_ptr() for t in d_pass], w, h, d_mean.data_ptr(), d_var.data_ptr(), True, stream)
    ds.render_features_device(cam.desc, photo.settings(), d_albedo.data_ptr(), d_normal.data_ptr(), stream)
    api.denoise_var_device(d_mean.data_ptr(), d_var.data_ptr(), d_albedo.data_ptr(), d_normal.data_ptr(), w, h,
                           d_out.data_ptr(), 0, d_work.data_ptr(), None, True, stream)
    torch.cuda.synchronize()
    pass_np = [t.cpu().numpy() for t in d_pass]
    exp_mean, exp_var = V.pass_moments(pass_np, 1)
    assert_same(d_mean.cpu().numpy(), exp_mean)
    assert_same(d_var.cpu().numpy(), exp_var)
    assert (exp_var[..., 3] == passes).all() and (exp_var[..., :3] > 0).any()
    exp, _ = V.denoise_var(exp_mean, exp_var, d_albedo.cpu().numpy(), d_normal.cpu().numpy(), gamma=1,
                           **_kw(api.DenoiseVarSettings()))
    got = d_out.cpu().numpy()
    assert_same(got, exp)
    assert not np.array_equal(got, exp_mean)
    den, mean, var = photo.shot_denoised_passes(world, passes)
    assert photo.settings().pass_ == 1
    assert np.array_equal(_bits(mean), _bits(exp_mean)) and np.array_equal(_bits(var), _bits(exp_var))
    assert np.array_equal(_bits(den), _bits(got))


def test_cpp_shot_denoised_passes_on_the_gpu(gpu, tmp_path):
    """tests/cpp/test_denoise_var_api.cpp in its `gpu` mode: raysnail::TakePhotoSettings::shot_denoised_passes (8 x 6,
    3 passes of 4 samples, seed 3, from pass 1, every other pixel masked) writes the frames the Python layer computes
    of the same world"""
    import subprocess
    from test_denoise_var_cpp import build_driver
    exe, out = build_driver(tmp_path), tmp_path / "frames.f32"
    r = subprocess.run([str(exe), "gpu", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
    got = np.fromfile(out, np.float32).reshape(3, 6, 8, 4)
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
    den, mean, var = cam.take_photo().samples(4).seed(3).pass_index(1).shot_denoised_passes(world, 3, EveryOther())
    for f in (den, mean, var):
        assert (f[1::2, 0::2] == 0.0).all()  # masked pixels stay [0,0,0,0] in all three
    assert (var[0::2, 0::2, 3] == 3.0).all()
    for g, e in zip(got, (den, mean, var)):
        assert np.array_equal(_bits(g), _bits(e))
