"""rs_pass_robust[_device] on the GPU, bit for bit (uint32 views) against the numpy restatement of the header's
contract (tests/robust_ref.py): test_gpu_denoise_var's seeded pass frames at 37 x 23 (smaller than two blocks' worth
of a row) and 149 x 67 (many blocks with a remainder) with a band of equal frames, a band of exact key ties between
different colours, fireflies planted in one and in two frames and a value whose square overflows added; and one
rendered chain."""
import ctypes as C

import numpy as np
import pytest

import denoise_var_ref as V
import robust_ref as R
from raysnail_amd import _abi as A
from raysnail_amd import api

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (149, 67)]
SENTINEL = -123.25
GUARD = 4096  # elements on each side of a guarded buffer
SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")
KS = [1, 2, 3, 4, 5, 16, 63, 64]
TRIMS = [0.0, 0.1, 0.5, None]
TRIM_IDS = dict(ids=lambda t: "auto" if t is None else f"trim{t}")
OVERFLOW = (6, 5)  # (y, x) of the value whose square overflows


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, exp):
    ok = (_bits(got) == _bits(exp)).all(axis=-1)
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (len(bad), [(int(y), int(x), got[y, x].tolist(), exp[y, x].tolist()) for y, x in bad[:4]])


class Guarded:
    """n elements of device memory between two guard zones that must come back untouched"""

    def __init__(self, torch, n, dtype=None):
        self.torch, self.n = torch, n
        dtype = dtype or torch.float32
        self.fill = SENTINEL if dtype == torch.float32 else 0xA5
        self.arena = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.arena[GUARD:GUARD + n]

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        assert bool((self.arena[:GUARD] == self.fill).all()) and bool((self.arena[GUARD + self.n:] == self.fill).all())

    def numpy(self, shape):
        return self.t.cpu().numpy().reshape(shape)


@pytest.fixture(scope="module")
def pass_frames():
    """per size: 64 seeded pass frames as test_gpu_denoise_var's (frame k masked on a checkerboard for odd k, loud values
    under half of the masks; a NaN pixel in frame 2 at a block edge or the last column, an Inf pixel in frame 0, one
    pixel masked in all frames), and on top of them: rows 9 and 10 equal in all frames; row 12 with the six orders of
    (1, 2, 3) as colours, frame by frame (key 6, or 14 squared: exact ties); 1e4 planted in frame 1 (row 14, where odd
    frames are masked on the checkerboard too) and in frames 0 and 3 (row 15); 1e20 in frame 2 at OVERFLOW. Never
    modified."""
    out = {}
    orders = [(1, 2, 3), (3, 2, 1), (2, 3, 1), (1, 3, 2), (3, 1, 2), (2, 1, 3)]
    for i, (w, h) in enumerate(SIZES):
        rng = np.random.default_rng(60 + i)
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
        for k in range(1, 64):
            frames[k][9:11] = frames[0][9:11]
        for k in range(64):
            frames[k][12, :, :3] = orders[k % 6]
            frames[k][12, :, 3] = 1.0
        frames[1][14, :, :3] = 1e4
        frames[0][15, :, :3] = 1e4
        frames[3][15, :, 0] = 1e4
        nx = 63 if w > 64 else w - 1
        frames[2][3, nx, 1] = np.array([0x7FC00321], np.uint32).view(np.float32)[0]
        frames[0][4, min(64, w - 2), 0] = np.inf
        frames[2][OVERFLOW][1] = 1e20
        for f in frames:
            f.setflags(write=False)
        out[(w, h)] = frames
    return out


def run_robust(torch, frames, gamma, trim, want=(True, True, True), alias_mean=False, stream=None):
    """rs_pass_robust_device on copies of the frames: (mean, var, trimmed) as numpy (None where not asked for). The
    outputs sit between guard zones; the inputs must come back as they went in (but for the frame the mean aliases)."""
    h, w = frames[0].shape[:2]
    dev = [torch.from_numpy(np.array(f, np.float32)).cuda() for f in frames]
    keep = [t.clone() for t in dev]
    mean = Guarded(torch, w * h * 4) if want[0] and not alias_mean else None
    var = Guarded(torch, w * h * 4) if want[1] else None
    trimmed = Guarded(torch, w * h, torch.uint8) if want[2] else None
    torch.cuda.synchronize()
    mean_ptr = dev[0].data_ptr() if alias_mean else (mean.ptr() if mean else 0)
    api.pass_robust_device([t.data_ptr() for t in dev], w, h, mean_ptr, var.ptr() if var else 0,
                           trimmed.ptr() if trimmed else 0, bool(gamma), trim, 0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    for g in (mean, var, trimmed):
        if g is not None:
            g.check()
    for t, k in list(zip(dev, keep))[1 if alias_mean else 0:]:
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    m = dev[0].cpu().numpy() if alias_mean else (mean.numpy((h, w, 4)) if mean else None)
    return m, (var.numpy((h, w, 4)) if var else None), (trimmed.numpy((h, w)) if trimmed else None)


def check(torch, frames, gamma, trim, **kw):
    mean, var, trimmed = run_robust(torch, frames, gamma, trim, **kw)
    exp_mean, exp_var, exp_trimmed = R.pass_robust(frames, gamma, trim)
    if trimmed is not None:
        bad = np.argwhere(trimmed != exp_trimmed)
        assert len(bad) == 0, (len(bad), [(int(y), int(x), int(trimmed[y, x]), int(exp_trimmed[y, x])) for y, x in bad[:4]])
    if mean is not None:
        assert_same(mean, exp_mean)
    if var is not None:
        assert_same(var, exp_var)
    return mean, var, trimmed


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("trim", TRIMS, **TRIM_IDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_robust(gpu, pass_frames, size, k, trim, gamma):
    frames = pass_frames[size][:k]
    mean, var, trimmed = check(gpu, frames, gamma, trim)
    h, w = mean.shape[:2]
    assert (_bits(mean)[h - 2, 1] == 0).all() and (_bits(var)[h - 2, 1] == 0).all() and trimmed[h - 2, 1] == 0
    n = var[..., 3]
    assert (trimmed <= np.where(n >= 2, (n - 2) // 2, 0)).all()
    if trim is None:
        assert (trimmed[9:11] == 0).all()  # equal frames: G = 0 up to rounding
    if k >= 3 and gamma == 1:
        y, x = OVERFLOW
        assert n[y, x] == k - 1 - (k // 2 if (x + y) % 2 == 1 else 0) and np.isfinite(mean[y, x]).all()
    if k >= 16 and trim in (0.5, None):
        # every pixel of rows 14 and 15 has n >= 8 and at most two planted values (row 14's only off the checkerboard,
        # where frame 1 is not masked): they are cut (at trim 0.1 of 16 frames one of two would stay), and what is left
        # is the seeded range [0, 3) (squared under gamma: v <= n 9^2 / 2)
        yy, xx = np.mgrid[0:h, 0:w]
        planted = ((yy == 14) & ((xx + yy) % 2 == 0)) | (yy == 15)
        assert (trimmed[planted] >= 1).all() and (mean[14:16, :, :3] <= 3.0).all()
        assert np.isfinite(var[14:16]).all() and (var[14:16, :, :3] <= 64 * 81.0 / 2).all()


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 5, 64])
@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_trim_zero_is_pass_moments_own_output(gpu, pass_frames, size, k, gamma):
    """trim = 0 against rs_pass_moments_device's two frames of the same device frames, bit for bit on every pixel none
    of whose squares overflow (one pixel of frame 2 under gamma, where the two differ as the header says)"""
    torch = gpu
    frames = pass_frames[size][:k]
    w, h = size
    mean, var, trimmed = run_robust(torch, frames, gamma, 0.0)
    dev = [torch.from_numpy(np.array(f, np.float32)).cuda() for f in frames]
    pm_mean = torch.full((h, w, 4), SENTINEL, dtype=torch.float32, device="cuda")
    pm_var = torch.full((h, w, 4), SENTINEL, dtype=torch.float32, device="cuda")
    api.pass_moments_device([t.data_ptr() for t in dev], w, h, pm_mean.data_ptr(), pm_var.data_ptr(), bool(gamma), 0)
    torch.cuda.synchronize()
    pm_mean, pm_var = pm_mean.cpu().numpy(), pm_var.cpu().numpy()
    assert (trimmed == 0).all()
    if gamma == 1 and k >= 3:
        y, x = OVERFLOW
        assert np.isinf(pm_mean[y, x, 1]) and np.isfinite(mean[y, x]).all() and var[y, x, 3] == pm_var[y, x, 3] - 1
        mean[y, x], var[y, x] = pm_mean[y, x], pm_var[y, x]
    assert_same(mean, pm_mean)
    assert_same(var, pm_var)


def test_each_output_null_aliasing_and_side_stream(gpu, pass_frames):
    torch = gpu
    for size in SIZES:
        frames = pass_frames[size][:5]
        for trim in (0.25, None):
            for want in ((True, False, False), (False, True, False), (True, True, False), (False, True, True),
                         (True, False, True)):
                got = check(torch, frames, 1, trim, want=want)
                assert [g is not None for g in got] == list(want)
            check(torch, frames, 1, trim, alias_mean=True)  # d_mean = frame 0
            check(torch, frames, 1, trim, stream=torch.cuda.Stream())


def host_robust(frames, gamma, trim, want):
    """rs_pass_robust with the wanted outputs only (api.pass_robust always asks for all three): (mean, var, trimmed),
    None where not asked for"""
    lib = A.load()
    h, w = frames[0].shape[:2]
    ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    outs = [np.full((h, w, 4), SENTINEL, np.float32) if on else None for on in want[:2]]
    outs.append(np.full((h, w), 255, np.uint8) if want[2] else None)
    rc = lib.rs_pass_robust(ptrs, len(frames), w, h, gamma, A.RS_ROBUST_TRIM_AUTO if trim is None else trim,
                            *[None if o is None else o.ctypes.data for o in outs])
    assert rc == 0, lib.rs_last_error()
    return outs


def test_host_entry_equals_device_entry(gpu, pass_frames):
    for size in SIZES:
        for k, gamma, trim in ((3, 1, None), (16, 1, 0.1), (64, 0, None)):
            frames = pass_frames[size][:k]
            mean, var, trimmed = api.pass_robust(frames, bool(gamma), trim)
            dmean, dvar, dtrimmed = run_robust(gpu, frames, gamma, trim)
            assert np.array_equal(_bits(mean), _bits(dmean)) and np.array_equal(_bits(var), _bits(dvar))
            assert trimmed.dtype == np.uint8 and np.array_equal(trimmed, dtrimmed)
    # mean only, var only, with and without `trimmed`, on the 67 x 5 corner of the frames (no multiple of the block, the
    # NaN and inf pixels inside), K = 3 and 5: neither a multiple of the rank loop's groups of four
    small = [np.ascontiguousarray(f[:5, :67]) for f in pass_frames[SIZES[1]][:5]]
    for k, gamma, trim in ((3, 1, None), (5, 0, 0.25)):
        for want in ((True, True, True), (True, True, False), (True, False, False), (False, True, True),
                     (True, False, True), (False, True, False)):
            host, dev = host_robust(small[:k], gamma, trim, want), run_robust(gpu, small[:k], gamma, trim, want)
            for on, a, b in zip(want, host, dev):
                assert (a is None and b is None) if not on else np.array_equal(_bits(a), _bits(b)), (k, want)


def test_outputs_through_denoise_var(gpu, pass_frames):
    """the two frames go into rs_denoise_var_device as rs_pass_moments' do: the result is the restatement's on the
    restated frames, and the firefly rows come out finite and below the frames' own range"""
    torch = gpu
    w, h = SIZES[1]
    frames = pass_frames[(w, h)][:16]
    d_frames = [torch.from_numpy(np.array(f, np.float32)).cuda() for f in frames]
    d_mean, d_var, d_out = (torch.full((h, w, 4), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(3))
    d_work = torch.empty((4 * w * h * 4,), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    api.pass_robust_device([t.data_ptr() for t in d_frames], w, h, d_mean.data_ptr(), d_var.data_ptr(), 0, True, None, stream)
    api.denoise_var_device(d_mean.data_ptr(), d_var.data_ptr(), 0, 0, w, h, d_out.data_ptr(), 0, d_work.data_ptr(), None,
                           True, stream)
    torch.cuda.synchronize()
    exp_mean, exp_var, _ = R.pass_robust(frames, 1, None)
    st = api.DenoiseVarSettings()
    exp, _ = V.denoise_var(exp_mean, exp_var, None, None, gamma=1, levels=st.levels, k_color=st.k_color,
                           sigma_normal=st.sigma_normal, sigma_depth=st.sigma_depth)
    got = d_out.cpu().numpy()
    assert_same(got, exp)
    assert np.isfinite(got[14:16]).all() and (got[14:16, :, :3] < 3.01).all()  # (row 12 holds 3.0; a rounding's room)


def test_rendered_chain(gpu):
    """a sphere and a light at 24 x 16, 4 passes of 4 spp: shot_denoised_passes(robust="auto") returns the restatement's
    mean and variance of the GPU's own pass frames, and rs_denoise_var's restatement of those and the photo's feature
    frames; robust=0.0 returns what the default does"""
    w, h, passes = 24, 16, 4
    hl, lights = api.HittableList(), api.HittableList()
    sun = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    hl.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    hl.add(sun)
    lights.add(sun)
    world = api.World(hl, lights)
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(w).height(h).build()
    photo = cam.take_photo().samples(4).depth(4).seed(5).pass_index(1)
    den, mean, var = photo.shot_denoised_passes(world, passes, robust="auto")
    assert photo.settings().pass_ == 1
    frames = [cam.take_photo().samples(4).depth(4).seed(5).pass_index(1 + k).shot(None, world) for k in range(passes)]
    exp_mean, exp_var, exp_trimmed = R.pass_robust(frames, 1, None)
    assert_same(mean, exp_mean)
    assert_same(var, exp_var)
    assert (exp_var[..., 3] == passes).all() and (exp_var[..., :3] > 0).any()
    albedo, normal = photo.shot_features(world)
    st = api.DenoiseVarSettings()
    exp, _ = V.denoise_var(exp_mean, exp_var, albedo, normal, gamma=1, levels=st.levels, k_color=st.k_color,
                           sigma_normal=st.sigma_normal, sigma_depth=st.sigma_depth)
    assert_same(den, exp)
    den0, mean0, var0 = photo.shot_denoised_passes(world, passes, robust=0.0)
    denp, meanp, varp = photo.shot_denoised_passes(world, passes)
    for a, b in ((den0, denp), (mean0, meanp), (var0, varp)):
        assert np.array_equal(_bits(a), _bits(b))
    pm_mean, pm_var = V.pass_moments(frames, 1)
    assert_same(meanp, pm_mean)
    assert_same(varp, pm_var)
