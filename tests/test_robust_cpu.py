"""rs_pass_robust[_device] without a GPU: the numpy restatement (tests/robust_ref.py) the GPU is compared against bit
for bit -- against rs_pass_moments' restatement at trim 0, against a float64 computation of the same statistics, its
trim counts at the edges of the contract, its tie-breaking, a planted firefly -- and the argument checks that run before
anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import denoise_var_ref as V
import robust_ref as R
from raysnail_amd import _abi as A
from raysnail_amd import api

NAN, INF = float("nan"), float("inf")
P = C.c_void_p
EPS = 2.0 ** -23  # f32 epsilon (twice the unit roundoff: the bounds below count roundings generously)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def seeded_frames(k, w=19, h=11, seed=3):
    """k frames of rgb in [0, 3), odd frames masked on a checkerboard, a NaN, an Inf and an everywhere-masked pixel"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (xx + yy) % 2 == 1
    frames = []
    for i in range(k):
        f = np.ones((h, w, 4), np.float32)
        f[..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(3.0)
        if i % 2 == 1:
            f[board] = [5.0, 5.0, 5.0, 0.0] if i % 4 == 1 else 0.0
        f[h - 2, 1] = 0.0
        frames.append(f)
    frames[min(2, k - 1)][3, w - 1, 1] = np.nan
    frames[0][4, 2, 0] = np.inf
    return frames


# ------------------------------------------------------------------------------ the restatement ----
@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 16, 64])
def test_trim_zero_is_pass_moments_bit_for_bit(k, gamma):
    frames = seeded_frames(k)
    mean, var, trimmed = R.pass_robust(frames, gamma, 0.0)
    exp_mean, exp_var = V.pass_moments(frames, gamma)
    assert np.array_equal(_bits(mean), _bits(exp_mean)) and np.array_equal(_bits(var), _bits(exp_var))
    assert (trimmed == 0).all()


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("trim", [0.0, 0.1, 0.25, 0.5, None], ids=lambda t: f"trim={t}")
@pytest.mark.parametrize("k", [2, 5, 16, 64])
def test_against_float64(k, trim, gamma):
    """The trim counts are integers and taken from the restatement; the statistics are then compared. Tolerances from n
    and the f32 epsilon, X the largest value (3, or 9 when the frames are squared). The sum of the h kept values has
    partial sums below h X, each addition within eps h X / 2: h^2 eps X / 2, which the division by h brings to
    h eps X / 2; the division's own rounding and the squares' (eps X / 2 each) stay below eps X together: the mean is
    within (n + 2) eps X (the sqrt of gamma is undone in f64 first, which adds its eps X). mw likewise, over n values.
    d = w - mw is then within (n + 3) eps X, d d within 2 X (n + 3) eps X + eps X^2 <= (2 n + 7) eps X^2; the n
    additions of Q add n^2 eps X^2 / 2: Q within n (3 n + 7) eps X^2, and v within that over h (h - 1) plus the
    division's eps v."""
    frames = seeded_frames(k)
    X = 9.0 if gamma else 3.0
    mean, var, trimmed = R.pass_robust(frames, gamma, trim)
    t = trimmed.astype(np.int64)
    mu, v = R.pass_robust_f64(frames, gamma, t)
    n = var[..., 3].astype(np.int64)
    some, two = n >= 1, n >= 2
    lin = mean[..., :3].astype(np.float64)
    lin = lin * lin if gamma else lin
    assert some.any() and two.any()
    assert (np.abs(lin[some] - mu[some]) <= (n[some] + 2)[..., None] * EPS * X + (2 * EPS * X if gamma else 0)).all()
    h = n - 2 * t
    assert (h[two] >= 2).all()
    bound = (n * (3 * n + 7) * EPS * X * X)[two] / (h * (h - 1.0))[two]
    assert (np.abs(var[..., :3][two] - v[two]) <= bound[..., None] + EPS * v[two]).all()
    assert (var[..., :3][~two] == 0).all() and (mean[~some] == 0).all() and (trimmed[~some] == 0).all()


def _column(keys, alpha=None):
    """K frames of one pixel whose red channel is keys[k] (green and blue 0)"""
    frames = []
    for i, s in enumerate(keys):
        f = np.zeros((1, 1, 4), np.float32)
        f[0, 0, 0] = s
        f[0, 0, 3] = 1.0 if alpha is None else alpha[i]
        frames.append(f)
    return frames


@pytest.mark.parametrize("n,expected", [(1, (0, 0, 0)), (2, (0, 0, 0)), (3, (0, 0, 0)), (4, (0, 1, 1)), (5, (0, 1, 1)),
                                        (64, (0, 16, 31))])
def test_fixed_trim_counts(n, expected):
    """t = min((n - 2) / 2, floor(trim n)) for trim 0, 0.25 and 0.5, with n counted over the contributing frames only
    (every third frame here is masked, up to the 64 the entry takes)"""
    rng = np.random.default_rng(n)
    keys, alpha = [], []
    while sum(alpha) < n:
        masked = len(keys) % 3 == 2 and len(keys) + (n - sum(alpha)) < 64
        keys.append(float(rng.random()) + 0.5)
        alpha.append(0.0 if masked else 1.0)
    for trim, t in zip((0.0, 0.25, 0.5), expected):
        mean, var, trimmed = R.pass_robust(_column(keys, alpha), 0, trim)
        assert var[0, 0, 3] == n and trimmed[0, 0] == t, (trim, trimmed)
        if n >= 2:
            assert np.isfinite(var).all() and n - 2 * t >= 2


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 64])
def test_auto_trim_counts(n):
    t_max = (n - 2) // 2 if n >= 2 else 0
    for gamma in (0, 1):
        # all keys equal: G = 0
        assert R.pass_robust(_column([0.7] * n), gamma)[2][0, 0] == 0
        # all keys zero: S_s = 0
        mean, var, trimmed = R.pass_robust(_column([0.0] * n), gamma)
        assert trimmed[0, 0] == 0 and (mean[0, 0] == [0, 0, 0, 1]).all() and var[0, 0, 3] == n
        # one non-zero key among zeros, wherever it stands: G = (n - 1) / n
        for at in {0, n // 2, n - 1}:
            keys = [0.0] * n
            keys[at] = 3.0
            mean, var, trimmed = R.pass_robust(_column(keys), gamma)
            assert trimmed[0, 0] == t_max
            if t_max >= 1:  # the one key is cut: the mean is the zeros'
                assert (mean[0, 0] == [0, 0, 0, 1]).all() and (var[0, 0, :3] == 0).all()


def test_ties_are_broken_by_frame_index():
    """four frames of key 6 in four colours, trim 0.25: frame 0 is the lowest and frame 3 the highest whatever their
    colours; the mean is frames 1 and 2's, the Winsorised values are frames 1, 1, 2, 2"""
    colours = [(1.0, 2.0, 3.0), (3.0, 2.0, 1.0), (2.0, 2.0, 2.0), (6.0, 0.0, 0.0)]
    frames = [np.array([[list(c) + [1.0]]], np.float32) for c in colours]
    mean, var, trimmed = R.pass_robust(frames, 0, 0.25)
    assert trimmed[0, 0] == 1
    assert (mean[0, 0] == [2.5, 2.0, 1.5, 1.0]).all()
    # w = [f1, f1, f2, f2]: mw = (2.5, 2, 1.5), Q = 4 * 0.25 in r and b, v = Q / (2 * 1)
    assert (var[0, 0] == [0.5, 0.0, 0.5, 4.0]).all()
    # the same colours in reverse frame order: now the old frame 3 is the lowest
    mean_r, var_r, _ = R.pass_robust(frames[::-1], 0, 0.25)
    assert (mean_r[0, 0] == [2.5, 2.0, 1.5, 1.0]).all()  # (frames 2 and 1 again: the middle pair)
    mean_s, _, _ = R.pass_robust([frames[1], frames[0], frames[3], frames[2]], 0, 0.25)
    assert (mean_s[0, 0] == [3.5, 1.0, 1.5, 1.0]).all()  # frames 0 and 3 of the original are the middle pair now
    # -0.0 and +0.0 are the same key
    z = _column([0.0, -0.0, 0.0, -0.0, 5.0])
    assert R.pass_robust(z, 0, 0.25)[2][0, 0] == 1 and R.pass_robust(z, 0, 0.25)[0][0, 0, 0] == 0


@pytest.mark.parametrize("gamma", [0, 1])
def test_planted_firefly(gamma):
    """16 frames of value 1 with a seeded +-5 % jitter, frame 7 set to 1000 on a checkerboard. The plain mean is above
    60 there; the auto trim and trim 0.125 leave every pixel's mean within the jitter's range. The auto trim cuts
    (trimmed >= 1) exactly on the checkerboard. The fixed trim's count is floor(0.125 * 16) = 2 on every pixel: the
    contract makes a fixed trim independent of the values, so `exactly on the checkerboard` can only be asked of the
    auto trim."""
    w, h = 24, 16
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (xx + yy) % 2 == 1
    frames = []
    for k in range(16):
        f = np.ones((h, w, 4), np.float32)
        f[..., :3] = np.float32(1.0) + np.float32(0.05) * (np.float32(2.0) * rng.random((h, w, 3), dtype=np.float32)
                                                           - np.float32(1.0))
        frames.append(f)
    frames[7][board, :3] = 1000.0
    plain, _ = V.pass_moments(frames, gamma)
    assert (plain[board][:, :3] > 60).all()
    for trim in (None, 0.125):
        mean, var, trimmed = R.pass_robust(frames, gamma, trim)
        assert (mean[..., :3] >= 0.95).all() and (mean[..., :3] <= 1.05).all()
        # every Winsorised value is a jittered one: Q <= 16 range^2 with range <= 1.05^2 - 0.95^2 = 0.2, h (h - 1) >= 2
        assert np.isfinite(var).all() and (var[..., :3] <= 16 * 0.2 * 0.2 / 2).all()
        if trim is None:
            assert ((trimmed >= 1) == board).all()
        else:
            assert (trimmed == 2).all()


# ------------------------------------------------------------------------------ argument checks ----
def _device(lib, frames=(0x1000, 0x2000), n=None, w=4, h=3, gamma=1, trim=0.1, mean=0x3000, var=0x4000, trimmed=0x5000,
            table=True):
    """rs_pass_robust_device with made-up device pointers: a call that fails its checks never dereferences them"""
    ptrs = (P * max(1, len(frames)))(*[P(f or None) for f in frames]) if table else None
    return lib.rs_pass_robust_device(ptrs, len(frames) if n is None else n, w, h, gamma, trim, P(mean or None),
                                     P(var or None), P(trimmed or None), None)


@pytest.mark.parametrize("kw", [
    dict(table=False), dict(frames=(0x1000, 0)), dict(frames=(0, 0x1000)),
    dict(frames=(), n=0), dict(frames=(0x1000,) * 65),
    dict(gamma=2), dict(gamma=-1),
    dict(w=0), dict(h=0), dict(w=0x10000, h=0x8000), dict(w=0xFFFFFFFF, h=0xFFFFFFFF),
    dict(mean=0, var=0),
    dict(trim=NAN), dict(trim=INF), dict(trim=-INF), dict(trim=-0.5), dict(trim=-2.0), dict(trim=0.50001), dict(trim=1.0),
    dict(trim=-1e-6),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_arguments(hip_lib, kw):
    """every invalid case of the header returns RS_E_INVALID with rs_last_error set, from both entry points, no device
    needed; the host entry's outputs stay untouched"""
    lib = hip_lib
    assert _device(lib, **kw) == A.RS_E_INVALID
    assert b"pass_robust" in lib.rs_last_error()
    frame = np.full((3, 4, 4), 0.5, np.float32)
    mean, var = np.full((3, 4, 4), 7.0, np.float32), np.full((3, 4, 4), 7.0, np.float32)
    trimmed = np.full((3, 4), 7, np.uint8)
    n_frames = len(kw["frames"]) if "frames" in kw else 2
    host = [frame.ctypes.data if ("frames" not in kw or f) else None for f in kw.get("frames", (1, 1))]
    ptrs = (P * max(1, n_frames))(*[P(f) for f in host]) if kw.get("table", True) else None
    both_null = "mean" in kw
    rc = lib.rs_pass_robust(ptrs, kw.get("n", n_frames), kw.get("w", 4), kw.get("h", 3), kw.get("gamma", 1),
                            kw.get("trim", 0.1), None if both_null else mean.ctypes.data,
                            None if both_null else var.ctypes.data, trimmed.ctypes.data)
    assert rc == A.RS_E_INVALID
    assert b"pass_robust" in lib.rs_last_error()
    assert (mean == 7.0).all() and (var == 7.0).all() and (trimmed == 7).all()


def test_bounds_of_the_valid_ranges_pass_validation(hip_lib):
    """n_frames 1 and 64, gamma 0, W H = 0x7FFFFFFF, trim 0, -0.0, 0.5 and auto, a NULL trimmed pass every other check:
    with both frame outputs NULL the call then fails on that alone (the last check, still before the device)"""
    lib = hip_lib
    for kw in (dict(frames=(0x1000,)), dict(frames=(0x1000,) * 64), dict(gamma=0), dict(w=0x7FFFFFFF, h=1),
               dict(w=1, h=0x7FFFFFFF), dict(trim=0.0), dict(trim=-0.0), dict(trim=0.5), dict(trim=A.RS_ROBUST_TRIM_AUTO),
               dict(trimmed=0)):
        assert _device(lib, mean=0, var=0, **kw) == A.RS_E_INVALID
        assert b"both outputs" in lib.rs_last_error(), (kw, lib.rs_last_error())
    for kw in (dict(mean=0), dict(var=0), dict(mean=0, trimmed=0)):
        assert _device(lib, frames=(0x1000, 0), **kw) == A.RS_E_INVALID
        assert b"null frame" in lib.rs_last_error()


def test_python_layer_raises(hip_lib):
    frame = np.full((3, 4, 4), 0.5, np.float32)
    for bad in (0.6, -0.1, NAN, "median", True):
        with pytest.raises(api.RaysnailError) as e:
            api.pass_robust([frame, frame], trim=bad)
        assert e.value.code == A.RS_E_INVALID
        with pytest.raises(api.RaysnailError) as e:
            api.pass_robust_device([0x1000, 0x2000], 4, 3, 0x3000, 0x4000, trim=bad)
        assert e.value.code == A.RS_E_INVALID
    for frames in ([frame] * 65, []):
        with pytest.raises(api.RaysnailError) as e:
            api.pass_robust(frames)
        assert e.value.code == A.RS_E_INVALID
    with pytest.raises(api.RaysnailError) as e:
        api.pass_robust_device([0x1000, 0x2000], 4, 3, 0, 0)  # no output
    assert e.value.code == A.RS_E_INVALID
    import raysnail_amd
    for name in ("pass_robust", "pass_robust_device"):
        assert getattr(raysnail_amd, name) is getattr(api, name)
    assert A.RS_ROBUST_TRIM_AUTO == -1.0
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raysnail_hip.h")).read()
    assert float(re.search(r"#define\s+RS_ROBUST_TRIM_AUTO\s+\(\(float\)([-0-9.]+)\)", text).group(1)) == A.RS_ROBUST_TRIM_AUTO


def test_shot_denoised_passes_refuses_a_bad_robust_before_rendering(hip_lib):
    hl, lights = api.HittableList(), api.HittableList()
    hl.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    world = api.World(hl, lights)
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(8).height(6).build()
    for bad in (0.75, -1.0, "gini", NAN):
        with pytest.raises(api.RaysnailError) as e:
            cam.take_photo().samples(1).shot_denoised_passes(world, 2, robust=bad)
        assert e.value.code == A.RS_E_INVALID and "trim" in str(e.value)
