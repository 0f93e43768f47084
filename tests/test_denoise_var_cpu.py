"""rs_pass_moments / rs_denoise_var (and their _device forms) without a GPU: the argument checks that run before
anything touches a device, the properties of the numpy restatements (tests/denoise_var_ref.py) the GPU is compared
against bit for bit, and the restatement's quality with the default settings on oracle renders."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import denoise_ref as D
import denoise_var_ref as V
from raysnail_amd import _abi as A
from raysnail_amd import api

NAN, INF = float("nan"), float("inf")
P = C.c_void_p


def _defaults():
    st = api.DenoiseVarSettings()
    return dict(levels=st.levels, k_color=st.k_color, sigma_normal=st.sigma_normal, sigma_depth=st.sigma_depth)


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


# --------------------------------------------------------------- argument checks: pass moments ----
def _pm_device(lib, frames=(0x1000, 0x2000), n=None, w=4, h=3, gamma=1, mean=0x3000, var=0x4000, table=True):
    """rs_pass_moments_device with made-up device pointers: a call that fails its checks never dereferences them"""
    ptrs = (P * max(1, len(frames)))(*[P(f or None) for f in frames]) if table else None
    return lib.rs_pass_moments_device(ptrs, len(frames) if n is None else n, w, h, gamma, P(mean or None), P(var or None), None)


@pytest.mark.parametrize("kw", [
    dict(table=False), dict(frames=(0x1000, 0)), dict(frames=(0, 0x1000)),
    dict(frames=(), n=0), dict(frames=(0x1000,) * 65),
    dict(gamma=2), dict(gamma=-1),
    dict(w=0), dict(h=0), dict(w=0x10000, h=0x8000), dict(w=0xFFFFFFFF, h=0xFFFFFFFF),
    dict(mean=0, var=0),
], ids=_ids)
def test_pass_moments_invalid_arguments(hip_lib, kw):
    """every invalid case of the header returns RS_E_INVALID with rs_last_error set, from both entry points, no device
    needed; the host entry's outputs stay untouched"""
    lib = hip_lib
    assert _pm_device(lib, **kw) == A.RS_E_INVALID
    assert b"pass_moments" in lib.rs_last_error()
    frame = np.full((3, 4, 4), 0.5, np.float32)
    mean, var = np.full((3, 4, 4), 7.0, np.float32), np.full((3, 4, 4), 7.0, np.float32)
    n_frames = len(kw["frames"]) if "frames" in kw else 2
    host = [frame.ctypes.data if ("frames" not in kw or f) else None for f in kw.get("frames", (1, 1))]
    ptrs = (P * max(1, n_frames))(*[P(f) for f in host]) if kw.get("table", True) else None
    both_null = "mean" in kw
    rc = lib.rs_pass_moments(ptrs, kw.get("n", n_frames), kw.get("w", 4), kw.get("h", 3), kw.get("gamma", 1),
                             None if both_null else mean.ctypes.data, None if both_null else var.ctypes.data)
    assert rc == A.RS_E_INVALID
    assert b"pass_moments" in lib.rs_last_error()
    assert (mean == 7.0).all() and (var == 7.0).all()


def test_pass_moments_bounds_of_the_valid_ranges_pass_validation(hip_lib):
    """n_frames 1 and 64, gamma 0, W H = 0x7FFFFFFF, one output NULL pass every other check: with both outputs NULL the
    call then fails on that alone (the last check, still before the device), which the error text shows"""
    lib = hip_lib
    for kw in (dict(frames=(0x1000,)), dict(frames=(0x1000,) * 64), dict(gamma=0), dict(w=0x7FFFFFFF, h=1),
               dict(w=1, h=0x7FFFFFFF)):
        assert _pm_device(lib, mean=0, var=0, **kw) == A.RS_E_INVALID
        assert b"both outputs" in lib.rs_last_error(), (kw, lib.rs_last_error())
    assert _pm_device(lib, mean=0, var=0, w=0x8000, h=0x10000) == A.RS_E_INVALID
    assert b"large" in lib.rs_last_error()
    # either output alone is enough: the one remaining complaint is the null frame pointer
    for kw in (dict(mean=0), dict(var=0)):
        assert _pm_device(lib, frames=(0x1000, 0), **kw) == A.RS_E_INVALID
        assert b"null frame" in lib.rs_last_error()


# ------------------------------------------------------------------ argument checks: denoiser ----
def _dv_device(lib, beauty=0x1000, var=0x1800, out=0x2000, out_var=0x2800, work=0x3000, w=4, h=3, levels=5, kc=3.0,
               sn=0.25, sd=0.1, gamma=1):
    return lib.rs_denoise_var_device(P(beauty or None), P(var or None), None, None, w, h, levels, kc, sn, sd, gamma,
                                     P(out or None), P(out_var or None), P(work or None), None)


def _dv_host(lib, frame, var, out, out_var, w=4, h=3, levels=5, kc=3.0, sn=0.25, sd=0.1, gamma=1):
    ptr = [None if a is None else a.ctypes.data for a in (frame, var, out, out_var)]
    return lib.rs_denoise_var(ptr[0], ptr[1], None, None, w, h, levels, kc, sn, sd, gamma, ptr[2], ptr[3])


@pytest.mark.parametrize("kw", [
    dict(beauty=0), dict(var=0), dict(out=0), dict(work=0),
    dict(levels=0), dict(levels=9),
    dict(kc=NAN), dict(kc=INF), dict(kc=0.0), dict(kc=-1.0), dict(kc=9e-5), dict(kc=1.0001e4),
    dict(sn=NAN), dict(sn=INF), dict(sn=9e-5), dict(sn=1.0001e4),
    dict(sd=NAN), dict(sd=-INF), dict(sd=9e-5), dict(sd=1.0001e4),
    dict(gamma=2), dict(gamma=-1),
    dict(w=0), dict(h=0), dict(w=0x10000, h=0x8000), dict(w=0xFFFFFFFF, h=0xFFFFFFFF),
], ids=_ids)
def test_denoise_var_invalid_arguments(hip_lib, kw):
    """every invalid case returns RS_E_INVALID with rs_last_error set (rs_denoise's texts), from both entry points, no
    device needed; the host entry's outputs stay untouched"""
    lib = hip_lib
    assert _dv_device(lib, **kw) == A.RS_E_INVALID
    assert b"denoise" in lib.rs_last_error()
    host_kw = {k: v for k, v in kw.items() if k not in ("beauty", "var", "out", "work")}
    frame = np.full((3, 4, 4), 0.5, np.float32)
    var = np.full((3, 4, 4), 0.01, np.float32)
    out, out_var = np.full((3, 4, 4), 7.0, np.float32), np.full((3, 4, 4), 7.0, np.float32)
    if "beauty" in kw:
        assert _dv_host(lib, None, var, out, out_var) == A.RS_E_INVALID
    elif "var" in kw:
        assert _dv_host(lib, frame, None, out, out_var) == A.RS_E_INVALID
    elif "out" in kw:
        assert _dv_host(lib, frame, var, None, out_var) == A.RS_E_INVALID
    elif "work" not in kw:
        assert _dv_host(lib, frame, var, out, out_var, **host_kw) == A.RS_E_INVALID
        assert b"denoise" in lib.rs_last_error()
    assert (out == 7.0).all() and (out_var == 7.0).all()


def test_denoise_var_bounds_of_the_valid_ranges_pass_validation(hip_lib):
    """levels 1 and 8, k_color and sigmas 1e-4 and 1e4, W H = 0x7FFFFFFF, a NULL out_var pass the checks: with a NULL
    work pointer the call then fails on that pointer alone (still before the device), which the error text shows"""
    lib = hip_lib
    for kw in (dict(levels=1), dict(levels=8), dict(kc=1e-4, sn=1e-4, sd=1e-4), dict(kc=1e4, sn=1e4, sd=1e4),
               dict(w=0x7FFFFFFF, h=1), dict(w=1, h=0x7FFFFFFF), dict(gamma=0), dict(out_var=0)):
        assert _dv_device(lib, work=0, **kw) == A.RS_E_INVALID
        assert b"null" in lib.rs_last_error(), (kw, lib.rs_last_error())
    assert _dv_device(lib, work=0, w=0x8000, h=0x10000) == A.RS_E_INVALID
    assert b"large" in lib.rs_last_error()


def test_python_layer_raises(hip_lib):
    frame = np.full((3, 4, 4), 0.5, np.float32)
    var = np.full((3, 4, 4), 0.01, np.float32)
    for st in (api.DenoiseVarSettings(levels=0), api.DenoiseVarSettings(k_color=NAN), api.DenoiseVarSettings(sigma_depth=1e5)):
        with pytest.raises(api.RaysnailError) as e:
            api.denoise_var(frame, var, settings=st)
        assert e.value.code == A.RS_E_INVALID
    with pytest.raises(api.RaysnailError) as e:
        api.denoise_var_device(0x1000, 0x1800, 0, 0, 4, 3, 0x2000, 0, 0)  # no workspace
    assert e.value.code == A.RS_E_INVALID
    with pytest.raises(api.RaysnailError) as e:
        api.pass_moments([frame] * 65)
    assert e.value.code == A.RS_E_INVALID
    with pytest.raises(api.RaysnailError) as e:
        api.pass_moments([])
    assert e.value.code == A.RS_E_INVALID
    with pytest.raises(api.RaysnailError) as e:
        api.pass_moments_device([0x1000, 0x2000], 4, 3, 0, 0)  # no output
    assert e.value.code == A.RS_E_INVALID
    import raysnail_amd
    for name in ("pass_moments", "pass_moments_device", "DenoiseVarSettings", "denoise_var", "denoise_var_device"):
        assert getattr(raysnail_amd, name) is getattr(api, name)


def test_defaults_are_the_headers():
    """_abi's RS_DENOISE_VAR_* and DenoiseVarSettings' defaults are the header's macros"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raysnail_hip.h")).read()
    got = {m.group(1): float(m.group(2)) for m in re.finditer(r"#define (RS_DENOISE_VAR_\w+)\s+\(\((?:uint32_t|float)\)([0-9.e-]+)\)", text)}
    assert got == {"RS_DENOISE_VAR_LEVELS": float(A.RS_DENOISE_VAR_LEVELS), "RS_DENOISE_VAR_K_COLOR": A.RS_DENOISE_VAR_K_COLOR,
                   "RS_DENOISE_VAR_EPS": A.RS_DENOISE_VAR_EPS}
    st = api.DenoiseVarSettings()
    assert (st.levels, st.k_color, st.sigma_normal, st.sigma_depth) == \
        (A.RS_DENOISE_VAR_LEVELS, A.RS_DENOISE_VAR_K_COLOR, A.RS_DENOISE_SIGMA_NORMAL, A.RS_DENOISE_SIGMA_DEPTH)
    assert np.float32(A.RS_DENOISE_VAR_EPS) == V.EPS


def test_host_only_scene_shot_denoised_passes(hip_lib):
    """on a world committed for no device the first pass's render is RS_E_STATE; passes = 1 is RS_E_INVALID before that"""
    h, lights = api.HittableList(), api.HittableList()
    light = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    h.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    h.add(light)
    lights.add(light)
    world = api.World(h, lights)
    world._scene = api.DeviceScene(world, devices=[])
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(4).height(3).build()
    photo = cam.take_photo().samples(4).seed(1).pass_index(2)
    with pytest.raises(api.RaysnailError) as e:
        photo.shot_denoised_passes(world, 4)
    assert e.value.code == A.RS_E_STATE
    assert photo.settings().pass_ == 2  # the photo's own pass index is back
    for passes in (1, 0):
        with pytest.raises(api.RaysnailError) as e:
            photo.shot_denoised_passes(world, passes)
        assert e.value.code == A.RS_E_INVALID


# ------------------------------------------------------------- the moments' restatement ----
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pass_frames(w, h, k, seed):
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(k):
        f = np.ones((h, w, 4), np.float32)
        f[..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(2.0)
        frames.append(f)
    return frames


def test_moments_of_one_frame():
    """K = 1: without gamma the frame comes back exactly; with it sqrt(x x) to an ulp; the variance is 0 with n = 1"""
    (f,) = _pass_frames(9, 7, 1, 1)
    mean, var = V.pass_moments([f], gamma=0)
    assert (_bits(mean) == _bits(f)).all()
    assert (_bits(var[..., :3]) == 0).all() and (var[..., 3] == 1.0).all()
    mean, var = V.pass_moments([f], gamma=1)
    assert np.allclose(mean, f, rtol=2e-7, atol=0) and (var[..., :3] == 0).all() and (var[..., 3] == 1.0).all()


def test_moments_masked_everywhere_and_nan_in_one_frame():
    frames = _pass_frames(9, 7, 5, 2)
    for f in frames:
        f[3, 4] = 0.0                        # masked in every frame
    frames[1][2, 2] = [0.5, 9.0, 0.25, 0.0]  # masked in one frame only, colour left in it
    frames[2][5, 6, 1] = NAN                 # NaN in one of five
    frames[4][0, 0, 2] = INF
    others = [f for k, f in enumerate(frames) if k != 2]
    for gamma in (0, 1):
        mean, var = V.pass_moments(frames, gamma)
        assert (_bits(mean)[3, 4] == 0).all() and (_bits(var)[3, 4] == 0).all()
        assert var[5, 6, 3] == 4.0 and var[2, 2, 3] == 4.0 and var[0, 0, 3] == 4.0 and var[1, 1, 3] == 5.0
        m4, v4 = V.pass_moments(others, gamma)
        assert (_bits(mean)[5, 6] == _bits(m4)[5, 6]).all() and (_bits(var)[5, 6] == _bits(v4)[5, 6]).all()
        assert np.isfinite(mean).all() and np.isfinite(var).all() and (mean[..., 3][var[..., 3] > 0] == 1.0).all()
        # against float64: the mean, and the variance of the mean s^2 / n
        x = np.stack([f[1, 1, :3].astype(np.float64) for f in frames])
        x = x * x if gamma else x
        assert np.allclose(var[1, 1, :3], x.var(axis=0, ddof=1) / 5, rtol=1e-5)
        assert np.allclose(mean[1, 1, :3], np.sqrt(x.mean(axis=0)) if gamma else x.mean(axis=0), rtol=1e-6)


def test_moments_of_identical_frames():
    """identical frames whose sum is exact (values on a 2^-8 grid below 1, K = 4): variance exactly 0"""
    rng = np.random.default_rng(3)
    f = np.ones((7, 9, 4), np.float32)
    f[..., :3] = rng.integers(0, 256, (7, 9, 3)).astype(np.float32) / np.float32(256.0)
    for gamma in (0, 1):
        mean, var = V.pass_moments([f, f.copy(), f.copy(), f.copy()], gamma)
        assert (_bits(var[..., :3]) == 0).all() and (var[..., 3] == 4.0).all()
        assert (mean == f).all()  # (x x on that grid is exact in f32, and its sqrt is x)


# ------------------------------------------------------------ the denoiser's restatement ----
def _frames(w, h, seed):
    beauty, albedo, normal = D.synthetic(w, h, seed)
    return beauty, V.synthetic_variance(w, h, seed + 100, albedo), albedo, normal


def test_unusable_pixels_pass_through_bit_for_bit():
    """alpha 0, NaN / Inf colour, NaN / negative / Inf variance, a NaN in each guide: both outputs have their input's
    bits there, and every other pixel is finite"""
    beauty, var, albedo, normal = _frames(37, 23, 1)
    bad = np.zeros((23, 37), bool)
    beauty[2, 3] = [0.5, 0.25, 0.125, 0.0]; bad[2, 3] = True
    beauty[5, 0, 1] = INF; bad[5, 0] = True
    beauty[11, 17, 0] = np.array([0x7FC01234], np.uint32).view(np.float32)[0]; bad[11, 17] = True
    var[4, 30, 2] = np.array([0x7FC00055], np.uint32).view(np.float32)[0]; bad[4, 30] = True
    var[15, 8, 0] = -1e-3; bad[15, 8] = True
    var[22, 36, 1] = INF; bad[22, 36] = True
    var[9, 9, 3] = NAN  # var.w is not read: carried over, the pixel stays usable
    albedo[7, 9, 3] = NAN; bad[7, 9] = True
    normal[8, 30, 1] = INF; bad[8, 30] = True
    for gamma in (0, 1):
        out, out_var = V.denoise_var(beauty, var, albedo, normal, gamma=gamma, **_defaults())
        assert (_bits(out)[bad] == _bits(beauty)[bad]).all() and (_bits(out_var)[bad] == _bits(var)[bad]).all()
        assert np.isfinite(out[~bad]).all() and np.isfinite(out_var[~bad][:, :3]).all()
        assert (_bits(out[..., 3]) == _bits(beauty[..., 3])).all() and (_bits(out_var[..., 3]) == _bits(var[..., 3])).all()
        assert (out_var[~bad][:, :3] >= 0).all()
    out, out_var = V.denoise_var(beauty, var, None, None, **_defaults())
    assert np.isfinite(out[7, 9]).all() and np.isfinite(out[8, 30]).all()


def test_one_nan_pixel_in_one_nan_pixel_out():
    beauty, var, albedo, normal = _frames(37, 23, 2)
    beauty[10, 20, 1] = NAN
    for guides in ((albedo, normal), (None, None)):
        out, out_var = V.denoise_var(beauty, var, *guides, **_defaults())
        nan_px = np.isnan(out).any(axis=-1)
        assert nan_px.sum() == 1 and nan_px[10, 20] and not np.isnan(out_var).any()
        assert (_bits(out)[10, 20] == _bits(beauty)[10, 20]).all() and (_bits(out_var)[10, 20] == _bits(var)[10, 20]).all()
        clean = beauty.copy()
        clean[10, 20] = [1.0, 1.0, 1.0, 1.0]
        assert not np.array_equal(out[10, 21], V.denoise_var(clean, var, *guides, **_defaults())[0][10, 21])


def test_masked_checkerboard():
    """no masked value leaks: the usable pixels' colours and variances do not depend on what the masked pixels hold
    (colour, variance or guides)"""
    beauty, var, albedo, normal = _frames(37, 23, 3)
    yy, xx = np.mgrid[0:23, 0:37]
    masked = (xx + yy) % 2 == 1
    b0 = beauty.copy(); b0[masked] = 0.0
    v0 = var.copy(); v0[masked] = 0.0
    a0 = albedo.copy(); a0[masked] = 0.0
    n0 = normal.copy(); n0[masked] = 0.0
    out0, ov0 = V.denoise_var(b0, v0, a0, n0, **_defaults())
    assert (_bits(out0)[masked] == 0).all() and (_bits(ov0)[masked] == 0).all()
    assert np.isfinite(out0).all() and np.isfinite(ov0).all()
    b1 = beauty.copy(); b1[masked, :3] = 1e6; b1[masked, 3] = 0.0
    v1 = var.copy(); v1[masked] = [1e9, 1e9, 1e9, 7.0]
    a1 = albedo.copy(); a1[masked] = [9.0, 9.0, 9.0, 1.0]
    n1 = normal.copy(); n1[masked] = [5.0, 5.0, 5.0, 1e3]
    out1, ov1 = V.denoise_var(b1, v1, a1, n1, **_defaults())
    assert (_bits(out1)[~masked] == _bits(out0)[~masked]).all() and (_bits(ov1)[~masked] == _bits(ov0)[~masked]).all()
    assert (_bits(out1)[masked] == _bits(b1)[masked]).all() and (_bits(ov1)[masked] == _bits(v1)[masked]).all()
    assert not np.array_equal(out0[~masked], b0[~masked])


def test_eight_levels_on_a_narrow_frame():
    for w, h in ((5, 3), (1, 1), (3, 200)):
        beauty, var, albedo, normal = _frames(w, h, 4)
        kw = dict(_defaults(), levels=8)
        out, out_var = V.denoise_var(beauty, var, albedo, normal, **kw)
        assert np.isfinite(out).all() and np.isfinite(out_var).all() and (out[..., 3] == 1.0).all()
    one = np.array([[[0.25, 0.5, 2.0, 1.0]]], np.float32)
    one_var = np.array([[[0.5, 0.25, 0.125, 4.0]]], np.float32)
    out, out_var = V.denoise_var(one, one_var, None, None, gamma=0, **kw)
    assert np.array_equal(out, one) and np.array_equal(out_var, one_var)  # h00 c / h00, (h00 h00) v / (h00 h00)


def test_constant_frame_is_a_fixed_point_and_its_variance_shrinks():
    beauty = np.ones((16, 24, 4), np.float32) * np.float32(0.5)
    beauty[..., 3] = 1.0
    var = np.full((16, 24, 4), 0.01, np.float32)
    var[..., 3] = 4.0
    out, out_var = V.denoise_var(beauty, var, None, None, gamma=0, **_defaults())
    assert np.abs(out[..., :3] - 0.5).max() < 1e-6
    assert (out_var[..., :3] < var[..., :3]).all() and (out_var[..., :3] > 0).all()


# ----------------------------------------------------------------------------- quality ----
def _rmse(a, b):
    e = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return math.sqrt(float(np.mean(e * e)))


@pytest.fixture(scope="module", params=["rtiow", "features"])
def quality_scene(request, oracle_lib):
    """the scene's oracle pass frames, 1024-spp references and 16-spp feature frames (computed once, never modified)"""
    return (request.param,) + V.quality_inputs(request.param)


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("cell", V.QUALITY_CELLS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_default_settings_beat_the_mean_and_the_fixed_sigma_filter(quality_scene, cell, gamma):
    """K passes of N spp: with the default settings the restatement's output is strictly closer (RMSE over rgb) to the
    1024-spp frame than the passes' mean, and than rs_denoise with its defaults on that mean -- also where the fixed
    sigma over-smooths (32 spp and more on RTIOW)"""
    name, frames, albedo, normal = quality_scene
    reference = frames[gamma]["ref"]
    mean, var = V.pass_moments(frames[gamma][cell], gamma)
    out, _ = V.denoise_var(mean, var, albedo, normal, gamma=gamma, **_defaults())
    fixed = D.denoise(mean, albedo, normal, gamma=gamma)
    e_mean, e_fixed, e_out = _rmse(mean, reference), _rmse(fixed, reference), _rmse(out, reference)
    print(f"{name} {cell[0]}x{cell[1]} gamma {gamma}: RMSE mean {e_mean:.5f}, rs_denoise {e_fixed:.5f} "
          f"({e_fixed / e_mean:.3f}), rs_denoise_var {e_out:.5f} ({e_out / e_mean:.3f} of the mean, "
          f"{e_out / e_fixed:.3f} of rs_denoise)")
    assert e_out < e_mean
    assert e_out < e_fixed
