"""rs_denoise / rs_denoise_device without a GPU: the argument checks that run before anything touches a device, the
properties of the numpy restatement (tests/denoise_ref.py) the GPU is compared against bit for bit, and the
restatement's quality with the default settings on oracle renders."""
import ctypes as C
import math

import numpy as np
import pytest

import denoise_ref as D
import features_ref as FR
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

NAN, INF = float("nan"), float("inf")
P = C.c_void_p


def _defaults():
    st = api.DenoiseSettings()
    return dict(levels=st.levels, sigma_color=st.sigma_color, sigma_normal=st.sigma_normal, sigma_depth=st.sigma_depth)


# ------------------------------------------------------------------------ argument checks ----
def _device(lib, beauty=0x1000, out=0x2000, work=0x3000, w=4, h=3, levels=5, sc=0.3, sn=0.25, sd=0.1, gamma=1):
    """rs_denoise_device with made-up device pointers: a call that fails its checks never dereferences them"""
    return lib.rs_denoise_device(P(beauty), None, None, w, h, levels, sc, sn, sd, gamma, P(out), P(work), None)


def _host(lib, frame, out, w=4, h=3, levels=5, sc=0.3, sn=0.25, sd=0.1, gamma=1):
    return lib.rs_denoise(None if frame is None else frame.ctypes.data, None, None, w, h, levels, sc, sn, sd, gamma,
                          None if out is None else out.ctypes.data)


@pytest.mark.parametrize("kw", [
    dict(beauty=0), dict(out=0), dict(work=0),
    dict(levels=0), dict(levels=9),
    dict(sc=NAN), dict(sc=INF), dict(sc=0.0), dict(sc=-1.0), dict(sc=9e-5), dict(sc=1.0001e4),
    dict(sn=NAN), dict(sn=INF), dict(sn=9e-5), dict(sn=1.0001e4),
    dict(sd=NAN), dict(sd=-INF), dict(sd=9e-5), dict(sd=1.0001e4),
    dict(gamma=2), dict(gamma=-1),
    dict(w=0), dict(h=0), dict(w=0x10000, h=0x8000), dict(w=0xFFFFFFFF, h=0xFFFFFFFF),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_arguments(hip_lib, kw):
    """every invalid case of the header returns RS_E_INVALID with rs_last_error set, from both entry points, no device
    needed (the pointers given to the device entry are never dereferenced)"""
    lib = hip_lib
    assert _device(lib, **kw) == A.RS_E_INVALID
    assert b"denoise" in lib.rs_last_error()
    host_kw = {k: v for k, v in kw.items() if k not in ("beauty", "out", "work")}
    frame = np.full((3, 4, 4), 0.5, np.float32)
    out = np.full((3, 4, 4), 7.0, np.float32)
    if "beauty" in kw:
        assert _host(lib, None, out) == A.RS_E_INVALID
    elif "out" in kw:
        assert _host(lib, frame, None) == A.RS_E_INVALID
    elif "work" not in kw:
        assert _host(lib, frame, out, **host_kw) == A.RS_E_INVALID
        assert b"denoise" in lib.rs_last_error()
    assert (out == 7.0).all()


def test_bounds_of_the_valid_ranges_pass_validation(hip_lib):
    """levels 1 and 8, sigmas 1e-4 and 1e4, W H = 0x7FFFFFFF pass the checks: with a NULL work pointer the call then
    fails on that pointer alone (still before the device), which the error text shows"""
    lib = hip_lib
    for kw in (dict(levels=1), dict(levels=8), dict(sc=1e-4, sn=1e-4, sd=1e-4), dict(sc=1e4, sn=1e4, sd=1e4),
               dict(w=0x7FFFFFFF, h=1), dict(w=1, h=0x7FFFFFFF), dict(gamma=0)):
        assert _device(lib, work=0, **kw) == A.RS_E_INVALID
        assert b"null" in lib.rs_last_error(), (kw, lib.rs_last_error())
    assert _device(lib, work=0, w=0x8000, h=0x10000) == A.RS_E_INVALID
    assert b"large" in lib.rs_last_error()


def test_python_layer_raises(hip_lib):
    frame = np.full((3, 4, 4), 0.5, np.float32)
    for st in (api.DenoiseSettings(levels=0), api.DenoiseSettings(sigma_color=NAN), api.DenoiseSettings(sigma_depth=1e5)):
        with pytest.raises(api.RaysnailError) as e:
            api.denoise(frame, settings=st)
        assert e.value.code == A.RS_E_INVALID
    with pytest.raises(api.RaysnailError) as e:
        api.denoise_device(0x1000, 0, 0, 4, 3, 0x2000, 0)  # no workspace
    assert e.value.code == A.RS_E_INVALID
    st = api.DenoiseSettings()
    assert (st.levels, st.sigma_color, st.sigma_normal, st.sigma_depth) == \
        (A.RS_DENOISE_LEVELS, A.RS_DENOISE_SIGMA_COLOR, A.RS_DENOISE_SIGMA_NORMAL, A.RS_DENOISE_SIGMA_DEPTH)


def test_defaults_are_the_headers():
    """_abi's RS_DENOISE_* are the header's macros"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raysnail_hip.h")).read()
    got = {m.group(1): float(m.group(2)) for m in re.finditer(r"#define (RS_DENOISE_\w+)\s+\(?([0-9.]+)f?\)?", text)}
    assert got == {"RS_DENOISE_LEVELS": float(A.RS_DENOISE_LEVELS), "RS_DENOISE_SIGMA_COLOR": A.RS_DENOISE_SIGMA_COLOR,
                   "RS_DENOISE_SIGMA_NORMAL": A.RS_DENOISE_SIGMA_NORMAL, "RS_DENOISE_SIGMA_DEPTH": A.RS_DENOISE_SIGMA_DEPTH}


def test_host_only_scene_shot_denoised_is_state_error(hip_lib):
    h, lights = api.HittableList(), api.HittableList()
    light = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    h.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    h.add(light)
    lights.add(light)
    world = api.World(h, lights)
    world._scene = api.DeviceScene(world, devices=[])
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(4).height(3).build()
    with pytest.raises(api.RaysnailError) as e:
        cam.take_photo().samples(4).seed(1).shot_denoised(world)
    assert e.value.code == A.RS_E_STATE


# ------------------------------------------------------------- properties of the restatement ----
synthetic = D.synthetic


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_unusable_pixels_pass_through_bit_for_bit():
    """alpha 0 with colour left in it, NaN and Inf colours of several payloads, a NaN in each guide: `out` has the
    beauty frame's bits there, and every other pixel is finite"""
    beauty, albedo, normal = synthetic(37, 23, 1)
    bad = np.zeros((23, 37), bool)
    beauty[2, 3] = [0.5, 0.25, 0.125, 0.0]; bad[2, 3] = True
    beauty[5, 0, 1] = INF; bad[5, 0] = True
    beauty[22, 36, 2] = -INF; bad[22, 36] = True
    beauty[11, 17, 0] = np.array([0x7FC01234], np.uint32).view(np.float32)[0]; bad[11, 17] = True
    albedo[7, 9, 3] = NAN; bad[7, 9] = True
    normal[8, 30, 1] = INF; bad[8, 30] = True
    for gamma in (0, 1):
        out = D.denoise(beauty, albedo, normal, gamma=gamma, **_defaults())
        assert (_bits(out)[bad] == _bits(beauty)[bad]).all()
        assert np.isfinite(out[~bad]).all()
        assert (out[..., 3] == beauty[..., 3]).all()
    # without the guides their NaNs do not matter
    out = D.denoise(beauty, None, None, **_defaults())
    assert np.isfinite(out[7, 9]).all() and np.isfinite(out[8, 30]).all()


def test_one_nan_pixel_in_one_nan_pixel_out():
    beauty, albedo, normal = synthetic(37, 23, 2)
    beauty[10, 20, 1] = NAN
    for guides in ((albedo, normal), (None, None)):
        out = D.denoise(beauty, *guides, **_defaults())
        nan_px = np.isnan(out).any(axis=-1)
        assert nan_px.sum() == 1 and nan_px[10, 20]
        assert (_bits(out)[10, 20] == _bits(beauty)[10, 20]).all()
        # and the neighbours are what they are without that pixel's contribution: not poisoned, not equal either
        clean = beauty.copy()
        clean[10, 20] = [1.0, 1.0, 1.0, 1.0]
        assert not np.array_equal(out[10, 21], D.denoise(clean, *guides, **_defaults())[10, 21])


def test_masked_checkerboard():
    """masked pixels stay [0,0,0,0]; no masked value leaks: the usable pixels' results do not depend on what the
    masked pixels hold (colour or guides)"""
    beauty, albedo, normal = synthetic(37, 23, 3)
    yy, xx = np.mgrid[0:23, 0:37]
    masked = (xx + yy) % 2 == 1
    b0 = beauty.copy(); b0[masked] = 0.0
    a0 = albedo.copy(); a0[masked] = 0.0
    n0 = normal.copy(); n0[masked] = 0.0
    out0 = D.denoise(b0, a0, n0, **_defaults())
    assert (_bits(out0)[masked] == 0).all()
    assert np.isfinite(out0).all()
    # the same mask (alpha 0) with loud values left behind in the masked pixels
    b1 = beauty.copy(); b1[masked, :3] = 1e6; b1[masked, 3] = 0.0
    a1 = albedo.copy(); a1[masked] = [9.0, 9.0, 9.0, 1.0]
    n1 = normal.copy(); n1[masked] = [5.0, 5.0, 5.0, 1e3]
    out1 = D.denoise(b1, a1, n1, **_defaults())
    assert (_bits(out1)[~masked] == _bits(out0)[~masked]).all()
    assert (_bits(out1)[masked] == _bits(b1)[masked]).all()
    # and filtering happened: the usable pixels moved
    assert not np.array_equal(out0[~masked], b0[~masked])


def test_eight_levels_on_a_narrow_frame():
    """levels = 8 (step 128) on 5 x 3 and 1 x 1 frames: every far tap leaves the frame, the output is finite"""
    for w, h in ((5, 3), (1, 1), (3, 200)):
        beauty, albedo, normal = synthetic(w, h, 4)
        kw = dict(_defaults(), levels=8)
        out = D.denoise(beauty, albedo, normal, **kw)
        assert np.isfinite(out).all() and (out[..., 3] == 1.0).all()
    one = np.array([[[0.25, 0.5, 2.0, 1.0]]], np.float32)
    assert np.array_equal(D.denoise(one, None, None, gamma=0, **kw), one)  # h00 c / h00


def test_constant_frame_is_a_fixed_point():
    """a flat colour under flat guides: every weight ratio reproduces the colour (to rounding of c h / h sums)"""
    beauty = np.ones((16, 24, 4), np.float32) * np.float32(0.5)
    beauty[..., 3] = 1.0
    out = D.denoise(beauty, None, None, gamma=0, **_defaults())
    assert np.abs(out[..., :3] - 0.5).max() < 1e-6


# ----------------------------------------------------------------------------- quality ----
def _rmse(a, b):
    e = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return math.sqrt(float(np.mean(e * e)))


@pytest.fixture(scope="module", params=["rtiow", "features"])
def quality_scene(request, oracle_lib):
    """64 x 40: the scene's oracle renders at 16 spp (seed 1) and 1024 spp (seed 2), depth 8, with and without gamma,
    and the 16-spp feature frames from features_ref (computed once, never modified)"""
    from oracle.binding import OracleScene
    if request.param == "rtiow":
        cam, world, _, _ = scenes.rtow_13_1(64, 40, seed=7)
    else:
        cam, world = scenes.features_scene(64, 40)
    orc = OracleScene(world)
    frames = {}
    for gamma in (0, 1):
        lo = cam.take_photo().samples(16).depth(8).seed(1).gamma(bool(gamma))
        hi = cam.take_photo().samples(1024).depth(8).seed(2).gamma(bool(gamma))
        frames[gamma] = (orc.render(cam.desc, lo.settings(), threads=8)[0], orc.render(cam.desc, hi.settings(), threads=8)[0])
    orc2, rec = FR.oracle_scene(world)
    albedo, normal, _ = FR.expected(cam.desc, lo.settings(), FR.oracle_hits(orc2), FR.Albedo(rec))
    return request.param, frames, albedo, normal


@pytest.mark.parametrize("gamma", [0, 1])
def test_default_settings_lower_the_error(quality_scene, gamma):
    """with the default settings the restatement's output is strictly closer (RMSE over rgb) to the 1024-spp frame
    than the 16-spp frame it was given"""
    name, frames, albedo, normal = quality_scene
    noisy, reference = frames[gamma]
    out = D.denoise(noisy, albedo, normal, gamma=gamma, **_defaults())
    before, after = _rmse(noisy, reference), _rmse(out, reference)
    print(f"{name} gamma {gamma}: RMSE 16 spp {before:.5f}, denoised {after:.5f}, ratio {after / before:.3f}")
    assert after < before
