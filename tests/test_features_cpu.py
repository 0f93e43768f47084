"""rs_render_features / rs_render_features_device without a GPU: the argument and state checks that run before
anything touches a device, the ABI version, and the Python wrappers on a host-only scene."""
import ctypes as C

import numpy as np
import pytest

from raysnail_amd import _abi as A
from raysnail_amd import api


def _scene(lib):
    h = C.c_void_p()
    assert lib.rs_scene_create(C.byref(h)) == 0
    return h


def _cam_st():
    cam = A.rs_camera_desc()
    cam.width, cam.height = 4, 3
    st = A.rs_render_settings()
    st.samples, st.depth = 4, 1
    return cam, st


def _host_only_world():
    h, lights = api.HittableList(), api.HittableList()
    light = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    h.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Lambertian(api.Color(0.5, 0.5, 0.5))))
    h.add(light)
    lights.add(light)
    world = api.World(h, lights)
    world._scene = api.DeviceScene(world, devices=[])
    return world


def test_abi_version_is_still_6(hip_lib):
    assert hip_lib.rs_abi_version() == 6 == A.ABI_VERSION
    assert A.KERNEL_NAMES[4] == "k_features"


def test_both_outputs_null_is_invalid(hip_lib):
    """before commit and on a host-only committed scene alike: the argument check comes first"""
    lib = hip_lib
    cam, st = _cam_st()
    s = _scene(lib)
    assert lib.rs_render_features(s, C.byref(cam), C.byref(st), None, None, None, None) == A.RS_E_INVALID
    assert lib.rs_render_features_device(s, C.byref(cam), C.byref(st), None, None, None, None, None) == A.RS_E_INVALID
    assert b"null" in lib.rs_last_error()
    lib.rs_scene_destroy(s)
    ds = _host_only_world().device_scene()
    assert lib.rs_render_features(ds.handle, C.byref(cam), C.byref(st), None, None, None, None) == A.RS_E_INVALID


def test_null_scene_camera_or_settings_is_invalid(hip_lib):
    lib = hip_lib
    cam, st = _cam_st()
    out = np.zeros((3, 4, 4), np.float32)
    s = _scene(lib)
    assert lib.rs_render_features(None, C.byref(cam), C.byref(st), None, out.ctypes.data, None, None) == A.RS_E_INVALID
    assert lib.rs_render_features(s, None, C.byref(st), None, out.ctypes.data, None, None) == A.RS_E_INVALID
    assert lib.rs_render_features_device(s, C.byref(cam), None, None, None, out.ctypes.data, None, None) == A.RS_E_INVALID
    lib.rs_scene_destroy(s)


def test_before_commit_is_state_error(hip_lib):
    lib = hip_lib
    cam, st = _cam_st()
    a = np.full((3, 4, 4), 7.0, np.float32)
    n = np.full((3, 4, 4), 7.0, np.float32)
    s = _scene(lib)
    assert lib.rs_render_features(s, C.byref(cam), C.byref(st), None, a.ctypes.data, n.ctypes.data, None) == A.RS_E_STATE
    assert lib.rs_render_features(s, C.byref(cam), C.byref(st), None, a.ctypes.data, None, None) == A.RS_E_STATE
    # (device pointers are never dereferenced: the state check comes before any device work)
    assert lib.rs_render_features_device(s, C.byref(cam), C.byref(st), None, C.c_void_p(0x1000), C.c_void_p(0x2000), None,
                                         None) == A.RS_E_STATE
    assert (a == 7.0).all() and (n == 7.0).all()
    lib.rs_scene_destroy(s)


def test_host_only_scene_is_state_error(hip_lib):
    """DeviceScene.render_features, render_features_device and TakePhotoSettings.shot_features on a scene committed
    for no device raise the library's RS_E_STATE"""
    world = _host_only_world()
    ds = world.device_scene()
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(4).height(3).build()
    photo = cam.take_photo().samples(4).seed(1)
    with pytest.raises(api.RaysnailError) as e:
        ds.render_features(cam.desc, photo.settings())
    assert e.value.code == A.RS_E_STATE
    with pytest.raises(api.RaysnailError) as e:
        ds.render_features_device(cam.desc, photo.settings(), 0x1000, 0x2000, stats=False)
    assert e.value.code == A.RS_E_STATE
    with pytest.raises(api.RaysnailError) as e:
        photo.shot_features(world)
    assert e.value.code == A.RS_E_STATE
    cam.desc.width = 0  # validate_render's checks apply: an empty image
    with pytest.raises(api.RaysnailError) as e:
        ds.render_features(cam.desc, photo.settings(), albedo=np.zeros((3, 0, 4), np.float32), want=(True, False))
    assert e.value.code == A.RS_E_STATE  # (state before shape, as rs_render)
