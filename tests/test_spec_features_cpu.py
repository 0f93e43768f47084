"""rs_render_features_specular without a GPU: the fixtures of tests/test_gpu_spec_features.py seen through the
restatement (tests/spec_features_ref.py) and the oracle alone, the argument and state checks that run before anything
touches a device, and the Python wrappers on a host-only scene."""
import ctypes as C

import numpy as np
import pytest

import features_ref as F
import spec_features_ref as R
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes


# ---------------------------------------------------------------- the restatement and its fixtures ----
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_zero_bounces_is_the_first_hit_frame(oracle_lib, name):
    """max_specular = 0: the restatement's frames are features_ref.expected's, bit for bit"""
    cam, _, photo, orc, alb, bouncer = R.fixture(name)
    ch = R.fixture_chains(name, 0) if 0 in R.FIXTURES[name][4] else \
        R.chains(cam.desc, photo.settings(), F.oracle_hits(orc), alb, 0, bouncer=bouncer)
    exp_a, exp_n, _ = F.expected(cam.desc, photo.settings(), F.oracle_hits(orc), alb)
    got_a, got_n = ch.frames()
    assert F.same_bits(got_a, exp_a).all() and F.same_bits(got_n, exp_n).all()
    assert (ch.calls == 1).all() and (ch.bounces == 0).all()
    assert ch.count(R.TERMINAL_AFTER) == ch.count(R.ESCAPE) == 0


def test_centre_line_through_a_glass_sphere(oracle_lib):
    """one ray along a glass sphere's centre line: normal incidence refracts straight on, twice, and ends on the
    diffuse sphere behind; depth is the sum of the three t1 (4 + 2 + 2), the albedo the diffuse colour under the
    glass's tint twice, the normal the diffuse sphere's"""
    hl, lights = api.HittableList(), api.HittableList()
    hl.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Dielectric(scenes.C32(0.5, 1.0, 0.25), 1.5).reflect_curve(api.Glass())))
    hl.add(api.Sphere((0.0, 0.0, -4.0), 1.0, api.Lambertian(scenes.C32(0.5, 0.25, 1.0))))
    light = api.Sphere((0.0, 40.0, 0.0), 5.0, api.DiffuseLight(scenes.C32(1.0, 1.0, 1.0)))
    lights.add(light)
    hl.add(light)
    orc, rec = R.oracle_scene(api.World(hl, lights))
    alb = F.Albedo(rec)
    ray = np.array([[0.0, 0.0, 5.0, 0.0, 0.0, -1.0, 0.0]])
    hit_fn = F.oracle_hits(orc)
    t1 = [hit_fn(np.array([[0.0, 0.0, z, 0.0, 0.0, -1.0, 0.0]]))[0, 1] for z in (5.0, 1.0, -1.0)]
    assert t1 == [4.0, 2.0, 2.0]
    vals, ending, bounces, tir, calls = R.trace(ray, hit_fn, alb, R.Bouncer(alb), 4)
    assert ending[0] == R.TERMINAL_AFTER and bounces[0] == 2 and tir[0] == 0 and calls[0] == 3
    assert vals[0].tolist() == [0.5 * 0.5 * 0.5, 0.25, 0.25 * 0.25, 1.0, 0.0, 0.0, 1.0, t1[0] + t1[1] + t1[2]]
    # with a budget of one bounce the chain stops on the glass's far side, from inside: the limit
    vals, ending, bounces, _, calls = R.trace(ray, hit_fn, alb, R.Bouncer(alb), 1)
    assert ending[0] == R.LIMIT and bounces[0] == 1 and calls[0] == 2
    assert vals[0].tolist() == [0.5 * 0.5, 1.0, 0.25 * 0.25, 1.0, 0.0, 0.0, 1.0, t1[0] + t1[1]]


def test_glass_twin_ignores_the_rng(oracle_lib):
    """the Dielectric twin registered without `glass` scatters the same ray under every rng seed, on refracting and on
    totally reflecting hits; the fixture's own Glass material does not (its Fresnel coin), which is why the twin is
    used"""
    cam, _, photo, orc, alb, bouncer = R.fixture("tir")
    rays = F.camera_rays(cam.desc, photo.settings(), [(x, y) for y in range(cam.desc.height) for x in (0, 5, 10, 15)])
    rays = rays.reshape(-1, 7)
    recs = F.oracle_hits(orc)(rays)
    assert (recs[:, 0] == 1.0).all()
    n_tir = 0
    for ray, r in zip(rays, recs):
        mid, d = bouncer.resolve(r)
        assert d.kind == A.RS_MAT_DIELECTRIC and d.glass == 1
        outs = [bouncer.scatter(mid, ray, r, seed) for seed in (1, 2, 3, 12345, 2 ** 63 + 9)]
        assert all(o[:12] == outs[0][:12] for o in outs)
        n_tir += int(bouncer(ray, r)[2])
    assert 0 < n_tir < len(rays)
    # the Glass original under the same seeds: at least one hit's ray depends on the draw
    g = A.rs_material_desc()
    g.kind, g.glass, g.refractive, g.multiplier, g.mix_p = A.RS_MAT_DIELECTRIC, 1, 1.5, 1.0, 0.5
    g.texture.kind = A.RS_TEX_SOLID
    out = C.c_int32()
    assert alb.lib.orc_material(alb.h, C.byref(g), C.byref(out)) == 0
    bouncer.twin[-7] = out.value
    try:
        differs = 0
        for ray, r in zip(rays, recs):
            outs = [bouncer.scatter(-7, ray, r, seed) for seed in range(1, 65)]  # (reflect_prob is 0.04 and up)
            differs += int(any(o[9:12] != outs[0][9:12] for o in outs))
        assert differs > 0
    finally:
        del bouncer.twin[-7]


def test_fixture_coverage(oracle_lib):
    """Stated before the GPU ran, from the oracle alone: across the fixtures every ending of a chain occurs (terminal
    at k = 0, terminal at k >= 1, escape, limit), at least one bounce is a total internal reflection, and in each
    fixture at least 10 % of the hitting samples bounce at least once. Metal's below-surface rejection is not
    required: the oracle's normals face the ray (dot(d, n) < 0), so dot(reflect(d, n), n) = -dot(d, n) > 0 on every
    hit it can report, and no fixture reaches it."""
    total = np.zeros(6, int)
    tirs = 0
    for name, (_, _, _, _, budgets, _) in sorted(R.FIXTURES.items()):
        for m in budgets:
            ch = R.fixture_chains(name, m)
            counts = [ch.count(e) for e in range(6)]
            hit = ch.hitting()
            share = float((ch.bounces[hit] >= 1).mean())
            print(f"{name} max_specular {m}: " + ", ".join(f"{R.ENDINGS[e]} {counts[e]}" for e in range(6)) +
                  f"; total internal reflections {int(ch.tir.sum())}; bouncing share of hitting samples {share:.3f}; "
                  f"World::hit calls per sample {ch.calls.mean():.3f}")
            assert (ch.calls <= m + 1).all()
            if m > 0:
                total += counts
                tirs += int(ch.tir.sum())
                assert share >= 0.10, (name, m, share)
    assert all(total[e] > 0 for e in (R.TERMINAL_FIRST, R.TERMINAL_AFTER, R.ESCAPE, R.LIMIT)), total.tolist()
    assert tirs >= 1
    assert total[R.METAL_REJECTED] == 0


def test_special_fixtures_end_as_designed(oracle_lib):
    """the hall of mirrors: every sample hits and runs to the limit at every budget; inside the glass sphere: every
    sample bounces, and the limit (total internal reflection for good), the escape and the terminal hit all occur; the
    rich scene's chains through the glass end on the medium's Isotropic boundary hit"""
    for m in R.FIXTURES["hall"][4]:
        ch = R.fixture_chains("hall", m)
        assert (ch.ending == R.LIMIT).all() and (ch.calls == m + 1).all() and (ch.bounces == m).all()
    ch = R.fixture_chains("tir", 8)
    assert (ch.bounces >= 1).all()
    assert min(ch.count(R.LIMIT), ch.count(R.ESCAPE), ch.count(R.TERMINAL_AFTER)) > 0
    assert int(ch.tir[ch.ending == R.LIMIT].min()) >= 1
    cam, _, photo, orc, alb, bouncer = R.fixture("rich")
    rays = F.camera_rays(cam.desc, photo.settings(), [(x, y) for y in range(cam.desc.height) for x in range(cam.desc.width)])
    rays = rays.reshape(-1, 7)
    hit_fn = F.oracle_hits(orc)
    first = hit_fn(rays)
    glass = [i for i, r in enumerate(first) if r[0] == 1.0 and bouncer.resolve(r)[1] is not None
             and bouncer.resolve(r)[1].kind == A.RS_MAT_DIELECTRIC]
    assert len(glass) > 50
    second = hit_fn(np.array([bouncer(rays[i], first[i])[0] for i in glass]))
    kinds = [bouncer.resolve(r)[1].kind for r in second if r[0] == 1.0]
    assert kinds.count(A.RS_MAT_ISOTROPIC) > len(glass) // 2


# ---------------------------------------------------------------- argument and state checks ----
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
    h.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Metal(api.Color(0.5, 0.5, 0.5))))
    h.add(light)
    lights.add(light)
    world = api.World(h, lights)
    world._scene = api.DeviceScene(world, devices=[])
    return world


def test_argument_checks_come_before_the_state_check(hip_lib):
    """max_specular = 17 and both outputs NULL are RS_E_INVALID before commit and on a host-only scene alike; 16 with
    an output passes the argument checks and meets RS_E_STATE; null scene, camera or settings are RS_E_INVALID"""
    lib = hip_lib
    assert lib.rs_abi_version() == 6
    cam, st = _cam_st()
    a = np.full((3, 4, 4), 7.0, np.float32)
    n = np.full((3, 4, 4), 7.0, np.float32)
    ap, np_ = a.ctypes.data, n.ctypes.data
    ds = _host_only_world().device_scene()
    fresh = _scene(lib)
    for s in (fresh, ds.handle):
        assert lib.rs_render_features_specular(s, C.byref(cam), C.byref(st), None, 17, ap, np_, None) == A.RS_E_INVALID
        assert b"max_specular" in lib.rs_last_error()
        assert lib.rs_render_features_specular_device(s, C.byref(cam), C.byref(st), None, 17, C.c_void_p(0x1000),
                                                      C.c_void_p(0x2000), None, None) == A.RS_E_INVALID
        assert lib.rs_render_features_specular(s, C.byref(cam), C.byref(st), None, 2, None, None, None) == A.RS_E_INVALID
        assert b"null" in lib.rs_last_error()
        assert lib.rs_render_features_specular_device(s, C.byref(cam), C.byref(st), None, 2, None, None, None,
                                                      None) == A.RS_E_INVALID
        for m in (0, 1, 16):
            assert lib.rs_render_features_specular(s, C.byref(cam), C.byref(st), None, m, ap, np_, None) == A.RS_E_STATE
            assert lib.rs_render_features_specular(s, C.byref(cam), C.byref(st), None, m, ap, None, None) == A.RS_E_STATE
            assert lib.rs_render_features_specular_device(s, C.byref(cam), C.byref(st), None, m, C.c_void_p(0x1000),
                                                          C.c_void_p(0x2000), None, None) == A.RS_E_STATE
    assert lib.rs_render_features_specular(None, C.byref(cam), C.byref(st), None, 1, ap, None, None) == A.RS_E_INVALID
    assert lib.rs_render_features_specular(fresh, None, C.byref(st), None, 1, ap, None, None) == A.RS_E_INVALID
    assert lib.rs_render_features_specular_device(fresh, C.byref(cam), None, None, 1, None, np_, None, None) == A.RS_E_INVALID
    assert (a == 7.0).all() and (n == 7.0).all()
    lib.rs_scene_destroy(fresh)


def test_python_wrappers_on_a_host_only_scene(hip_lib):
    """DeviceScene.render_features / render_features_device and TakePhotoSettings.shot_features / shot_denoised /
    shot_denoised_passes take the new parameter and raise the library's codes"""
    world = _host_only_world()
    ds = world.device_scene()
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(4).height(3).build()
    photo = cam.take_photo().samples(4).seed(1)
    for call, code in ((lambda: ds.render_features(cam.desc, photo.settings(), max_specular=3), A.RS_E_STATE),
                       (lambda: ds.render_features(cam.desc, photo.settings(), max_specular=17), A.RS_E_INVALID),
                       (lambda: ds.render_features_device(cam.desc, photo.settings(), 0x1000, 0x2000, stats=False,
                                                          max_specular=2), A.RS_E_STATE),
                       (lambda: ds.render_features_device(cam.desc, photo.settings(), 0x1000, 0x2000, stats=False,
                                                          max_specular=99), A.RS_E_INVALID),
                       (lambda: photo.shot_features(world, None, 2), A.RS_E_STATE),
                       (lambda: photo.shot_features(world, max_specular=17), A.RS_E_INVALID),
                       (lambda: photo.shot_denoised(world, guide_specular=2), A.RS_E_STATE),
                       (lambda: photo.shot_denoised_passes(world, 2, guide_specular=2), A.RS_E_STATE)):
        with pytest.raises(api.RaysnailError) as e:
            call()
        assert e.value.code == code
