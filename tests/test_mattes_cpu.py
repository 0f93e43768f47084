"""rs_render_mattes and rs_matte_extract without a GPU: the restatement (tests/mattes_ref.py) on hand-made id multisets,
the special fixtures of tests/test_gpu_mattes.py seen through the oracle alone, the argument checks that run before
anything touches a device, the exported symbols and the Python wrappers on a host-only scene."""
import ctypes as C
import random

import numpy as np
import pytest

import features_ref as F
import mattes_ref as M
import spec_features_ref as R
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

BG, EMPTY = A.RS_MATTE_ID_BACKGROUND, A.RS_MATTE_ID_EMPTY


# ---------------------------------------------------------------- the restatement on hand-made multisets ----
def test_constants_are_the_headers():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raysnail_hip.h")).read()
    assert "#define RS_MATTE_MAX_RANKS     8" in hdr and A.RS_MATTE_MAX_RANKS == 8
    assert "#define RS_MATTE_MAX_DISTINCT  64" in hdr and A.RS_MATTE_MAX_DISTINCT == 64
    assert "#define RS_MATTE_ID_BACKGROUND ((int32_t)-2)" in hdr and BG == -2
    assert "#define RS_MATTE_ID_EMPTY      ((int32_t)0x80000000)" in hdr and EMPTY == -2 ** 31
    assert "#define RS_KERNEL_MATTES     5" in hdr and A.RS_KERNEL_MATTES == 5
    assert np.int32(EMPTY) == np.iinfo(np.int32).min


def test_ranking_and_ties():
    """count descending; equal counts by id ascending, signed: the background (-2) and no material (-1) before 0"""
    ids = [7, 3, 3, 7, 5, -1, -1, BG, BG, 9]
    i, c, o = M.rank_ids(ids, 8)
    assert i.tolist() == [BG, -1, 3, 7, 5, 9, EMPTY, EMPTY] and o == 0
    assert c.tolist() == [np.float32(0.2)] * 4 + [np.float32(0.1)] * 2 + [0.0, 0.0]
    assert i.dtype == np.int32 and c.dtype == np.float32
    i, c, _ = M.rank_ids(ids, 1)
    assert i.tolist() == [BG] and c.tolist() == [np.float32(0.2)]
    i, c, _ = M.rank_ids([4, 4, 4, 2], 4)
    assert i.tolist() == [4, 2, EMPTY, EMPTY] and c.tolist() == [0.75, 0.25, 0.0, 0.0]
    assert np.signbit(c[2:]).sum() == 0  # +0.0


def test_one_id_and_coverage_rounding():
    """one id: coverage exactly 1; the coverage is the f64 quotient rounded to f32 once"""
    for n in (1, 4, 121):
        i, c, o = M.rank_ids([12] * n, 4)
        assert i.tolist() == [12, EMPTY, EMPTY, EMPTY] and c.tolist() == [1.0, 0.0, 0.0, 0.0] and o == 0
    _, c, _ = M.rank_ids([1] * 40 + [2] * 81, 2)
    assert c.tolist() == [np.float32(81.0 / 121.0), np.float32(40.0 / 121.0)]


def test_exactly_64_and_65_distinct_ids():
    """64 distinct ids: all kept, no overflow. 65: the largest id (signed) is dropped whatever its count, the others
    keep their full counts, overflow is 1"""
    ids64 = list(range(-2, 62))
    i, c, o = M.rank_ids(ids64 + [61, 61], 8)
    assert o == 0 and i.tolist() == [61] + list(range(-2, 5)) and c[0] == np.float32(3.0 / 66.0)
    # id 62 has the most samples and is still the one that goes
    ids65 = ids64 + [62] * 10 + [5, 5]
    i, c, o = M.rank_ids(ids65, 8)
    assert o == 1 and 62 not in i.tolist()
    assert i.tolist() == [5, -2, -1, 0, 1, 2, 3, 4]
    assert c[0] == np.float32(3.0 / 76.0) and c[1] == np.float32(1.0 / 76.0)  # N stays the pixel's sample count
    # a negative id is smaller than every handle: the background survives, a large handle does not
    i, _, o = M.rank_ids([BG] + list(range(1000, 1064)), 1)
    assert o == 1
    kept = M.rank_ids([BG] + list(range(1000, 1064)), 8)[0].tolist()
    assert kept == [BG] + list(range(1000, 1007))
    i, _, _ = M.rank_ids([BG] + list(range(1000, 1064)) + [1063] * 5, 1)
    assert i.tolist() == [BG]  # 1063, the 65th, is gone with its six samples


def test_shuffles_do_not_matter():
    """the result depends on the multiset alone, with and without overflow"""
    rnd = random.Random(7)
    for distinct, n in ((5, 64), (64, 100), (65, 130), (90, 121)):
        ids = [rnd.randrange(-2, distinct - 2) for _ in range(n - distinct)] + list(range(-2, distinct - 2))
        ref = M.rank_ids(ids, 8)
        assert ref[2] == (1 if distinct > 64 else 0)
        for _ in range(5):
            rnd.shuffle(ids)
            got = M.rank_ids(ids, 8)
            assert got[0].tolist() == ref[0].tolist() and got[1].tolist() == ref[1].tolist() and got[2] == ref[2]


def test_no_samples():
    """N = 0: every rank of every pixel is (empty, +0.0), overflow 0"""
    i, c, o = M.layers(np.zeros((6, 0), np.int64), 3, 2, 4)
    assert i.shape == (2, 3, 4) and (i == EMPTY).all() and (c == 0.0).all() and not np.signbit(c).any() and (o == 0).all()


def test_matte_extract_restatement():
    """the sum in rank order from +0.0 over the wanted ids, rounded per addition; empty ranks never count, even when
    the empty id is asked for"""
    ids = np.array([[[3, 5, BG, EMPTY], [5, EMPTY, EMPTY, EMPTY]]], np.int32)
    third = np.float32(1.0 / 3.0)
    cov = np.array([[[0.5, third, np.float32(1.0 / 6.0), 0.0], [1.0, 7.0, 7.0, 7.0]]], np.float32)
    assert M.matte_extract(ids, cov, [3]).tolist() == [[0.5, 0.0]]
    assert M.matte_extract(ids, cov, [5]).tolist() == [[third, 1.0]]
    assert M.matte_extract(ids, cov, [5, 3]).tolist() == [[np.float32(np.float32(0.5) + third), 1.0]]
    assert M.matte_extract(ids, cov, [3, 5, BG])[0, 0] == np.float32(np.float32(np.float32(0.5) + third) + np.float32(1.0 / 6.0))
    assert M.matte_extract(ids, cov, [77]).tolist() == [[0.0, 0.0]]
    assert M.matte_extract(ids, cov, [EMPTY, 5]).tolist() == [[third, 1.0]]
    assert M.matte_extract(ids, cov, [BG]).dtype == np.float32
    # rounding per addition, in rank order: 1 + 2^-24 + 2^-24 stays 1 in that order
    e = np.float32(2.0 ** -24)
    ids = np.array([[[1, 2, 3]]], np.int32)
    assert M.matte_extract(ids, np.array([[[1.0, e, e]]], np.float32), [1, 2, 3])[0, 0] == np.float32(1.0)
    assert M.matte_extract(ids, np.array([[[e, e, 1.0]]], np.float32), [1, 2, 3])[0, 0] > np.float32(1.0)


# ---------------------------------------------------------------- the fixtures, from the oracle alone ----
def _oracle_ids(cam, world, st, max_specular):
    orc, rec = R.oracle_scene(world)
    alb = F.Albedo(rec)
    return M.frame_ids(cam.desc, st, F.oracle_hits(orc), R.Bouncer(alb), max_specular)


def test_lattice_fixture_overflows_one_pixel(oracle_lib):
    """stated before the GPU ran: pixel (1, 0) of the sphere lattice has 71 distinct ids (overflow 1, the background
    and the 63 smallest handles kept), pixel (0, 0) has 31 (overflow 0, more than 8 ranks), the others the background"""
    cam, world, photo, mats = M.lattice_scene()
    ids, calls = _oracle_ids(cam, world, photo.settings(), 0)
    assert ids.shape == (6, 100) and (calls == 1).all()
    distinct = [len(set(ids[p].tolist())) for p in range(6)]
    assert distinct == [31, 71, 1, 1, 1, 1]
    li, lc, lo = M.layers(ids, 3, 2, 8)
    assert lo.tolist() == [[0, 1, 0], [0, 0, 0]]
    assert li[0, 1, 0] == BG and lc[0, 1, 0] == np.float32(0.3) and (lc[0, 1, 1:] == np.float32(0.01)).all()
    kept = sorted(set(ids[1].tolist()))[:64]
    assert li[0, 1, 1:].tolist() == kept[1:8] and kept[0] == BG and max(set(ids[1].tolist())) > kept[-1]
    assert li[0, 0, 0] == BG and lc[0, 0, 0] == np.float32(0.7)
    assert (li[1] == np.array([BG] + [EMPTY] * 7)).all() and (lc[1, :, 0] == 1.0).all()
    # the handles are the creation order
    ds = api.DeviceScene(world, devices=[])
    assert [ds.material_id(m) for m in mats] == list(range(100))


@pytest.mark.parametrize("left_first", [True, False])
def test_tie_fixture(oracle_lib, left_first):
    """the middle column's pixels are halved exactly between the two rects at sqrt_spp 2 and 4, and rank 0 goes to the
    material created first (the smaller handle), whichever side it is on"""
    cam, world, left, right = M.tie_scene(left_first)
    ds = api.DeviceScene(world, devices=[])
    first, second = (left, right) if left_first else (right, left)
    assert ds.material_id(first) == 0 and ds.material_id(second) == 1
    for samples in (4, 16):
        ids, _ = _oracle_ids(cam, world, cam.take_photo().samples(samples).seed(1).settings(), 0)
        li, lc, lo = M.layers(ids, 5, 3, 2)
        assert (li[:, 2] == np.array([0, 1])).all() and (lc[:, 2] == 0.5).all() and (lo == 0).all()
        side = [ds.material_id(left), ds.material_id(right)]
        assert (li[:, :2, 0] == side[0]).all() and (li[:, 3:, 0] == side[1]).all() and (li[:, :2, 1] == EMPTY).all()


def test_chain_ids_against_the_chain_restatement(oracle_lib):
    """on the features scene (37 x 23, N = 4) the ids' chains make spec_features_ref's World::hit calls; a sample has
    the background id exactly when its chain missed or escaped; at max_specular 0 the id is the first hit's field 12;
    an object without a material reports RS_NO_MATERIAL; chains through the mirrors change some ids"""
    cam, world = scenes.features_scene(37, 23)
    st = cam.take_photo().samples(4).seed(5).pass_index(1).settings()
    orc, rec = R.oracle_scene(world)
    alb = F.Albedo(rec)
    bouncer = R.Bouncer(alb)
    hit_fn = F.oracle_hits(orc)
    per_m = {}
    for m in (0, 1, 4):
        ids, calls = M.frame_ids(cam.desc, st, hit_fn, bouncer, m)
        ch = R.chains(cam.desc, st, hit_fn, alb, m, bouncer=bouncer)
        assert (calls == ch.calls).all()
        assert ((ids == BG) == ((ch.ending == R.MISS) | (ch.ending == R.ESCAPE))).all()
        per_m[m] = ids
        if m > 0:
            assert ch.count(R.ESCAPE) > 0 and ch.count(R.TERMINAL_AFTER) > 0
    rays = F.camera_rays(cam.desc, st, [(x, y) for y in range(23) for x in range(37)]).reshape(-1, 7)
    recs = hit_fn(rays)
    first = np.where(recs[:, 0] == 1.0, recs[:, 12], BG).astype(np.int64).reshape(-1, 4)
    assert (per_m[0] == first).all()
    assert (per_m[0] == A.RS_NO_MATERIAL).any() and (per_m[0] == BG).any()
    assert (per_m[1] != per_m[0]).any() and (per_m[4] != per_m[1]).any()


# ---------------------------------------------------------------- argument and state checks ----
def _scene(lib):
    h = C.c_void_p()
    assert lib.rs_scene_create(C.byref(h)) == 0
    return h


def _host_only_world():
    h, lights = api.HittableList(), api.HittableList()
    light = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(api.Color(1.0, 0.9, 0.8)))
    h.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Metal(api.Color(0.5, 0.5, 0.5))))
    h.add(api.Sphere((3.0, 0.0, 0.0), 1.0, None))
    h.add(light)
    lights.add(light)
    world = api.World(h, lights)
    world._scene = api.DeviceScene(world, devices=[])
    return world


def test_symbols_are_exported(hip_lib):
    for name in ("rs_render_mattes", "rs_render_mattes_device", "rs_matte_extract_device", "rs_matte_extract"):
        assert name in A.EXPORTED_SYMBOLS and getattr(hip_lib, name) is not None
    assert hip_lib.rs_abi_version() == 6


def test_render_mattes_argument_checks(hip_lib):
    """ranks 0 and 9, max_specular 17 and a NULL ids or cov are RS_E_INVALID with a message, before commit and on a
    host-only scene alike and before the state check; a valid call meets RS_E_STATE; overflow may be NULL; nothing is
    written"""
    lib = hip_lib
    cam = A.rs_camera_desc()
    cam.width, cam.height = 4, 3
    st = A.rs_render_settings()
    st.samples, st.depth = 4, 1
    ids = np.full((3, 4, 8), 7, np.int32)
    cov = np.full((3, 4, 8), 7.0, np.float32)
    ovf = np.full((3, 4), 7, np.uint8)
    ip, cp, op = ids.ctypes.data, cov.ctypes.data, ovf.ctypes.data
    fresh = _scene(lib)
    for s in (fresh, _host_only_world().device_scene().handle):
        head = (s, C.byref(cam), C.byref(st), None)
        for ranks, m, a, b, word in ((0, 0, ip, cp, b"ranks"), (9, 0, ip, cp, b"ranks"), (2 ** 32 - 1, 0, ip, cp, b"ranks"),
                                     (4, 17, ip, cp, b"max_specular"), (4, 0, None, cp, b"null"), (4, 0, ip, None, b"null"),
                                     (4, 0, None, None, b"null")):
            assert lib.rs_render_mattes(*head, ranks, m, a, b, op, None) == A.RS_E_INVALID, (ranks, m)
            assert word in lib.rs_last_error(), (word, lib.rs_last_error())
            assert lib.rs_render_mattes_device(*head, ranks, m, a, b, op, None, None) == A.RS_E_INVALID
            assert word in lib.rs_last_error()
        for ranks, m in ((1, 0), (8, 16), (4, 1)):
            assert lib.rs_render_mattes(*head, ranks, m, ip, cp, op, None) == A.RS_E_STATE
            assert lib.rs_render_mattes(*head, ranks, m, ip, cp, None, None) == A.RS_E_STATE
            assert lib.rs_render_mattes_device(*head, ranks, m, C.c_void_p(0x1000), C.c_void_p(0x2000), None, None,
                                               None) == A.RS_E_STATE
    assert lib.rs_render_mattes(None, C.byref(cam), C.byref(st), None, 4, 0, ip, cp, op, None) == A.RS_E_INVALID
    assert lib.rs_render_mattes(fresh, None, C.byref(st), None, 4, 0, ip, cp, op, None) == A.RS_E_INVALID
    assert lib.rs_render_mattes_device(fresh, C.byref(cam), None, None, 4, 0, ip, cp, op, None, None) == A.RS_E_INVALID
    assert (ids == 7).all() and (cov == 7.0).all() and (ovf == 7).all()
    lib.rs_scene_destroy(fresh)


def test_matte_extract_argument_checks(hip_lib):
    """every invalid argument of both entries is RS_E_INVALID with a message before anything touches a device"""
    lib = hip_lib
    ids = np.zeros((3, 4, 2), np.int32)
    cov = np.zeros((3, 4, 2), np.float32)
    out = np.full((3, 4), 7.0, np.float32)
    want = (C.c_int32 * 65)(*range(65))
    ip, cp, op = ids.ctypes.data, cov.ctypes.data, out.ctypes.data
    bad = [((ip, cp, 4, 3, 0, want, 1, op), b"ranks"), ((ip, cp, 4, 3, 9, want, 1, op), b"ranks"),
           ((ip, cp, 4, 3, 2, want, 0, op), b"n_wanted"), ((ip, cp, 4, 3, 2, want, 65, op), b"n_wanted"),
           ((ip, cp, 0, 3, 2, want, 1, op), b"empty"), ((ip, cp, 4, 0, 2, want, 1, op), b"empty"),
           ((ip, cp, 65536, 32768, 2, want, 1, op), b"too large"),
           ((None, cp, 4, 3, 2, want, 1, op), b"null"), ((ip, None, 4, 3, 2, want, 1, op), b"null"),
           ((ip, cp, 4, 3, 2, None, 1, op), b"null"), ((ip, cp, 4, 3, 2, want, 1, None), b"null")]
    for args, word in bad:
        assert lib.rs_matte_extract(*args) == A.RS_E_INVALID, args
        assert word in lib.rs_last_error() and b"matte_extract" in lib.rs_last_error(), lib.rs_last_error()
        assert lib.rs_matte_extract_device(*args, None) == A.RS_E_INVALID, args
        assert word in lib.rs_last_error()
    assert (out == 7.0).all()


def test_python_wrappers_on_a_host_only_scene(hip_lib):
    """DeviceScene.render_mattes / render_mattes_device, TakePhotoSettings.shot_mattes and matte_extract[_device] raise
    the library's codes; DeviceScene.material_id names the scene's materials"""
    world = _host_only_world()
    ds = world.device_scene()
    cam = api.CameraBuilder().look_from(api.Point3(13.0, 2.0, 3.0)).look_at(api.Point3(0.0, 0.0, 0.0)).fov(20.0) \
        .width(4).height(3).build()
    photo = cam.take_photo().samples(4).seed(1)
    ids = np.zeros((3, 4, 2), np.int32)
    cov = np.zeros((3, 4, 2), np.float32)
    for call, code in ((lambda: ds.render_mattes(cam.desc, photo.settings()), A.RS_E_STATE),
                       (lambda: ds.render_mattes(cam.desc, photo.settings(), 8, 16, want_overflow=False), A.RS_E_STATE),
                       (lambda: ds.render_mattes(cam.desc, photo.settings(), ranks=0), A.RS_E_INVALID),
                       (lambda: ds.render_mattes(cam.desc, photo.settings(), ranks=9), A.RS_E_INVALID),
                       (lambda: ds.render_mattes(cam.desc, photo.settings(), max_specular=17), A.RS_E_INVALID),
                       (lambda: ds.render_mattes_device(cam.desc, photo.settings(), 0x1000, 0x2000, stats=False), A.RS_E_STATE),
                       (lambda: ds.render_mattes_device(cam.desc, photo.settings(), 0, 0x2000, stats=False), A.RS_E_INVALID),
                       (lambda: ds.render_mattes_device(cam.desc, photo.settings(), 0x1000, 0x2000, ranks=9), A.RS_E_INVALID),
                       (lambda: photo.shot_mattes(world), A.RS_E_STATE),
                       (lambda: photo.shot_mattes(world, None, 4, 2), A.RS_E_STATE),
                       (lambda: photo.shot_mattes(world, ranks=0), A.RS_E_INVALID),
                       (lambda: photo.shot_mattes(world, max_specular=17), A.RS_E_INVALID),
                       (lambda: api.matte_extract(ids, cov, []), A.RS_E_INVALID),
                       (lambda: api.matte_extract(ids, cov, list(range(65))), A.RS_E_INVALID),
                       (lambda: api.matte_extract(ids, cov, [2 ** 31]), A.RS_E_INVALID),
                       (lambda: api.matte_extract(np.zeros((3, 4, 9), np.int32), np.zeros((3, 4, 9), np.float32), [1]),
                        A.RS_E_INVALID),
                       (lambda: api.matte_extract_device(0x1000, 0x2000, 4, 3, 2, [], 0x3000), A.RS_E_INVALID),
                       (lambda: api.matte_extract_device(0, 0x2000, 4, 3, 2, [1], 0x3000), A.RS_E_INVALID),
                       (lambda: api.matte_extract_device(0x1000, 0x2000, 4, 3, 2, [1], 0), A.RS_E_INVALID)):
        with pytest.raises(api.RaysnailError) as e:
            call()
        assert e.value.code == code
    metal = world.hittables.objects[0].material
    lamp = world.hittables.objects[2].material
    assert ds.material_id(metal) == 0 and ds.material_id(lamp) == 1 and ds.material_id(None) == A.RS_NO_MATERIAL
    with pytest.raises(KeyError):
        ds.material_id(api.Metal(api.Color(0.5, 0.5, 0.5)))
