"""Ray queries without a GPU: the fixtures of tests/trace_ref.py hold what tests/test_gpu_trace.py relies on (oracle
only), and every invalid argument of the four rs_trace_* entries is refused before a device is needed."""
import ctypes as C

import numpy as np
import pytest

import edge_rays as E
import trace_ref as T
from raysnail_amd import _abi as A
from raysnail_amd import api

SCENES = sorted(E.SCENES)


@pytest.mark.parametrize("name", SCENES)
def test_hit_share(oracle_lib, name):
    """between a fifth and seven tenths of the rays hit at tmin = 1e-4: both outcomes are well covered"""
    share = float(np.mean(T.reference(name, "inf")[:, 0] == 1.0))
    assert 0.2 <= share <= 0.7, share


@pytest.mark.parametrize("name", E.NEAR_FIRST)
def test_tied_rows_are_few(oracle_lib, name):
    """rows on which two or more objects share the world's t1 are at most 8 % of the rows: the tolerant compare of the
    near-first scenes never covers more than that"""
    ref = T.reference(name, "inf")
    tied, _ = T.ties(name, T.table(name, "inf"), ref)
    share = float(np.mean(tied.sum(axis=0) >= 2))
    assert share <= 0.08, share
    # and the helper's ties are edge_rays' own under tmax = +inf
    tied0, _ = E.ties(name, T.TMIN)
    assert np.array_equal(tied, tied0)


@pytest.mark.parametrize("name", ["nest0", "nest2"])
def test_range_end_is_initial(oracle_lib, name):
    """with the range ending exactly at the hit, or at half of it, the oracle still hits on some rays: what answers is
    another root, operand or object inside the shorter range. A post-filter returns a miss there. (nest2 has such rows
    in the `t1` family only: 8 of them, none at t1 / 2.)"""
    rows = {fam: T.still_hit_rows(name, fam) for fam in ("t1", "t1_half")}
    print(name, {fam: len(r) for fam, r in rows.items()})
    assert sum(len(r) for r in rows.values()) >= 1
    for fam, r in rows.items():
        # (which end of the range is open is each object's own rule: a CSG record may sit exactly on the end)
        assert np.all(T.reference(name, fam)[r, 1] <= T.table(name, fam)[r, 7])


@pytest.mark.parametrize("name", SCENES)
def test_families(oracle_lib, name):
    """the helper's families: `inf` is edge_rays' reference; where every object returns its closest root in range (the
    near-first scenes) a range that ends one ulp past the hit keeps t1 -- a CSG object may lose its hit there, its
    other operand's root being cut off; a range that is empty (negative end, end below tmin) hits nothing; the hit
    flag is the occlusion byte by definition"""
    full = E.reference(name, T.TMIN)
    assert np.array_equal(E.bits(T.reference(name, "inf")), E.bits(full))
    up = T.reference(name, "t1_up")
    finite_hit = (full[:, 0] == 1.0) & np.isfinite(full[:, 1])
    if name in E.NEAR_FIRST:
        assert np.array_equal(E.bits(up[finite_hit, :2]), E.bits(full[finite_hit, :2]))
    for fam in ("neg", "below_tmin"):
        assert not T.reference(name, fam)[:, 0].any()
    for fam in T.FAMILIES:
        rec = T.reference(name, fam)
        assert set(np.unique(rec[:, 0])) <= {0.0, 1.0}
        assert np.all(rec[rec[:, 0] == 0.0] == 0.0)          # a miss is all zero: as_records' convention
        t = T.table(name, fam)
        assert t.shape == (len(full), 8) and np.array_equal(E.bits(t[:, :7]), E.bits(E.rays(name)[0]))


def test_shared_material_world(oracle_lib):
    """the extra reference-order world: its mode and order, several objects under one material, and on at least three
    quarters of the hit rows exactly one object on which the hit point lies (so `object` is pinned there); on at most
    5 % none answers alone as it does in the world (a ray through a box's edge: two faces at one t)"""
    w = T.shared_material_world()
    info = api.DeviceScene(w, devices=[]).info()
    assert (info.scene_mode, info.ref_order) == (3, 1)
    ref, on = T.shared_material_candidates()
    hit = ref[:, 0] == 1.0
    assert 0.2 <= hit.mean() <= 0.8
    assert np.mean(on[:, hit].sum(axis=0) == 0) <= 0.05 and not on[:, ~hit].any()
    assert np.mean(on[:, hit].sum(axis=0) == 1) >= 0.75
    assert len({id(o.material) for o in w.hittables.objects}) < len(w.hittables.objects) - 4


def test_as_records_and_miss_rows():
    ids = np.array([[1, 1, 3, 7], [0, 0, T.NONE, T.NONE]], np.int32)
    geom = np.array([[2.0, 3.0, 1, 2, 3, 0, 1, 0], [np.inf, 0, 0, 0, 0, 0, 0, 0]])
    uv = np.array([[0.25, 0.5], [0.0, 0.0]])
    rec = T.as_records(ids, geom, uv)
    assert rec[0].tolist() == [1.0, 2.0, 3.0, 1, 2, 3, 0, 1, 0, 0.25, 0.5, 1.0, 3.0] and not rec[1].any()
    assert T.miss_rows_ok(ids, geom, uv)
    for bad in ((1, 0, -0.0), (1, 1, 1.0)):
        g = geom.copy()
        g[bad[0], bad[1]] = bad[2]
        assert not T.miss_rows_ok(ids, g, uv)
    i2 = ids.copy()
    i2[1, 2] = -1
    assert not T.miss_rows_ok(i2, geom, uv)


def test_object_ids():
    """DeviceScene.object_ids: the export handles -- one per object, one per triangle of a mesh, the members' for a
    TfFacade over a mesh -- on a host-only commit; a stranger is a KeyError"""
    w = E.world("flat")
    ds = api.DeviceScene(w, devices=[])
    handles = T.leaf_handles("flat", ds)
    assert len(handles) == len(E.leaf_objects(w)) and len(set(handles)) == len(handles)
    mesh = [o for o in w.hittables.objects if isinstance(o, api.TriangleMesh)][0]
    tri = ds.object_ids(mesh)
    assert len(tri) == 32 and tri == list(range(tri[0], tri[0] + 32))
    assert sorted(handles) == sorted(ds.tree()["lprim"].tolist())  # every leaf entry of the tree names one of them
    with pytest.raises(KeyError):
        ds.object_ids(api.Sphere((0.0, 0.0, 0.0), 1.0, None))
    # a nested world: the handles of the world's own objects are what the tree's leaves name (lprim is empty there)
    w2 = E.world("nest2")
    ds2 = api.DeviceScene(w2, devices=[])
    tree = ds2.tree()
    leaves = sorted(~c for c in tree["child"].ravel().tolist() if c < 0 and c != -2 ** 31)
    if len(tree["lprim"]):
        leaves = sorted(tree["lprim"][leaves].tolist())
    assert leaves == sorted(T.leaf_handles("nest2", ds2))


def test_invalid_arguments(hip_lib):
    """every refusal of the four entries, through the library, without a device: argument errors are RS_E_INVALID,
    then a scene that is not committed or has no device is RS_E_STATE; n == 0 changes neither"""
    lib = hip_lib
    ds = api.DeviceScene(E.world("spheres"), devices=[])  # a host-only commit
    h = ds.handle
    buf = np.zeros(64 * 4 + 16, np.uint8)
    base = (buf.ctypes.data + 15) & ~15                      # 16-byte aligned
    rays, ids, geom, uv, occ = base, base + 64, base + 128, base + 192, base + 64
    assert lib.rs_trace_closest_device(h, 0, rays, 1, 1e-4, ids, geom, uv, None) == A.RS_E_STATE
    assert lib.rs_trace_closest_device(h, 0, rays, 1, 1e-4, ids, None, None, None) == A.RS_E_STATE
    assert lib.rs_trace_occluded_device(h, 0, rays, 1, 1e-4, occ, None) == A.RS_E_STATE
    assert lib.rs_trace_closest(h, rays, 1, 1e-4, ids, geom, uv) == A.RS_E_STATE
    assert lib.rs_trace_occluded(h, rays, 1, 1e-4, occ) == A.RS_E_STATE
    assert lib.rs_trace_closest_device(h, 0, None, 0, 1e-4, ids, None, None, None) == A.RS_E_STATE
    # NULLs
    assert lib.rs_trace_closest_device(h, 0, None, 1, 1e-4, ids, geom, uv, None) == A.RS_E_INVALID
    assert lib.rs_trace_closest_device(h, 0, rays, 1, 1e-4, None, geom, uv, None) == A.RS_E_INVALID
    assert lib.rs_trace_closest_device(h, 0, None, 0, 1e-4, None, None, None, None) == A.RS_E_INVALID
    assert lib.rs_trace_occluded_device(h, 0, None, 1, 1e-4, occ, None) == A.RS_E_INVALID
    assert lib.rs_trace_occluded_device(h, 0, rays, 1, 1e-4, None, None) == A.RS_E_INVALID
    assert lib.rs_trace_closest(h, None, 1, 1e-4, ids, geom, uv) == A.RS_E_INVALID
    assert lib.rs_trace_closest(h, rays, 1, 1e-4, None, geom, uv) == A.RS_E_INVALID
    assert lib.rs_trace_occluded(h, None, 1, 1e-4, occ) == A.RS_E_INVALID
    assert lib.rs_trace_occluded(h, rays, 1, 1e-4, None) == A.RS_E_INVALID
    assert lib.rs_trace_closest_device(None, 0, rays, 1, 1e-4, ids, geom, uv, None) == A.RS_E_INVALID
    # a replica outside the committed device list
    assert lib.rs_trace_closest_device(h, 1, rays, 1, 1e-4, ids, geom, uv, None) == A.RS_E_INVALID
    assert lib.rs_trace_occluded_device(h, 7, rays, 1, 1e-4, occ, None) == A.RS_E_INVALID
    # misaligned rays / geom (the other outputs need none; the host forms stage through memory of their own)
    assert lib.rs_trace_closest_device(h, 0, rays + 8, 1, 1e-4, ids, geom, uv, None) == A.RS_E_INVALID
    assert lib.rs_trace_closest_device(h, 0, rays, 1, 1e-4, ids, geom + 8, uv, None) == A.RS_E_INVALID
    assert lib.rs_trace_occluded_device(h, 0, rays + 8, 1, 1e-4, occ, None) == A.RS_E_INVALID
    assert lib.rs_trace_closest_device(h, 0, rays, 1, 1e-4, ids + 4, geom, uv + 8, None) == A.RS_E_STATE
    assert lib.rs_trace_closest(h, rays + 8, 1, 1e-4, ids + 4, geom + 8, uv + 8) == A.RS_E_STATE
    assert b"host-only" in lib.rs_last_error()
    # before commit
    s = C.c_void_p()
    assert lib.rs_scene_create(C.byref(s)) == 0
    try:
        assert lib.rs_trace_closest_device(s, 0, rays, 1, 1e-4, ids, geom, uv, None) == A.RS_E_STATE
        assert lib.rs_trace_occluded(s, rays, 1, 1e-4, occ) == A.RS_E_STATE
        assert lib.rs_trace_closest_device(s, 0, rays, 1, 1e-4, None, geom, uv, None) == A.RS_E_INVALID
    finally:
        lib.rs_scene_destroy(s)
    # the Python layer raises what the library refuses, and shapes its own argument
    with pytest.raises(api.RaysnailError) as e:
        ds.trace(np.zeros((3, 8)))
    assert e.value.code == A.RS_E_STATE
    with pytest.raises(api.RaysnailError):
        ds.trace(np.zeros((3, 7)), occlusion=True)
    with pytest.raises(ValueError):
        ds.trace(np.zeros((3, 6)))
    assert A.RS_TRACE_NONE == -2 ** 31
