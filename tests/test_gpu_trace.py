"""Ray queries on the GPU (rs_trace_closest[_device], rs_trace_occluded[_device]) against the oracle's World::hit with
each ray's own range (tests/trace_ref.py over tests/edge_rays.py's scenes and rays), bit for bit.

Reference-order scenes (nest0, nest2, rich) walk the oracle's tree in its order: every field of every ray is the
oracle's. Near-first scenes (spheres, spheres_moving, flat): hit flag and t1 are the oracle's on every ray and so is the
whole record wherever one object alone has that t1; where several tie, the record is one tied object's -- the rule
tests/test_gpu_edge_rays.py states for the near-first walk. The occlusion byte is the oracle's hit flag on every ray,
tied or not. Every device output lies between guard zones that must stay intact."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import edge_rays as E
import trace_ref as T
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes before and after every device output (a multiple of 16: geom stays aligned)
FILL = 0xA5
SCENES = sorted(E.SCENES)


# ------------------------------------------------------------------------------- running ----
class _Out:
    """A device output of `nbytes` bytes between two guard zones."""

    def __init__(self, torch, nbytes):
        self.torch, self.nbytes = torch, nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def get(self, dtype, shape):
        """the payload; asserts the guard zones first"""
        host = self.buf.cpu().numpy()
        assert np.all(host[:GUARD] == FILL) and np.all(host[GUARD + self.nbytes:] == FILL), "guard zone overwritten"
        return host[GUARD:GUARD + self.nbytes].view(dtype).reshape(shape).copy()


def _closest(torch, ds, rays8, tmin, want_geom=True, want_uv=True, stream=None, replica=0):
    """rs_trace_closest_device on a host table: (ids, geom or None, uv or None)"""
    n = len(rays8)
    d_rays = torch.from_numpy(np.array(rays8)).cuda() if n else None  # (a copy: the tables are read-only)
    ids = _Out(torch, n * 16)
    geom = _Out(torch, n * 64) if want_geom else None
    uv = _Out(torch, n * 16) if want_uv else None
    torch.cuda.synchronize()
    ds.trace_closest_device(d_rays.data_ptr() if n else 0, n, tmin, ids.ptr, geom.ptr if geom else 0, uv.ptr if uv else 0,
                            stream_ptr=stream.cuda_stream if stream else 0, replica=replica)
    (stream or torch.cuda).synchronize()
    return (ids.get(np.int32, (n, 4)), geom.get(np.float64, (n, 8)) if geom else None,
            uv.get(np.float64, (n, 2)) if uv else None)


def _occluded(torch, ds, rays8, tmin, stream=None, replica=0):
    n = len(rays8)
    d_rays = torch.from_numpy(np.array(rays8)).cuda() if n else None  # (a copy: the tables are read-only)
    occ = _Out(torch, n)
    torch.cuda.synchronize()
    ds.trace_occluded_device(d_rays.data_ptr() if n else 0, n, tmin, occ.ptr,
                             stream_ptr=stream.cuda_stream if stream else 0, replica=replica)
    (stream or torch.cuda).synchronize()
    return occ.get(np.uint8, (n,))


@functools.lru_cache(maxsize=None)
def _gpu(name: str, family: str, tmin: float):
    """both forms on T.table(name, family, tmin): one launch each per table, shared by the tests"""
    import torch
    ds = E.world(name).device_scene()
    r8 = T.table(name, family, tmin)
    out = _closest(torch, ds, r8, tmin) + (_occluded(torch, ds, r8, tmin),)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------- comparing ----
def _differs(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """elementwise: NaN against NaN is equal (no portable bit pattern), everything else by its bits"""
    nan = np.isnan(b)
    return (np.isnan(a) != nan) | ((E.bits(a) != E.bits(b)) & ~nan)


def _describe(what, rows, r8, got, ref, limit=4):
    lines = [f"{what}: {len(rows)} of {len(r8)} rays differ"]
    for i in rows[:limit]:
        lines.append(f"  ray {i} {r8[i].tolist()}\n    gpu    {got[i].tolist()}\n    oracle {ref[i].tolist()}")
    return "\n".join(lines)


def _check_closest(name, what, r8, tmin, ids, geom, uv, ref, must_hit=()):
    """the closest form's outputs against the oracle's records `ref` by the scene's rule (module docstring); returns
    (tied, recs) of T.ties when it had to compute them (near-first scenes with a differing row), else None"""
    assert T.miss_rows_ok(ids, geom, uv), what
    got = T.as_records(ids, geom, uv)
    bad = _differs(got, ref)
    assert np.all(ids[list(must_hit), 0] == 1), what
    if name in E.REF_ORDER:
        rows = np.flatnonzero(bad.any(axis=1))
        assert len(rows) == 0, _describe(what, rows, r8, got, ref)
        return None
    # bitwise, except that a t1 of zero may carry either sign: two spheres touching at the ray's origin give +0 and -0
    # (a tie: E.ties), and the tied object's own bits are asserted below
    zero = (ref[:, 1] == 0.0) & (got[:, 1] == 0.0)
    rows = np.flatnonzero((bad[:, :2].any(axis=1) & ~zero) | bad[:, 0])
    assert len(rows) == 0, _describe(what, rows, r8, got, ref)
    differ = bad.any(axis=1)
    if not differ.any():
        return None
    tied, recs = T.ties(name, r8, ref, tmin)
    tie = tied.sum(axis=0) >= 2
    rows = np.flatnonzero(differ & ~tie)
    assert len(rows) == 0, _describe(what, rows, r8, got, ref)
    rows = np.flatnonzero(differ)
    same = ~_differs(recs[:, rows, 1:13], np.broadcast_to(got[rows, 1:13], recs[:, rows, 1:13].shape))
    ok = np.any(np.all(same, axis=2) & tied[:, rows], axis=0)
    assert ok.all(), _describe(what, rows[~ok], r8, got, ref)
    return tied, recs


def _check_objects(name, ids, ds):
    """every hit's `object` is a handle of a world object that can carry the record's material"""
    can = T.handle_materials(E.world(name), ds)
    for h in np.flatnonzero(ids[:, 0] == 1):
        obj, mat = int(ids[h, 3]), int(ids[h, 2])
        assert obj in can and (mat in can[obj] or None in can[obj]), (name, h, obj, mat, can.get(obj))


# ------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("tmin", E.TMINS)
@pytest.mark.parametrize("name", SCENES)
def test_closest_to_infinity(gpu, name, tmin):
    """all of rays(name) with tmax = +inf at three tmin: the records by the scene's rule, uv included in `rich`; the
    occlusion byte is the oracle's hit flag on every row; `object` names an object that carries the record's material,
    and in the near-first scenes, on untied hit rows, the object E.ties names as the winner"""
    ids, geom, uv, occ = _gpu(name, "inf", tmin)
    r8, ref = T.table(name, "inf", tmin), E.reference(name, tmin)
    _check_closest(name, f"{name} tmin {tmin}", r8, tmin, ids, geom, uv, ref)
    assert np.array_equal(occ, (ref[:, 0] == 1.0).astype(np.uint8))
    ds = E.world(name).device_scene()
    _check_objects(name, ids, ds)
    if name == "rich":
        assert ds.info().scene_mode == 0 and np.any(uv != 0.0)
    else:
        assert np.all(E.bits(uv) == 0)  # no (u, v) in a scene that reads none: +0.0
    if name in E.NEAR_FIRST:
        tied, _ = E.ties(name, tmin)
        handles = np.array(T.leaf_handles(name, ds))
        rows = np.flatnonzero((ref[:, 0] == 1.0) & (tied.sum(axis=0) == 1))
        assert len(rows) > len(ref) // 10
        winner = handles[np.argmax(tied[:, rows], axis=0)]
        assert np.array_equal(ids[rows, 3], winner)


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("name", SCENES)
def test_tmax_families(gpu, name, family):
    """each family of range ends at tmin = 1e-4 against the oracle under that range: hit flag and t1 on every row, the
    full record on untied rows (every row in the reference-order scenes); the rows that still hit with the range ending
    at or before the full range's t1 are hits (the range end is the walk's initial one, not a filter); the occlusion
    byte is the oracle's hit flag on every row"""
    ids, geom, uv, occ = _gpu(name, family, T.TMIN)
    r8, ref = T.table(name, family), T.reference(name, family)
    must = T.still_hit_rows(name, family) if family in ("t1", "t1_half") else ()
    _check_closest(name, f"{name} {family}", r8, T.TMIN, ids, geom, uv, ref, must_hit=must)
    assert np.array_equal(occ, (ref[:, 0] == 1.0).astype(np.uint8))
    assert np.array_equal(occ, ids[:, 0].astype(np.uint8))
    _check_objects(name, ids, E.world(name).device_scene())


def test_object_under_a_shared_material(gpu):
    """a reference-order world whose objects share one material: the records are the oracle's, and `object` is the
    handle of an object on which the hit point lies (that object alone, asked with the range ending just past t1,
    answers with the world's t1, point and normal) -- on the rows where one does, at least 95 % of the hits"""
    import torch
    w = T.shared_material_world()
    ds = w.device_scene()
    ref, on = T.shared_material_candidates()
    r8 = T.with_tmax(E.rays("nest0")[0], np.inf)
    ids, geom, uv = _closest(torch, ds, r8, T.TMIN)
    assert T.miss_rows_ok(ids, geom, uv)
    rows = np.flatnonzero(_differs(T.as_records(ids, geom, uv), ref).any(axis=1))
    assert len(rows) == 0, _describe("shared material", rows, r8, T.as_records(ids, geom, uv), ref)
    handles = [ds.object_ids(o)[0] for o in w.hittables.objects]
    slot = {h: k for k, h in enumerate(handles)}
    checked = 0
    for i in np.flatnonzero((ref[:, 0] == 1.0) & (on.sum(axis=0) >= 1)):
        assert on[slot[int(ids[i, 3])], i], (i, ids[i], np.flatnonzero(on[:, i]))
        checked += 1
    assert checked >= 0.95 * (ref[:, 0] == 1.0).sum()
    grey = ds.material_id(w.hittables.objects[1].material)
    assert len(set(ids[(ids[:, 0] == 1) & (ids[:, 2] == grey), 3].tolist())) >= 5  # one material, several objects


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4171])
def test_batch_sizes(gpu, n):
    """prefixes of one table (flat, the range ending at twice the hit): each prefix's outputs are the prefix of the
    whole table's, in both forms, with the guard zones before and after every output intact (asserted by the run)"""
    import torch
    name, family = "flat", "t1_twice"
    ids, geom, uv, occ = _gpu(name, family, T.TMIN)
    assert len(ids) == 4171
    ds = E.world(name).device_scene()
    r8 = T.table(name, family)[:n]
    i2, g2, u2 = _closest(torch, ds, r8, T.TMIN)
    assert np.array_equal(i2, ids[:n]) and np.array_equal(E.bits(g2), E.bits(geom[:n]))
    assert np.array_equal(E.bits(u2), E.bits(uv[:n]))
    assert np.array_equal(_occluded(torch, ds, r8, T.TMIN), occ[:n])


@pytest.mark.parametrize("name", ["nest0", "spheres"])
def test_second_trip_of_the_grid(gpu, name):
    """256 x 4171 rays, the table tiled: more than 8 blocks per compute unit, so the grid-stride loop takes a second
    trip (the grid rule of raysnail_hip.h). Every tile equals the first bit for bit, compared on the device; the first
    is compared with the oracle."""
    import torch
    family, tiles = "t1_twice", 256
    r8 = T.table(name, family)
    n = tiles * len(r8)
    assert n > 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256
    ds = E.world(name).device_scene()
    d_rays = torch.from_numpy(np.array(r8)).cuda().repeat(tiles, 1).contiguous()
    d_ids = torch.full((n, 4), 7, dtype=torch.int32, device="cuda")
    d_geom = torch.full((n, 8), -7.0, dtype=torch.float64, device="cuda")
    d_uv = torch.full((n, 2), -7.0, dtype=torch.float64, device="cuda")
    d_occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ds.trace_closest_device(d_rays.data_ptr(), n, T.TMIN, d_ids.data_ptr(), d_geom.data_ptr(), d_uv.data_ptr())
    ds.trace_occluded_device(d_rays.data_ptr(), n, T.TMIN, d_occ.data_ptr())
    torch.cuda.synchronize()
    for t, width in ((d_ids, 4), (d_geom.view(torch.int64), 8), (d_uv.view(torch.int64), 2), (d_occ, 1)):
        v = t.view(tiles, len(r8), width)
        assert bool((v == v[:1]).all())
    ids, geom, uv = (t[:len(r8)].cpu().numpy() for t in (d_ids, d_geom, d_uv))
    ref = T.reference(name, family)
    _check_closest(name, f"{name} tiled", r8, T.TMIN, ids, geom, uv, ref)
    assert np.array_equal(d_occ[:len(r8)].cpu().numpy(), (ref[:, 0] == 1.0).astype(np.uint8))


@pytest.mark.parametrize("name", ["rich", "flat"])
def test_optional_outputs(gpu, name):
    """d_geom NULL, d_uv NULL, both NULL: the outputs that are given are what the full call gives"""
    import torch
    ids, geom, uv, _ = _gpu(name, "inf", T.TMIN)
    ds = E.world(name).device_scene()
    r8 = T.table(name, "inf")
    for want_geom, want_uv in ((False, True), (True, False), (False, False)):
        i2, g2, u2 = _closest(torch, ds, r8, T.TMIN, want_geom=want_geom, want_uv=want_uv)
        assert np.array_equal(i2, ids)
        assert (g2 is None) == (not want_geom) and (u2 is None) == (not want_uv)
        assert g2 is None or np.array_equal(E.bits(g2), E.bits(geom))
        assert u2 is None or np.array_equal(E.bits(u2), E.bits(uv))


def test_stream_replica_and_host_forms(gpu):
    """a side stream; replica 1 of a scene committed to devices {0, 0}; the host forms, with (n, 8) and (n, 7) tables:
    all give what the default call gives"""
    torch = gpu
    name, family = "nest2", "t1_twice"
    ids, geom, uv, occ = _gpu(name, family, T.TMIN)
    r8 = T.table(name, family)
    ds = E.world(name).device_scene()
    side = torch.cuda.Stream()
    i2, g2, u2 = _closest(torch, ds, r8, T.TMIN, stream=side)
    assert np.array_equal(i2, ids) and np.array_equal(E.bits(g2), E.bits(geom)) and np.array_equal(E.bits(u2), E.bits(uv))
    assert np.array_equal(_occluded(torch, ds, r8, T.TMIN, stream=side), occ)
    two = api.DeviceScene(E.world(name), devices=[0, 0])
    i3, g3, u3 = _closest(torch, two, r8, T.TMIN, replica=1)
    assert np.array_equal(i3, ids) and np.array_equal(E.bits(g3), E.bits(geom)) and np.array_equal(E.bits(u3), E.bits(uv))
    assert np.array_equal(_occluded(torch, two, r8, T.TMIN, replica=1), occ)
    with pytest.raises(api.RaysnailError) as e:
        _occluded(torch, two, r8, T.TMIN, replica=2)
    assert e.value.code == A.RS_E_INVALID
    i4, g4, u4 = ds.trace(r8, T.TMIN)
    assert np.array_equal(i4, ids) and np.array_equal(E.bits(g4), E.bits(geom)) and np.array_equal(E.bits(u4), E.bits(uv))
    assert np.array_equal(ds.trace(r8, T.TMIN, occlusion=True), occ)
    i5, g5, u5 = ds.trace(E.rays(name)[0])                    # (n, 7): tmax = +inf, tmin = 1e-4
    full = _gpu(name, "inf", T.TMIN)
    assert np.array_equal(i5, full[0]) and np.array_equal(E.bits(g5), E.bits(full[1]))
    assert np.array_equal(ds.trace(E.rays(name)[0], occlusion=True), full[3])
    i6, g6, u6 = ds.trace(np.zeros((0, 8)))
    assert i6.shape == (0, 4) and g6.shape == (0, 8) and u6.shape == (0, 2)


@pytest.mark.parametrize("tmax", [np.inf, 1.0])
@pytest.mark.parametrize("name", SCENES)
def test_nonfinite_rays(gpu, name, tmax):
    """rays with NaN or infinite components (E.nonfinite_rays) under tmax = +inf and 1.0: the records are the oracle's,
    NaNs by position and the rest bit for bit, by the scene's rule; the occlusion byte is the oracle's flag"""
    import torch
    r8 = T.with_tmax(E.nonfinite_rays(name)[0], tmax)
    ref = E.nonfinite_reference(name, T.TMIN) if tmax == np.inf else T.oracle_records(E.oracle(name), r8, T.TMIN)
    ds = E.world(name).device_scene()
    ids, geom, uv = _closest(torch, ds, r8, T.TMIN)
    _check_closest(name, f"{name} non-finite tmax {tmax}", r8, T.TMIN, ids, geom, uv, ref)
    assert np.array_equal(_occluded(torch, ds, r8, T.TMIN), (ref[:, 0] == 1.0).astype(np.uint8))


def test_raymarcher(gpu):
    """256 camera rays (16 x 16 stratum centres) into scenes.raymarching_test's world, through the marcher's own
    instantiation: the closest form against rs_probe_world_hit's records of the same rays (pinned against
    tests/raymarch_ref.py by tests/test_gpu_raymarch.py), the occlusion form against the closest form's flag; with the
    range ending at 12.0 -- behind the bulb, before the far ground -- against the probe's records cut there (a sphere
    returns its closest root in range, so the shorter range only removes its hits; the marcher never reads the range
    end, and all its hits here lie before 12)"""
    import torch
    cam, world, _, _ = scenes.raymarching_test(16, 16)
    ds = world.device_scene()
    st = cam.take_photo().samples(1).seed(5).settings()
    xys = np.array([[x, y, 0] for y in range(16) for x in range(16)], np.uint32)
    cr = np.zeros((256, 11))
    assert ds.lib.rs_probe_camera(ds.handle, C.byref(cam.desc), C.byref(st), xys.ctypes.data, 256, 1, cr.ctypes.data) == 0
    r7 = np.ascontiguousarray(cr[:, :7])
    probe = np.full((256, 13), -7.0)
    assert ds.lib.rs_probe_world_hit(ds.handle, r7.ctypes.data, 256, T.TMIN, np.inf, probe.ctypes.data) == 0
    r8 = T.with_tmax(r7, np.inf)
    ids, geom, uv = _closest(torch, ds, r8, T.TMIN)
    assert T.miss_rows_ok(ids, geom, uv)
    rows = np.flatnonzero(_differs(T.as_records(ids, geom, uv), probe).any(axis=1))
    assert len(rows) == 0, _describe("marcher", rows, r8, T.as_records(ids, geom, uv), probe)
    bulb = ds.object_ids(world.hittables.objects[1])[0]
    assert 20 <= (ids[:, 3] == bulb).sum() <= 236 and (ids[:, 0] == 1).sum() > (ids[:, 3] == bulb).sum()
    assert np.array_equal(_occluded(torch, ds, r8, T.TMIN), ids[:, 0].astype(np.uint8))
    cut = T.with_tmax(r7, 12.0)
    ids2, geom2, uv2 = _closest(torch, ds, cut, T.TMIN)
    keep = (probe[:, 0] == 1.0) & (probe[:, 1] < 12.0)
    assert np.all(probe[ids[:, 3] == bulb, 1] < 12.0)
    want = np.where(keep[:, None], probe, 0.0)
    assert keep.any() and (~keep & (probe[:, 0] == 1.0)).any()
    rows = np.flatnonzero(_differs(T.as_records(ids2, geom2, uv2), want).any(axis=1))
    assert len(rows) == 0, _describe("marcher, tmax 12", rows, cut, T.as_records(ids2, geom2, uv2), want)
    assert np.array_equal(_occluded(torch, ds, cut, T.TMIN), keep.astype(np.uint8))


def test_cpp_layer_on_the_gpu(gpu, tmp_path):
    """tests/cpp/test_trace_api.cpp in its `gpu` mode: World::trace_closest, trace_occluded and object_ids of the C++
    host layer give what the Python layer gives of the same world and rays"""
    import test_trace_cpp as TC
    exe, path = TC.build(tmp_path), tmp_path / "trace.bin"
    r8 = TC.rays()
    r8.tofile(tmp_path / "rays.bin")
    r = subprocess.run([str(exe), "gpu", str(tmp_path / "rays.bin"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-500:])
    n = len(r8)
    raw = np.fromfile(path, np.uint8)
    pos, got = 0, []
    for count, dt in ((n * 4, np.int32), (n * 8, np.float64), (n * 2, np.float64), (n, np.uint8), (n * 4, np.int32),
                      (3, np.uint32)):
        size = count * np.dtype(dt).itemsize
        got.append(raw[pos:pos + size].view(dt))
        pos += size
    assert pos == len(raw)
    world, objs = TC.world()
    ds = world.device_scene()
    ids, geom, uv = ds.trace(r8, 1e-3)
    assert 0.2 < ids[:, 0].mean() < 0.9
    assert np.array_equal(got[0].reshape(n, 4), ids) and np.array_equal(E.bits(got[1].reshape(n, 8)), E.bits(geom))
    assert np.array_equal(E.bits(got[2].reshape(n, 2)), E.bits(uv))
    assert np.array_equal(got[3], ds.trace(r8, 1e-3, occlusion=True))
    assert np.array_equal(got[4].reshape(n, 4), ids)          # want_geom = want_uv = false
    assert got[5].tolist() == [ds.object_ids(o)[0] for o in objs]
