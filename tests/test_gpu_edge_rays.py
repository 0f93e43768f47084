"""World::hit on the GPU against the oracle where ordinary arithmetic ends (tests/edge_rays.py): direction
components exactly +0 / -0 / subnormal / tiny, origins on bounding-box planes, on surfaces and at centres, tangent
rays and exact ties -- the inputs of slab64's NaN-ignoring min / max, make_rayf's clamp and slack, sort_push4's
order, the a == 0 / len == 0 / delta == 0 branches and the closed range ends.

Records are compared bitwise (through uint64), so the sign of a zero counts. Reference-order scenes walk the
oracle's tree in its order: every field of every ray is the oracle's. Near-first scenes visit children by entry
distance: the hit flag and t1 are the oracle's on every ray and so is the whole record wherever one object alone
has that t1; where several objects tie, the record is one tied object's (which one: DESIGN section 4; printed here,
not asserted). tests/test_edge_rays_cpu.py guards the fixtures."""
import functools

import numpy as np
import pytest

import edge_rays as E
from raysnail_amd import _abi as A

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _probe(name: str, tmin: float) -> np.ndarray:
    """One rs_probe_world_hit call per (scene, tmin), all families concatenated (the probe allocates per call)."""
    r = E.rays(name)[0]
    ds = E.world(name).device_scene()
    out = np.full((len(r), 13), -7.0)
    assert ds.lib.rs_probe_world_hit(ds.handle, r.ctypes.data, len(r), tmin, E.INF, out.ctypes.data) == 0
    out.setflags(write=False)
    return out


def _rows_differing(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.flatnonzero(np.any(E.bits(a) != E.bits(b), axis=1))


def _describe(name, tmin, rows, gpu, ref, limit=5):
    r = E.rays(name)[0]
    lines = [f"{name} tmin {tmin}: {len(rows)} of {len(r)} rays differ"]
    for i in rows[:limit]:
        lines.append(f"  ray {i} o {r[i, :3]} d {r[i, 3:6]} time {r[i, 6]}\n    gpu    {gpu[i]}\n    oracle {ref[i]}")
    return "\n".join(lines)


@pytest.mark.parametrize("tmin", E.TMINS)
@pytest.mark.parametrize("name", E.REF_ORDER)
def test_reference_order_records_exact(gpu, name, tmin):
    """nest0, nest2, rich: all 13 fields of every ray, bit for bit; ties are defined too (the oracle's tree in the
    oracle's order)."""
    got, ref = _probe(name, tmin), E.reference(name, tmin)
    rows = _rows_differing(got, ref)
    assert len(rows) == 0, _describe(name, tmin, rows, got, ref)


@pytest.mark.parametrize("tmin", E.TMINS)
@pytest.mark.parametrize("name", E.NEAR_FIRST)
def test_near_first_records(gpu, name, tmin):
    """spheres, spheres_moving, flat: hit flag and t1 of every ray are the oracle's; a ray that is not a tie has all
    13 fields equal; a tie ray's record is, in fields 1-11 and the material, the record of one tied object."""
    got, ref = _probe(name, tmin), E.reference(name, tmin)
    # bitwise, except that a t1 of zero may carry either sign: two spheres touching at the ray's origin give +0 and
    # -0 (a tie: E.ties), and the tied object's own bits are asserted below
    zero = (ref[:, 1] == 0.0) & (got[:, 1] == 0.0)
    rows = np.flatnonzero(np.any(E.bits(got[:, :2]) != E.bits(ref[:, :2]), axis=1) & ~zero)
    assert len(rows) == 0, _describe(name, tmin, rows, got, ref)
    rows = _rows_differing(got[:, :1], ref[:, :1])
    assert len(rows) == 0, _describe(name, tmin, rows, got, ref)
    tied, recs = E.ties(name, tmin)
    tie = tied.sum(axis=0) >= 2
    differ = np.zeros(len(ref), bool)
    differ[_rows_differing(got, ref)] = True
    rows = np.flatnonzero(differ & ~tie)
    assert len(rows) == 0, _describe(name, tmin, rows, got, ref)
    ok = E.matches_a_tied_object(got, tied, recs)
    rows = np.flatnonzero(tie & ~ok)
    assert len(rows) == 0, _describe(name, tmin, rows, got, ref)
    msg = f"{name} tmin {tmin}: {int(tie.sum())} tie rays, {int((tie & ~differ).sum())} chose the oracle's winner"
    # pairs of objects tied (the two alone) on several rays: does the same one win on all of them?
    winners = {}
    for i in np.flatnonzero(tied.sum(axis=0) == 2):
        a, b = np.flatnonzero(tied[:, i])
        won = [bool(np.all(E.bits(recs[k, i, 1:13]) == E.bits(got[i, 1:13]))) for k in (a, b)]
        if won[0] != won[1]:
            winners.setdefault((a, b), []).append(0 if won[0] else 1)
    several = [w for w in winners.values() if len(w) > 1]
    msg += (f"; {len(several)} pairs of objects tie on several rays, {sum(len(set(w)) > 1 for w in several)} of them "
            f"with a ray-dependent winner")
    if name == "flat":
        a, b = E.coplanar_rects(name)
        both = np.flatnonzero(tied[a] & tied[b] & (tied.sum(axis=0) == 2))
        mats = E.leaf_objects(E.world(name))
        win_a = int((got[both, 12] == mats[a][1]).sum())
        win_b = int((got[both, 12] == mats[b][1]).sum())
        ref_a = int((ref[both, 12] == mats[a][1]).sum())
        kind = "one winner for all rays" if min(win_a, win_b) == 0 else "a ray-dependent winner"
        msg += (f"; coplanar rects' overlap, {len(both)} rays: first rect {win_a}, second rect {win_b} ({kind}); "
                f"the oracle: first rect {ref_a}, second rect {len(both) - ref_a}")
    print(msg)


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_signed_zero_twins(gpu, name):
    """A direction with +0 components and its twin with -0 give bit-identical GPU records, as they do on the oracle
    (test_edge_rays_cpu.py): the same object wins, ties included, and every field has the same bits -- but for
    records whose own t1 is a zero (tmin = 0, the origin on the surface), where the signs of zeros follow the
    direction's and the twins' records are equal as numbers."""
    twins = E.rays(name)[2]
    for tmin in E.TMINS:
        got, ref = _probe(name, tmin), E.reference(name, tmin)
        a, b = got[twins[:, 0]], got[twins[:, 1]]
        rows = np.flatnonzero(np.any(a != b, axis=1))
        assert len(rows) == 0, _describe(name, tmin, twins[rows].ravel(), got, ref, limit=6)
        rows = np.flatnonzero(np.any(E.bits(a) != E.bits(b), axis=1) & ~((a[:, 0] == 1.0) & (a[:, 1] == 0.0)))
        assert len(rows) == 0, _describe(name, tmin, twins[rows].ravel(), got, ref, limit=6)


def test_triangle_hit_at_infinity(gpu):
    """`slanted`: rays parallel to a triangle's plane. Triangle::hit's closed range end accepts t = +inf under
    World::hit's range end +inf; the oracle reports that hit, with a NaN point and normal, and so must the probe.
    NaNs have no portable bit pattern: they are compared by position, every other field bitwise."""
    n = 0
    for tmin in E.TMINS:
        got, ref = _probe("slanted", tmin), E.reference("slanted", tmin)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan)
        rows = np.flatnonzero(np.any((E.bits(got) != E.bits(ref)) & ~nan, axis=1))
        assert len(rows) == 0, _describe("slanted", tmin, rows, got, ref)
        n += int(((got[:, 0] == 1.0) & (got[:, 1] == np.inf)).sum())
    assert n >= 20, n


def _differs_nan_aware(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: NaN against NaN is equal (no portable bit pattern), everything else by its bits."""
    nan = np.isnan(b)
    return (np.isnan(a) != nan) | ((E.bits(a) != E.bits(b)) & ~nan)


@pytest.mark.parametrize("tmin", E.TMINS)
@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_nonfinite_rays(gpu, name, tmin):
    """Rays with NaN or infinite components (E.nonfinite_rays: what a degenerate level of shading hands to
    World::hit): the hit flag and every field are the oracle's, NaNs by position and the rest bit for bit. A box
    test ignores a NaN axis (aabb.rs's f64::max / min), so the f32 culls must too (make_rayf). Near-first scenes:
    where several objects tie on t1 the record is one tied object's, as in test_near_first_records."""
    r, kind = E.nonfinite_rays(name)
    ds = E.world(name).device_scene()
    got = np.full((len(r), 13), -7.0)
    assert ds.lib.rs_probe_world_hit(ds.handle, r.ctypes.data, len(r), tmin, E.INF, got.ctypes.data) == 0
    ref = E.nonfinite_reference(name, tmin)
    bad = _differs_nan_aware(got, ref)
    rows = np.flatnonzero(bad[:, :2].any(axis=1))
    assert len(rows) == 0, (name, tmin, rows[:5], r[rows[:5]], got[rows[:5]], ref[rows[:5]])
    rows = np.flatnonzero(bad.any(axis=1))
    if name in E.NEAR_FIRST and len(rows):
        tied, recs = E.ties(name, tmin, r, ref)
        same = ~_differs_nan_aware(recs[:, rows, 1:13], np.broadcast_to(got[rows, 1:13], recs[:, rows, 1:13].shape))
        ok = np.any(np.all(same, axis=2) & tied[:, rows], axis=0) & (tied[:, rows].sum(axis=0) >= 2)
        rows = rows[~ok]
    assert len(rows) == 0, (name, tmin, rows[:5], r[rows[:5]], got[rows[:5]], ref[rows[:5]])


@pytest.mark.parametrize("mode", [A.RS_MODE_MEGAKERNEL, A.RS_MODE_WAVEFRONT])
@pytest.mark.parametrize("where", ["plane", "centre", "surface"])
@pytest.mark.parametrize("name", E.FRAME_SCENES)
def test_frames_from_special_origins(gpu, name, where, mode):
    """Frames through each scene mode's own kernels (the probe runs the generic walk only), 32 x 20, 4 spp, depth
    6, aperture 0, the eye exactly on a bounding-box plane two objects share, at a sphere's centre, or on a sphere's
    surface: every primary ray starts there. The frame and the segment count are the oracle's."""
    cam = E.frame_camera(name, where)
    world = E.world(name)
    photo = cam.take_photo().samples(4).depth(6).seed(7).mode(mode)
    img = photo.shot(None, world)
    ref, rstats = E.oracle(name).render(cam.desc, photo.settings(), threads=8)
    assert photo.last_stats.segments == rstats.segments
    assert np.array_equal(img, ref), float(np.mean(np.all(img == ref, axis=-1)))
