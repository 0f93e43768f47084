"""World::hit on the GPU against the oracle far from the coordinate origin and at other scales (tests/far_worlds.py):
edge_rays.py's six worlds and ray families translated by up to 2^40 and scaled by 2^-130 .. 2^130 -- where the f32
boxes of the tree are one ulp wide, subnormal, zero or infinite and the f32 cull of the walks (rs_cull.h) must still
never lose a box the exact test accepts -- plus named rays for the three classes of boxes it used to lose, and one
small frame per walk over the 2^29-translated world.

Compared as tests/test_gpu_edge_rays.py compares: reference-order worlds (nest0, nest2, rich) in all 13 fields bit
for bit; near-first worlds (spheres, spheres_moving, flat) in the hit flag and t1 on every ray and in the whole record
wherever one object alone has that t1, and where several tie the record is one tied object's. NaNs (the oracle has
some at these scales) are compared by position. tests/test_far_worlds_cpu.py guards the fixtures."""
import numpy as np
import pytest

import edge_rays as E
import far_worlds as F
from raysnail_amd import _abi as A

pytestmark = pytest.mark.gpu


def _probe_world(w, r: np.ndarray, tmin: float) -> np.ndarray:
    ds = w.device_scene()
    out = np.full((len(r), 13), -7.0)
    assert ds.lib.rs_probe_world_hit(ds.handle, r.ctypes.data, len(r), tmin, E.INF, out.ctypes.data) == 0
    return out


def _differs(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: NaN against NaN is equal (no portable bit pattern), everything else by its bits."""
    nan = np.isnan(b)
    return (np.isnan(a) != nan) | ((E.bits(a) != E.bits(b)) & ~nan)


def _describe(what, r, rows, gpu, ref, limit=4):
    lines = [f"{what}: {len(rows)} of {len(r)} rays differ"]
    for i in rows[:limit]:
        lines.append(f"  ray {i} o {r[i, :3]} d {r[i, 3:6]} time {r[i, 6]}\n    gpu    {gpu[i]}\n    oracle {ref[i]}")
    return "\n".join(lines)


def _compare(what, name, w, r, got, ref, tmin):
    bad = _differs(got, ref)
    if name in E.REF_ORDER:
        rows = np.flatnonzero(bad.any(axis=1))
        assert len(rows) == 0, _describe(what, r, rows, got, ref)
        return
    # near-first: flag and t1 on every ray (a t1 of zero may carry either sign: two objects touching at the origin)
    zero = (ref[:, 1] == 0.0) & (got[:, 1] == 0.0)
    rows = np.flatnonzero((bad[:, :2].any(axis=1) & ~zero) | bad[:, 0])
    assert len(rows) == 0, _describe(what, r, rows, got, ref)
    rows = np.flatnonzero(bad.any(axis=1))
    if len(rows):   # these must be ties, and the record one tied object's
        tied, recs = F.tied_objects(w, r, ref, tmin, rows)
        same = ~_differs(recs[:, :, 1:13], np.broadcast_to(got[rows, 1:13], recs[:, :, 1:13].shape))
        ok = np.any(np.all(same, axis=2) & tied, axis=0) & (tied.sum(axis=0) >= 2)
        assert ok.all(), _describe(what, r, rows[~ok], got, ref)


def _cells():
    out = []
    for name in F.NAMES:
        for v in F.VARIANTS:
            for dm in (F.DIR_MODES if v in F.SCALED else ("dirs_scaled",)):
                if (name, v, dm) not in F.ORACLE_HITS_NOTHING:
                    out.append((name, v, dm))
    return out


@pytest.mark.parametrize("name,variant,dir_mode", _cells())
def test_far_world_records(gpu, name, variant, dir_mode):
    """One probe call per (world, variant, direction mode, tmin) over about 1 500 rays."""
    w = F.world(name, variant)
    r = F.rays(name, variant, dir_mode)[0]
    for tmin in F.tmins(variant, dir_mode):
        ref = F.reference(name, variant, dir_mode, tmin)
        assert ref[:, 0].sum() >= 100
        _compare(f"{name} {variant} {dir_mode} tmin {tmin}", name, w, r, _probe_world(w, r, tmin), ref, tmin)


@pytest.mark.parametrize("case", sorted(F.NAMED))
def test_named_rays(gpu, case):
    """The rays whose boxes the cull lost (A: |o| / |d| beyond f32 on an axis the ray is parallel to, B: an origin
    beyond the largest float, C: 1e30 < |1 / d| <= 3e38), in a flat, a spheres and a reference-order world: the
    oracle hits (test_far_worlds_cpu.py), and the record is the oracle's."""
    from oracle.binding import OracleScene
    w, r = F.named_world(case), F.named_ray(case)
    ref = E.oracle_records(OracleScene(w), r, F.NAMED_TMIN)
    got = _probe_world(w, r, F.NAMED_TMIN)
    assert ref[0, 0] == 1.0
    assert not _differs(got, ref).any(), _describe(case, r, [0], got, ref)


@pytest.mark.parametrize("mode", [A.RS_MODE_MEGAKERNEL, A.RS_MODE_WAVEFRONT, A.RS_MODE_AUTO])
@pytest.mark.parametrize("name", F.FRAME_NAMES)
def test_frames_far_from_the_origin(gpu, name, mode):
    """Frames through each scene mode's own kernels (the probe runs the generic walk only) over the world translated
    by 2^29: 8 x 6, 4 spp, depth 4, the camera looking along an axis, so every bounce ray starts far from the
    coordinate origin. The frame and the world.hit count are the oracle's."""
    cam = F.frame_camera(name)
    w = F.world(name, F.FRAME_VARIANT)
    photo = cam.take_photo().samples(4).depth(4).seed(7).mode(mode)
    img = photo.shot(None, w)
    ref, rstats = F.oracle(name, F.FRAME_VARIANT).render(cam.desc, photo.settings(), threads=8)
    assert photo.last_stats.segments == rstats.segments
    assert np.array_equal(img, ref), float(np.mean(np.all(img == ref, axis=-1)))
