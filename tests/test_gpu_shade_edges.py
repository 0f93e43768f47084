"""One level of ray_color after the hit on the GPU against the oracle, on exact records (tests/shade_edges.py):
rs_probe_shade runs each scene mode's own shade_step -- so its own shade_surface<-1, SM>, the three-way light dispatch
(sphere_random / Obj<0, 0>::random / obj_random<SM>) -- on the rows orc_shade_level evaluates with the oracle's
Material::scatter, Pdf and lights_random.

Everything is compared bitwise (through uint64, so the sign of a zero counts): the continues flag, the emission, the
factor, the next ray and the four RNG words after the level (a missing or an extra draw changes them). NaNs have no
portable bit pattern and are compared by position. No tolerance and no excluded rows.

Light kinds the API cannot put into a lights list (test_light_kinds_*): a BVH or HittableList as one light (the device
scene and the oracle export a group's members, so the list gets the members one by one, never BVH::random's constant),
and the RayMarcher (the oracle has none, so there is nothing to compare it with). Everything else Obj::random names is
listed: spheres, a moving sphere, xz / xy / yz rects, triangles, a quadric, a box, a scaled and a rotated TfFacade, an
Intersection, a Difference and a ConstantMedium.

tests/test_shade_edges_cpu.py guards the fixtures."""
import functools

import numpy as np
import pytest

import edge_rays as E
import shade_edges as S
from raysnail_amd import _abi as A

pytestmark = pytest.mark.gpu

FIELDS = ("continues", "L.x", "L.y", "L.z", "T.x", "T.y", "T.z", "o.x", "o.y", "o.z", "d.x", "d.y", "d.z", "time",
          "rng.x", "rng.y", "rng.z", "rng.w")


@functools.lru_cache(maxsize=None)
def _probe(name: str) -> np.ndarray:
    """One rs_probe_shade call per scene, all families concatenated."""
    r = S.rows(name)[0]
    ds = S.world(name).device_scene()
    assert ds.info().scene_mode == S.EXPECT_MODE[name]
    out = np.full(r.shape, -7.0)
    rc = ds.lib.rs_probe_shade(ds.handle, r.ctypes.data, len(r), S.SEED, out.ctypes.data)
    assert rc == 0, ds.lib.rs_last_error()
    out.setflags(write=False)
    return out


def _differing(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """(n, 18) bool: fields that differ -- NaN against NaN is equal, everything else by its bits."""
    nan = np.isnan(ref)
    return (np.isnan(got) != nan) | ((E.bits(got) != E.bits(ref)) & ~nan)


def _describe(name, family, rows, got, ref, bad, limit=4):
    r = S.rows(name)[0]
    lines = [f"{name} / {family}: {len(rows)} rows differ"]
    for i in rows[:limit]:
        what = ", ".join(FIELDS[k] for k in np.flatnonzero(bad[i]))
        lines.append(f"  row {i} ({what})\n    in     {r[i]}\n    gpu    {got[i]}\n    oracle {ref[i]}")
    return "\n".join(lines)


@pytest.mark.parametrize("name,family", [(n, f) for n in S.SCENE_NAMES for f in S.families(n)])
def test_level_exact(gpu, name, family):
    """Every row of the family: all 18 output fields are the oracle's."""
    got, ref = _probe(name), S.reference(name)
    bad = _differing(got, ref)
    rows = S.family_rows(name, family)
    rows = rows[np.any(bad[rows], axis=1)]
    assert len(rows) == 0, _describe(name, family, rows, got, ref, bad)


def test_probe_rejects_unknown_materials(gpu):
    ds = S.world("spheres").device_scene()
    r = S.rows("spheres")[0][:4].copy()
    out = np.zeros_like(r)
    for bad in (float(len(S.MATERIALS)), -2.0, 0.5, S.NAN):
        r[2, 17] = bad
        assert ds.lib.rs_probe_shade(ds.handle, r.ctypes.data, len(r), S.SEED, out.ctypes.data) == A.RS_E_INVALID
    assert ds.lib.rs_probe_shade(ds.handle, None, 0, S.SEED, out.ctypes.data) == A.RS_E_INVALID


@pytest.mark.parametrize("mode", [A.RS_MODE_MEGAKERNEL, A.RS_MODE_WAVEFRONT])
@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_light_kinds_frames(gpu, name, mode):
    """Frames through each scene mode's own kernels (the streaming kernels' instantiations of the light dispatch
    included), 32 x 20, 4 spp, depth 6, over the world whose lights list holds every kind the mode admits: the frame
    and the segment count are the oracle's."""
    cam = S.frame_camera()
    world = S.world(name)
    photo = cam.take_photo().samples(4).depth(6).seed(7).mode(mode)
    img = photo.shot(None, world)
    ref, rstats = S.oracle(name).render(cam.desc, photo.settings(), threads=8)
    assert photo.last_stats.segments == rstats.segments
    assert np.array_equal(img, ref), float(np.mean(np.all(img == ref, axis=-1)))
