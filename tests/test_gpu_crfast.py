"""The scatter math's fast paths on the GPU (raysnail_amd/csrc/rs_crfast.h: sincos_cr_fast in random_cosine_direction,
random_cosine_direction_exponent and random_unit, sin3_negative_fast in tex_color; shade_surface's BSDF branch without
its x / x) against the oracle, which keeps calling include/rs_crmath.h's originals: frames and segment counts are equal
bit for bit.

* RTIOW 96 x 60 x 16 at depth 8 (the bench scene: the camera launch's in-place shading, the lean and the heavy launch);
* DiffuseMetal balls (the exponent lobe's sincos and the reflection pdf's quotient), one of them checkered;
* cornell_smoke 48 x 48, the smallest frame the suite renders of a rich-mode scene with an Isotropic medium (random_unit);
* a checker of scale 1e4 on the ground sphere of radius 1000 and on a ball: arguments to 1e7, beyond |k| = 2^20, where
  the sign comes from sin_sign itself;
* one level of ray_color (rs_probe_shade against orc_shade_level, tests/shade_edges.py's worlds and row layout) on
  normals and ray directions at the edges of the pdf's dot product c. What they reach, by the code: c is
  sqrt(1 - r2) |w|^2 plus rounding for the cosine pdf and r2 |w_refl|^2 plus rounding for the reflection pdf, w =
  unit(n), so a finite normal gives c > 0 unless the draw itself is 0. The rows therefore hold: zero, huge (unit(n) = 0)
  and non-finite normals and reflected directions, whose c is NaN (the 1e-5 floor and a NaN quotient); normals of
  denormal length whose squared length rounds in the denormals (|w| != 1, c scaled) or underflows to 0 (w infinite or
  NaN); normals facing away from the ray (the reflection pdf's gate, a negative d.n); normals with denormal components
  beside ordinary ones; a reflected direction of length 1e160, whose squared length overflows (w_refl = 0, every lobe
  draw is NaN and rejected, the lobe returns the normal): c is exactly 0, the pdf 0, the factor 0 / 1e-5; and ordinary
  rows beside them, whose quotient is the 1.0 the fast branch writes. A c that is negative or denormal with a finite
  ONB needs a draw of exactly 0 or 1 (probability 2^-64) and is not among the rows; such values take the unchanged
  expression by the branch's own condition (c >= 2^-1000)."""
import functools
import itertools

import numpy as np
import pytest

import edge_rays as E
import shade_edges as S
from raysnail_amd import scenes
from raysnail_amd.api import CameraBuilder, Checker, Color, Dielectric, DiffuseLight, DiffuseMetal, Glass, Gradient, \
    HittableList, Lambertian, Metal, Point3, Sphere, World

pytestmark = pytest.mark.gpu
SKY = Gradient(Color(0.3, 0.4, 0.5, 1.0), Color(0.7, 0.89, 1.0, 1.0))


def _oracle(world):
    from oracle.binding import OracleScene
    return OracleScene(world)


def _same_frame(world, cam, spp=16, depth=8, seed=5):
    photo = cam.take_photo().samples(spp).depth(depth).seed(seed)
    img = photo.shot(None, world)
    ref, rstats = _oracle(world).render(cam.desc, photo.settings(), threads=16)
    assert photo.last_stats.segments == rstats.segments
    assert np.array_equal(img, ref), float(np.mean(np.all(img == ref, axis=-1)))


def _balls(ground, extra):
    """A ground sphere of radius 1000, a 5 x 5 field of small balls, three larger ones, `extra`, and a light sphere"""
    g = np.random.default_rng(41)
    mats = [Lambertian(Color(0.7, 0.3, 0.2, 1.0)), Metal(Color(0.7, 0.6, 0.5, 1.0)),
            Dielectric(Color(1.0, 1.0, 1.0, 1.0), 1.5).reflect_curve(Glass()), Lambertian(Color(0.2, 0.5, 0.7, 1.0))]
    h = HittableList()
    h.add(Sphere((0.0, -1000.0, 0.0), 1000.0, ground))
    for k, (a, b) in enumerate(itertools.product(range(-2, 3), range(-2, 3))):
        h.add(Sphere((a + 0.9 * g.random(), 0.2, b + 0.9 * g.random()), 0.2, mats[k % 4]))
    h.add(Sphere((0.0, 1.0, 0.0), 1.0, mats[2]))
    h.add(Sphere((-2.2, 0.7, 0.6), 0.7, mats[0]))
    h.add(Sphere((2.1, 0.6, -0.4), 0.6, mats[1]))
    for s in extra:
        h.add(s)
    lights = HittableList()
    light = Sphere((30.0, 40.0, 10.0), 4.0, DiffuseLight(Color(1.0, 0.9, 0.8, 1.0)).multiplier(3.0))
    h.add(light)
    lights.add(light)
    cam = CameraBuilder().look_from(Point3(0.5, 2.5, 9.0)).look_at(Point3(0.0, 0.6, 0.0)).fov(35.0) \
        .aperture(0.05).focus(9.0).width(64).height(40).build()
    return cam, World(h, lights, SKY, (0.0, 0.0))


def test_rtiow_96x60(gpu):
    cam, world, _, _ = scenes.rtow_13_1(96, 60)
    _same_frame(world, cam)


def test_diffuse_metal_balls(gpu):
    extra = [Sphere((1.2, 0.8, 2.0), 0.8, DiffuseMetal(20.0, Color(0.8, 0.7, 0.3, 1.0))),
             Sphere((-1.6, 0.5, 2.6), 0.5, DiffuseMetal(4.0, Checker(Color(0.9, 0.9, 0.9, 1.0), Color(0.2, 0.3, 0.1, 1.0), 10.0))),
             Sphere((0.2, 0.4, 3.2), 0.4, DiffuseMetal(0.0, Color(0.6, 0.7, 0.8, 1.0))),
             Sphere((2.6, 0.5, 1.8), 0.5, DiffuseMetal(300.0, Color(0.9, 0.9, 0.9, 1.0)))]
    cam, world = _balls(DiffuseMetal(2.0, Color(0.5, 0.5, 0.5, 1.0)), extra)
    assert world.device_scene().info().scene_mode == 1
    _same_frame(world, cam, seed=4)


def test_rich_isotropic_medium(gpu):
    cam, world = scenes.cornell_smoke(48, 48)
    assert world.device_scene().info().scene_mode == 0
    _same_frame(world, cam, seed=11)


def test_checker_scale_1e4(gpu):
    big = Checker(Color(0.2, 0.3, 0.1, 1.0), Color(0.9, 0.9, 0.9, 1.0), 1e4)
    cam, world = _balls(Lambertian(big), [Sphere((1.2, 0.8, 2.0), 0.8, Lambertian(big))])
    assert world.device_scene().info().scene_mode == 1
    _same_frame(world, cam, seed=6)


# ---------------------------------------------------------------------------------------------- one level ----
D0 = (0.5, -1.0, 0.25)
T = 2.0 ** -537   # (1.5 T)^2 = 2.25 * 2^-1074: a squared length that rounds in the denormals
EDGE_NORMALS = (
    (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0),                                       # unit(0): NaN
    (1e200, 0.0, 0.0), (1e160, 1e160, 1e160), (0.0, 1.5e154, 0.0),            # len2 = inf: w = 0, u = unit(0)
    (S.INF, 0.0, 0.0), (0.0, -S.INF, 0.0), (S.NAN, 1.0, 0.0),
    (1.5 * T, 0.0, 0.0), (0.0, 1.5 * T, 0.0), (1.5 * T, 0.3 * T, 0.7 * T), (0.0, 2.5 * T, -1.5 * T),   # |w| != 1
    (0.0, 0.75 * T, 0.0), (0.6 * T, 0.6 * T, 0.0),                            # len2 rounds up to / down from 2^-1074
    (2.0 ** -540, 2.0 ** -541, 0.0), (0.0, 2.0 ** -1074, 0.0), (2.0 ** -1074, 2.0 ** -1074, 2.0 ** -1074),  # len2 = 0
    (0.0, 2.0 ** -1074, 2.0 ** -500), (2.0 ** -1060, 1.0, 0.0), (1.0, 2.0 ** -1074, -(2.0 ** -1030)),       # mixed
    (0.0, -1.0, 0.0), (0.0, -3.0, -4.0), (-0.5, 1.0, -0.25),                  # facing away from the ray / along it
    (0.0, 1.0, 0.0), (0.0, 3.0, 4.0), (1e-3, 1.0, 0.0), (0.7, 0.1, -0.7),     # ordinary
)
EDGE_DIR_SCALES = (1.0, 2.0 ** -530, 2.0 ** -540, 1e160)   # the reflected direction's length: rounds, underflows, overflows
EDGE_MATERIALS = ("lam", "checker", "dmetal", "mixed", "mixed_light")
REPS = 6


@functools.lru_cache(maxsize=None)
def _edge_rows(name: str) -> np.ndarray:
    I = S.ids(name)
    rows = []
    for m, n, _ in itertools.product(EDGE_MATERIALS, EDGE_NORMALS, range(REPS)):
        rows.append(S._row(D0, n, I[m]))
    for s, n, _ in itertools.product(EDGE_DIR_SCALES[1:], ((0.0, 1.0, 0.0), (0.0, 3.0, 4.0), (0.0, 1.5 * T, 0.0)), range(REPS)):
        rows.append(S._row(tuple(c * s for c in D0), n, I["dmetal"], t1=0.0))
    r = np.ascontiguousarray(np.array(rows, dtype=np.float64))
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_level_on_pdf_edges(gpu, name):
    r = _edge_rows(name)
    ref = S.oracle(name).shade_level(r, S.SEED)
    ds = S.world(name).device_scene()
    got = np.full(r.shape, -7.0)
    assert ds.lib.rs_probe_shade(ds.handle, r.ctypes.data, len(r), S.SEED, got.ctypes.data) == 0, ds.lib.rs_last_error()
    nan = np.isnan(ref)
    bad = (np.isnan(got) != nan) | ((E.bits(got) != E.bits(ref)) & ~nan)
    rows = np.flatnonzero(np.any(bad, axis=1))
    assert len(rows) == 0, (name, len(rows), [(int(i), r[i].tolist(), got[i].tolist(), ref[i].tolist()) for i in rows[:3]])
    # the rows do reach a NaN factor, the zero pdf and the plain quotient: BSDF-branch rows (the next ray starts at p)
    bsdf = (ref[:, 0] == 1.0) & np.all(E.bits(ref[:, 7:10]) == E.bits(r[:, 7:10]), axis=1)
    factor = ref[:, 4:7]
    assert np.any(bsdf & np.any(np.isnan(factor), axis=1)) and np.any(bsdf & np.all(factor > 0.0, axis=1))
    assert np.any(bsdf & np.all(factor == 0.0, axis=1))
