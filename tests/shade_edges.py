"""Scenes and hit-record families for one level of ray_color after the hit (shade_step / shade_surface / emission,
Obj::random, onb_from, the PDFs, tex_color) where ordinary arithmetic ends: cos_theta exactly 1, refr * sin_theta on
either side of 1, reflections exactly in the surface, normals parallel to (0, 1, 0) and zero normals, light samples
from a light's own centre, texture coordinates at +-0, integers, huge values, NaN and inf.

One world per scene mode (EXPECT_MODE). Each holds every material its mode admits, one small "tag" sphere per
material in a row at y = 1, z = 2 (a ray down -z at tag k reports material id k: MATERIALS' order is the id order), and
a lights list with every hittable kind the mode admits, a moving sphere among them; the list lengths are 3, 8, 10, 14
and 15. The rows of a scene are synthetic records for rs_probe_shade / orc_shade_level: 18 doubles = ray o d time,
hit p n t1 outside u v material id; they come in named families (FAMILIES), one per edge.

A plain helper module (like edge_rays.py): tests/test_shade_edges_cpu.py guards these fixtures on the oracle,
tests/test_gpu_shade_edges.py compares the GPU's level with the oracle's on them.
"""
from __future__ import annotations

import functools
import itertools
import math
from fractions import Fraction

import numpy as np

import edge_rays as E
from raysnail_amd import scenes
from raysnail_amd.api import (AARect, AARectMetrics, BlinnPhong, Box, CameraBuilder, Checker, CommonMaterialSettings,
                              ConstantMedium, Dielectric, Difference, DiffuseLight, DiffuseMetal, Glass, Gradient,
                              HittableList, Intersection, Isotropic, Lambertian, Metal, MixedMaterial, Perlin,
                              SmoothType, Sphere, TfFacade, Transform, TriangleMesh, World)
from raysnail_amd.scenes import C32

SEED = 20
NAN, INF = float("nan"), float("inf")
SCENE_NAMES = ("spheres", "flat", "nest0", "nest2", "rich")
EXPECT_MODE = {"spheres": 1, "flat": 2, "nest0": 3, "nest2": 4, "rich": 0}
N_LIGHTS = {"spheres": 3, "flat": 8, "nest0": 10, "nest2": 14, "rich": 15}
# material names in id order (MixedMaterials after their parts); the rich scene appends RICH_MATERIALS
MATERIALS = ("lam", "lam_phong", "checker", "metal", "dmetal", "glass", "diel", "light", "mixed", "mixed_light")
RICH_MATERIALS = ("blinn", "iso", "perlin_none", "perlin_vec", "perlin_marble", "image")
LAM_COLOR = (0.7, 0.3, 0.2)   # lam and lam_phong: the same colour, so only light_multi tells them apart
COS_PDF = 0.3183098861837907  # camera.rs's pdf_val of the light branch


def materials(rich: bool):
    lam = Lambertian(C32(*LAM_COLOR))
    metal = Metal(C32(0.8, 0.8, 0.7))
    dmetal = DiffuseMetal(8.0, C32(0.6, 0.7, 0.8))
    light = DiffuseLight(Checker(C32(1.0, 0.5, 0.25), C32(0.5, 1.0, 0.75), 2.0)).multiplier(4.0)
    m = {
        "lam": lam,
        "lam_phong": Lambertian(C32(*LAM_COLOR)).set(CommonMaterialSettings(0.5, 4)),
        "checker": Lambertian(Checker(C32(0.1, 0.2, 0.3), C32(0.9, 0.8, 0.7), 2.0)),
        "metal": metal, "dmetal": dmetal,
        "glass": Dielectric(C32(0.9, 1.0, 0.95), 1.5).reflect_curve(Glass()),
        "diel": Dielectric(C32(0.95, 0.9, 1.0), 1.5),
        "light": light,
        "mixed": MixedMaterial(lam, metal, 0.5),
        "mixed_light": MixedMaterial(light, dmetal, 0.25),
    }
    if rich:
        m.update({
            "blinn": BlinnPhong(0.5, 4.0, C32(0.99, 0.69, 0.2)),
            "iso": Isotropic(C32(0.4, 0.5, 0.6)),
            "perlin_none": Lambertian(Perlin(64, False, 5).smooth(SmoothType.None_).scale(3.0)),
            "perlin_vec": Lambertian(Perlin(256, True, 2).scale(4.0)),
            "perlin_marble": Lambertian(Perlin(256, True, 2).scale(4.0).marble(5)),
            "image": Lambertian(scenes.synthetic_image(64, 32, seed=11)),
        })
    return m


def material_names(name: str):
    return MATERIALS + (RICH_MATERIALS if name == "rich" else ())


def ids(name: str):
    """material name -> id (the order the tag spheres use them in; "default": -1, the world's default material)."""
    d = {n: k for k, n in enumerate(material_names(name))}
    d["default"] = -1
    return d


# the lights' positions: rows of the `lights` and `onb_zero` families start from them
SPHERE_LIGHT_CENTRES = ((0.0, 4.0, 0.0), (-3.0, 3.0, 1.0))
MOVING_LIGHT_CENTRE = (3.0, 4.0, 0.0)
QUADRIC_LIGHT_CENTRE = (2.0, 2.0, 2.0)


def _lights(name: str, light):
    """The lights list of a scene: every kind the mode admits (Obj::random's cases), a moving sphere second."""
    out = [Sphere(SPHERE_LIGHT_CENTRES[0], 1.0, light),
           Sphere(MOVING_LIGHT_CENTRE, 0.5, light).with_speed((0.0, 0.5, 0.0)),
           Sphere(SPHERE_LIGHT_CENTRES[1], 0.5, light)]
    if name == "spheres":
        return out
    out.append(AARect.new_xz(AARectMetrics(6.0, (-1.0, 1.0), (-1.0, 1.0)), light))
    out.append(AARect.new_xy(AARectMetrics(-4.0, (-2.0, 2.0), (1.0, 3.0)), light))   # rect.rs's xz formula as it stands
    out.append(AARect.new_yz(AARectMetrics(-5.0, (1.0, 3.0), (-2.0, 2.0)), light))
    tri = np.array([[1.0, 1.0, -3.0, 3.0, 1.0, -3.0, 3.0, 3.0, -3.0], [1.0, 1.0, -3.0, 3.0, 3.0, -3.0, 1.0, 3.0, -3.0]])
    out.append(TriangleMesh(tri, None, light))                                        # two entries: origin - p0
    if name == "flat":
        return out
    cx, cy, cz = QUADRIC_LIGHT_CENTRE
    out.append(E._quadric(light, xx=1.0, yy=1.0, zz=1.0, x=-2 * cx, y=-2 * cy, z=-2 * cz, c=11.75))  # radius 1/2: -origin
    out.append(Box((-3.0, 1.0, -3.0), (-2.0, 2.0, -2.0), light))                      # the constant (1, 0, 0)
    if name == "nest0":
        return out
    # only the origin is inverse-transformed (tf_facade.rs): a scaled and a rotated one
    out.append(TfFacade(Sphere((0.0, 0.0, 0.0), 0.5, light),
                        E._stack(Transform.scale((1.0, 2.0, 1.0)), Transform.translate((4.0, 2.0, -2.0)))))
    out.append(TfFacade(AARect.new_xz(AARectMetrics(0.0, (-0.5, 0.5), (-0.5, 0.5)), light),
                        E._stack(Transform.rotate_by_z_axis(math.pi / 2), Transform.translate((-4.0, 2.0, -2.0)))))
    out.append(Intersection(Sphere((1.0, 6.0, -3.0), 0.75, None), Box((0.5, 5.5, -3.5), (1.5, 6.5, -2.5), None), light))
    out.append(Difference(Box((-1.5, 5.0, -4.0), (-0.5, 6.0, -3.0), light), Sphere((-1.0, 5.5, -3.0), 0.5, None), None))
    if name == "nest2":
        return out
    out.append(ConstantMedium(Sphere((4.0, 5.0, 1.0), 0.5, None), C32(0.9, 0.9, 0.9), 2.0))  # the constant (1, 0, 0)
    return out


def _scene(name: str) -> World:
    rich = name == "rich"
    mats = materials(rich)
    h, lights = HittableList(), HittableList()
    for k, n in enumerate(material_names(name)):          # the tag spheres fix the material ids: first use
        h.add(Sphere((k - 8.0, 1.0, 2.0), 0.25, mats[n]))
    h.add(Sphere((9.0, 1.0, 2.0), 0.25, None))            # the world's default material
    if name == "spheres":
        h.add(Sphere((0.0, -100.0, 0.0), 100.0, mats["checker"]))
    else:
        h.add(AARect.new_xz(AARectMetrics(0.0, (-10.0, 10.0), (-10.0, 10.0)), mats["checker"]))
    if name in ("nest2", "rich"):                         # a TfFacade over a CSG node: nesting depth 2
        cyl = Intersection(E._quadric(None, xx=1.0, zz=1.0, c=-1.0), Box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), None),
                           mats["dmetal"])
        h.add(TfFacade(cyl, E._stack(Transform.scale((0.5, 1.0, 0.5)), Transform.translate((2.0, 1.0, -1.0)))))
    for o in _lights(name, mats["light"]):
        h.add(o)
        lights.add(o)
    return World(h, lights, Gradient(C32(0.3, 0.4, 0.5), C32(0.7, 0.89, 1.0)), (0.0, 1.0))


@functools.lru_cache(maxsize=None)
def world(name: str) -> World:
    return _scene(name)


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    from oracle.binding import OracleScene
    return OracleScene(world(name))


def frame_camera():
    return CameraBuilder().look_from((0.5, 4.0, 14.0)).look_at((0.0, 3.0, 0.0)).fov(60.0).aperture(0.0) \
        .width(32).height(20).shutter_speed(1.0).build()


# ------------------------------------------------------------------------------- exact helpers ----
def len2(x: float, y: float, z: float) -> float:
    """vec3.rs:152-155 z.mul_add(z, x.mul_add(x, y * y)), exactly (a fused multiply-add rounds once)."""
    inner = float(Fraction(x) * Fraction(x) + Fraction(y * y))
    return float(Fraction(z) * Fraction(z) + Fraction(inner))


def unit(v):
    inv = 1.0 / math.sqrt(len2(*v))
    return (v[0] * inv, v[1] * inv, v[2] * inv)


def onb_takes_fallback(n) -> bool:
    """onb.rs:26-40: does ONB::build_from(n) take the (1, 0, 0) axis (|up x w|^2 < 1e-8)?"""
    w = unit(n)
    uc = (1.0 * w[2] - 0.0 * w[1], 0.0 * w[0] - 0.0 * w[2], 0.0 * w[1] - 1.0 * w[0])
    return len2(*uc) < 0.00000001


_M64, _M32 = (1 << 64) - 1, (1 << 32) - 1


def _splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class Rng:
    """The row's stream, restated: rand_core 0.6 seed_from_u64 (PCG32 expansion) of rs_stream_key(seed, 0, row, 0),
    rand_xorshift's XorShiftRng, gen() = next_u64 / 2^64. Checked against the oracle's words in the CPU tests."""

    def __init__(self, seed: int, row: int):
        st = _splitmix64(_splitmix64(_splitmix64(_splitmix64(seed) ^ 0) ^ row) ^ 0)
        s = []
        for _ in range(4):
            st = (st * 6364136223846793005 + 11634580027462260723) & _M64
            xs = (((st >> 18) ^ st) >> 27) & _M32
            rot = st >> 59
            s.append(((xs >> rot) | (xs << ((32 - rot) & 31))) & _M32)
        if not any(s):
            s = [0x0BAD5EED] * 4
        self.s = s

    def next_u32(self) -> int:
        x, y, z, w = self.s
        t = (x ^ (x << 11)) & _M32
        w2 = w ^ (w >> 19) ^ (t ^ (t >> 8))
        self.s = [y, z, w, w2]
        return w2

    def gen(self) -> float:
        lo = self.next_u32()
        hi = self.next_u32()
        return float((hi << 32) | lo) / 18446744073709551616.0

    def words(self):
        return [float(v) for v in self.s]


# ------------------------------------------------------------------------------- rows ----
FAMILIES = ("generic", "diel_normal", "diel_tir", "diel_nan", "metal_graze", "onb_up", "onb_near", "onb_zero",
            "light_start", "pdf_floor", "phong_lambert", "checker_zero", "lights", "blinn_same", "perlin_edges",
            "image_uv")
RICH_ONLY = ("blinn_same", "perlin_edges", "image_uv")
AXES = ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0))
P0 = (0.5, 2.0, -1.5)


def _row(d, n, mat, p=P0, t1=2.0, outside=1.0, u=0.25, v=0.75, time=0.0, o=None):
    """A record on the ray: o = p - t1 d unless given (so p != ray_at(t1 - 0.0002) whenever d != 0, and a next ray
    that starts at p is a BSDF-branch ray)."""
    d, p = np.asarray(d, float), np.asarray(p, float)
    if o is None:
        with np.errstate(invalid="ignore", over="ignore"):
            o = p - t1 * d
    return [*o, *d, time, *p, *n, t1, outside, u, v, float(mat)]


def _facing(d, n):
    """(n or -n, outside) as HitRecord::new stores them (hit.rs:32-53)."""
    out = float(np.dot(d, n)) < 0.0
    return (tuple(n) if out else tuple(-c for c in n)), (1.0 if out else 0.0)


def _generic(I, name):
    rows = []
    dirs = E.d_axis()[::5]
    for m in list(material_names(name)) + ["default"]:
        for k, d in enumerate(dirs):
            for a in (0, 2, 4):
                n, outside = _facing(d, AXES[a])
                rows.append(_row(d, n, I[m], p=(k - 5.0, a * 0.5, 1.0 - k), outside=outside, time=0.25 * (k % 4)))
    return rows


def _diel_normal(I, name):
    """cos_theta exactly 1: d = -n on the axes. `diel` always refracts (reflect_prob 0), `glass` reflects with r0."""
    rows = []
    for m, rep in (("diel", 2), ("glass", 16)):
        for n, outside, _ in itertools.product(AXES, (0.0, 1.0), range(rep)):
            rows.append(_row(tuple(-c for c in n), n, I[m], outside=outside))
    return rows


TIR_S = 2.0 / 3.0   # sin_theta at which 1.5 * sin_theta crosses 1


def _tir_sines():
    s = list(np.linspace(0.55, 0.8, 41))
    near = [TIR_S]
    for _ in range(4):
        near = [np.nextafter(near[0], 0.0)] + near + [np.nextafter(near[-1], 1.0)]
    return s + near


def _diel_tir(I, name):
    """refr * sin_theta on either side of 1: d = (s, -sqrt(1 - s^2), 0) against n = (0, 1, 0), from inside (refr =
    1.5, total reflection above s = 2/3) and from outside (refr = 1/1.5, never)."""
    rows = []
    for m, outside, s in itertools.product(("diel", "glass"), (0.0, 1.0), _tir_sines()):
        rows.append(_row((s, -math.sqrt(1.0 - s * s), 0.0), (0.0, 1.0, 0.0), I[m], outside=outside))
    return rows


def _diel_nan(I, name):
    """1 - |r_parallel|^2 below 0: directions that are not unit vectors (a refracted direction is never normalised
    upstream). d = (k, -1, 0) has cos_theta = 1, so nothing reflects totally, and r_parallel = (k refr, 0, 0): a NaN
    direction with a finite factor for k refr > 1. d = (0, -2, 0): sin_theta itself is NaN."""
    rows = []
    for m, outside, k in itertools.product(("diel", "glass"), (0.0, 1.0), (0.25, 0.5, 1.0, 1.25, 1.5, 1.75, 2.0, 4.0)):
        rows.append(_row((k, -1.0, 0.0), (0.0, 1.0, 0.0), I[m], outside=outside))
        rows.append(_row((0.0, -2.0 * k, 0.0), (0.0, 1.0, 0.0), I[m], outside=outside))
    return rows


def _metal_graze(I, name):
    """dot(reflected, n) exactly 0 (absorbed: !(.. > 0)), a hair on either side, and normal incidence."""
    rows = []
    e = 2.0 ** -60
    for m in ("metal", "dmetal"):
        for n in AXES:
            for d in E.d_axis():
                if float(np.dot(d, n)) == 0.0:
                    rows.append(_row(d, n, I[m]))
            a = AXES[(AXES.index(n) + 2) % 6]                      # an axis perpendicular to n
            for s in (e, -e, 0.5, -0.5):
                rows.append(_row(tuple(a[i] + s * n[i] for i in range(3)), n, I[m]))
            rows.append(_row(tuple(-c for c in n), n, I[m]))        # normal incidence: reflected = -d
    return rows


def _onb_up(I, name):
    """ONB::build_from of a normal parallel to (0, 1, 0): the (1, 0, 0) fallback, with every sign of zero."""
    rows = []
    for s, zx, zz, _ in itertools.product((1.0, -1.0, 2.0, -2.0, 2.0 ** -20, -1e-5), (0.0, -0.0), (0.0, -0.0), range(3)):
        rows.append(_row((0.25, -1.0, 0.5), (zx, s, zz), I["lam"]))
    return rows


def onb_near_normals():
    eps = [1e-4 * (1.0 + j * 2.0 ** -30) for j in range(-40, 41)] + [1e-5, 3e-5, 3e-4, 1e-3]
    out = []
    for e in eps:
        out += [(e, 1.0, 0.0), (0.0, 1.0, -e), (e, -1.0, 0.5 * e)]
    return out


def _onb_near(I, name):
    """|up x w|^2 just on either side of 1e-8: normals (eps, 1, 0) with eps around 1e-4."""
    return [_row((0.25, -1.0, 0.5), n, I["lam"], outside=1.0 if n[1] > 0 else 0.0) for n in onb_near_normals()]


def _light_points(name):
    pts = list(SPHERE_LIGHT_CENTRES) + [MOVING_LIGHT_CENTRE, (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)]
    if name not in ("spheres", "flat"):
        pts.append(QUADRIC_LIGHT_CENTRE)
    return pts


def _onb_zero(I, name):
    """unit(0): a light sample from a hit point at a sphere light's centre (Sphere::random's ONB of centre -
    origin) or at the origin under a quadric light (-origin); and a zero normal."""
    rows = []
    for p, _ in itertools.product(_light_points(name), range(64)):
        rows.append(_row((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), I["lam"], p=p))
    for m, _ in itertools.product(("lam", "dmetal"), range(12)):
        rows.append(_row((0.5, -1.0, 0.0), (0.0, 0.0, 0.0), I[m]))
    return rows


LIGHT_START_T1 = (0.0, -0.0, 1e-300, 1e-4, float(np.nextafter(0.0002, 0.0)), 0.0002, float(np.nextafter(0.0002, 1.0)),
                  0.0003, 1.0)


def _light_start(I, name):
    """The light ray's start ray_at(t1 - 0.0002) with t1 below, at and above 0.0002."""
    rows = []
    for m, t1, k in itertools.product(("lam", "dmetal"), LIGHT_START_T1, range(6)):
        d = AXES[k]
        n = tuple(-c for c in d)
        o = (1.0, 2.0, -1.0)
        p = tuple(o[i] + t1 * d[i] for i in range(3))
        rows.append(_row(d, n, I[m], p=p, t1=t1, o=o))
    return rows


def _pdf_floor(I, name):
    """pdf_val <= 0 or NaN -> 1e-5. The cosine and reflection PDFs of a sampled direction are positive unless the
    normal's ONB is NaN (a zero, an infinite or a NaN normal); BlinnPhong's value goes negative for a short incoming
    ray that leaves the surface (rich scene). Ordinary rows stand beside them: not replaced."""
    rows = []
    for n, _ in itertools.product(((0.0, 0.0, 0.0), (INF, 0.0, 0.0), (NAN, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 3.0, 4.0)),
                                  range(12)):
        rows.append(_row((0.5, -1.0, 0.25), n, I["lam"]))
    if name == "rich":
        for s, _ in itertools.product((2.0 ** -4, 2.0 ** -10, 1.0), range(16)):
            rows.append(_row((0.5 * s, 1.0 * s, 0.25 * s), (0.0, 1.0, 0.0), I["blinn"]))
    return rows


def _phong_lambert(I, name):
    """phong_highlight on a Lambertian with phong_factor > 0: lam_phong (test twin: the same rows with `lam`)."""
    rows = []
    for d, a, _ in itertools.product(E.d_axis()[::5], (0, 2, 4), range(4)):
        n, outside = _facing(d, AXES[a])
        rows.append(_row(d, n, I["lam_phong"], outside=outside))
    return rows


def _checker_zero(I, name):
    """Checker's sin(s x) sin(s y) sin(s z) < 0 on the planes where a sine is exactly +0 or -0."""
    rows = []
    for m in ("checker", "light"):
        for p in itertools.product((-0.0, 0.0, 0.5, -0.5, 1.0, -1.0), repeat=3):
            rows.append(_row((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), I[m], p=p, o=(p[0], p[1], p[2] + 2.0)))
        for c in (NAN, INF, -INF, 1e300, -(2.0 ** 60)):            # and where a sine has no value or no period left
            for p in ((c, 0.5, 0.5), (0.5, c, 0.5), (0.5, 0.5, c), (c, c, c)):
                rows.append(_row((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), I[m], p=p, o=(0.0, 0.0, 2.0)))
    return rows


def _lights_family(I, name):
    """Obj::random of every light in the list, from hit points on and off the lights, at their centres and at the
    origin, at several times (the moving light's centre does not follow them upstream)."""
    pts = _light_points(name) + [(0.0, 5.0, 0.0), (0.0, 6.0, 0.0), (-2.5, 1.5, -2.5), (1.0, 1.0, -3.0), (0.3, 0.7, -1.1),
                                 (4.0, 2.0, -2.0), (-4.0, 2.0, -2.0), (-5.0, 2.0, 0.0)]
    rows = []
    for k, (p, j) in enumerate(itertools.product(pts, range(28))):
        rows.append(_row((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), I["lam_phong" if j % 4 == 3 else "lam"], p=p,
                         time=(0.0, 0.5, 1.0)[k % 3]))
    return rows


def _blinn_same(I, name):
    """BlinnPhongPdf's unit(-r_in + d) with d == r_in: the Box and ConstantMedium lights' direction is the constant
    (1, 0, 0), and so is the ray's."""
    rows = []
    for n, _ in itertools.product(((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)), range(48)):
        rows.append(_row((1.0, 0.0, 0.0), n, I["blinn"], outside=1.0 if n[0] < 0 else 0.0))
    return rows


PERLIN_COORDS = (0.0, -0.0, 1.0, -1.0, 3.0, -7.0, 0.25, -0.25, 2.0 ** 31, -(2.0 ** 31), 2.0 ** 63, -(2.0 ** 63), 1e19,
                 -1e19, 1e300, INF, -INF, NAN)


def _perlin_edges(I, name):
    """perlin_noise at integer, negative and huge coordinates (as_isize saturates), at inf and at NaN."""
    rows = []
    for m in ("perlin_none", "perlin_vec", "perlin_marble"):
        for c in PERLIN_COORDS:
            for p in ((c, 0.25, 0.25), (0.25, c, 0.25), (0.25, 0.25, c), (c, c, c)):
                rows.append(_row((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), I[m], p=p, o=(0.0, 0.0, 2.0)))
    return rows


IMAGE_UV = (0.0, -0.0, 0.5, float(np.nextafter(1.0, 0.0)), 1.0, float(np.nextafter(1.0, 2.0)), -(2.0 ** -1074),
            -(2.0 ** -52), NAN, INF, -INF)


def _image_uv(I, name):
    """image_texel at u, v in {+-0, 1, 1 + ulp, -ulp, NaN, +-inf}."""
    return [_row((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), I["image"], u=u, v=v) for u, v in itertools.product(IMAGE_UV, IMAGE_UV)]


_BUILDERS = {"generic": _generic, "diel_normal": _diel_normal, "diel_tir": _diel_tir, "diel_nan": _diel_nan,
             "metal_graze": _metal_graze, "onb_up": _onb_up, "onb_near": _onb_near, "onb_zero": _onb_zero,
             "light_start": _light_start, "pdf_floor": _pdf_floor, "phong_lambert": _phong_lambert,
             "checker_zero": _checker_zero, "lights": _lights_family, "blinn_same": _blinn_same,
             "perlin_edges": _perlin_edges, "image_uv": _image_uv}


def families(name: str):
    return tuple(f for f in FAMILIES if name == "rich" or f not in RICH_ONLY)


@functools.lru_cache(maxsize=None)
def rows(name: str):
    """(rows (n, 18), family (n,) index into FAMILIES): every family of the scene in one table, one probe call."""
    I = ids(name)
    out, fam = [], []
    for f in families(name):
        r = _BUILDERS[f](I, name)
        out += r
        fam += [FAMILIES.index(f)] * len(r)
    r = np.ascontiguousarray(np.array(out, dtype=np.float64))
    assert r.shape[1] == 18 and len(r) < 10000
    r.setflags(write=False)
    return r, np.array(fam)


def family_rows(name: str, family: str) -> np.ndarray:
    return np.flatnonzero(rows(name)[1] == FAMILIES.index(family))


@functools.lru_cache(maxsize=None)
def reference(name: str) -> np.ndarray:
    """The oracle's level on the scene's rows: computed once, shared, read-only."""
    ref = oracle(name).shade_level(rows(name)[0], SEED)
    ref.setflags(write=False)
    return ref


def light_branch(r: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """(n,) bool: the level continued with a light sample (the next ray does not start at the hit point; only
    meaningful for the materials that sample: not Metal / Dielectric)."""
    return (ref[:, 0] == 1.0) & np.any(E.bits(ref[:, 7:10]) != E.bits(r[:, 7:10]), axis=1)
