"""Scenes and ray families for World::hit where ordinary arithmetic ends: direction components that are
exactly +0 / -0 / subnormal / tiny, origins exactly on bounding-box planes, on surfaces and at centres,
tangent rays (discriminant exactly 0) and objects hit at exactly the same t.

Every coordinate of every scene is an integer or a half-integer (a few spheres aside, where a scene wants
objects off the lattice), so every plane, centre and tangent point is exact in binary. The origins are the
lattice {-3, -2.5, ..., 3}^3; the directions are the families D_axis, D_scaled and D_near below.

A plain helper module (like features_ref.py): tests/test_edge_rays_cpu.py guards these fixtures on the CPU,
tests/test_gpu_edge_rays.py compares the GPU's records with the oracle's on them.
"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
import math

import numpy as np

from raysnail_amd import scenes
from raysnail_amd.api import (AARect, AARectMetrics, BlinnPhong, Box, CameraBuilder, ConstantMedium, Dielectric,
                              Difference, DiffuseLight, Glass, Gradient, HittableList, Intersection, Lambertian, Metal,
                              Perlin, Quadric, SmoothType, Sphere, TfFacade, Transform, TransformStack, TriangleMesh,
                              World)
from raysnail_amd.scenes import C32

INF = float("inf")
TMINS = (0.0, 1e-4, 0.5)
FAMILIES = ("axis", "scaled", "near")   # (the `nonfinite` family is a table of its own: nonfinite_rays())
# what DeviceScene(world, devices=[]).info() must say: (scene_mode, tree_arity or None, ref_order)
EXPECT_INFO = {"spheres": (1, 4, 0), "spheres_moving": (1, 4, 0), "flat": (2, None, 0), "nest0": (3, None, 1),
               "nest2": (4, None, 1), "rich": (0, None, 1)}
NEAR_FIRST = ("spheres", "spheres_moving", "flat")
REF_ORDER = ("nest0", "nest2", "rich")
MOVING_TIMES = (0.0, 0.25, 1.0, 2.0, -1.0)  # the last two outside the range the boxes were built for


# ------------------------------------------------------------------------------- scenes ----
def _world(h: HittableList, time_range=(0.0, 0.0)) -> World:
    lights = HittableList()
    lamp = Sphere((0.0, 64.0, 0.0), 8.0, DiffuseLight(C32(1.0, 0.9, 0.8)).multiplier(4.0))
    h.add(lamp)
    lights.add(lamp)
    return World(h, lights, Gradient(C32(0.3, 0.4, 0.5), C32(0.7, 0.89, 1.0)), time_range)


def _sphere_mats():
    return [Lambertian(C32(0.7, 0.3, 0.2)), Metal(C32(0.8, 0.8, 0.7)),
            Dielectric(C32(1.0, 1.0, 1.0), 1.5).reflect_curve(Glass()), Lambertian(C32(0.2, 0.5, 0.8))]


def spheres(moving: bool = False) -> World:
    """5 x 5 x 2 spheres of radius 0.5 at unit spacing: they touch, so rays through the tangent points tie, and
    the lattice rays in their boxes' face planes are tangent (delta == 0). Box planes at x, z = +-0.5, +-1.5,
    +-2.5 and y = -1, 0, 1."""
    h = HittableList()
    mats = _sphere_mats()
    speeds = {(0, 0, 0): (0.5, 0.0, 0.0), (2, 1, 3): (0.0, 0.5, 0.0), (4, 0, 4): (0.0, 0.0, -1.0)}
    for i, j, k in itertools.product(range(5), range(2), range(5)):
        s = Sphere((i - 2.0, j - 0.5, k - 2.0), 0.5, mats[(i + 2 * j + 3 * k) % 4])
        if moving and (i, j, k) in speeds:
            s.with_speed(speeds[(i, j, k)])
        h.add(s)
    return _world(h, (0.0, 1.0) if moving else (0.0, 0.0))


def _lattice_mesh(material) -> TriangleMesh:
    """4 x 4 quads on integer vertices over x, z in [-2, 2] at y = -2: shared edges and vertices on lattice rays.
    Planar on purpose: a lattice ray parallel to a slanted triangle's plane gets t = +-inf from Triangle::hit's
    division by zero, which the closed range end accepts, and a record of NaNs (test_gpu_edge_rays.py checks that
    case on its own, without bit patterns)."""
    return _grid_mesh(material, lambda i, j: -2.0)


def _grid_mesh(material, height) -> TriangleMesh:
    def v(i, j):
        return (i - 2.0, height(i, j), j - 2.0)
    tris = []
    for i, j in itertools.product(range(4), range(4)):
        a, b, c, d = v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)
        tris.append(a + b + c)
        tris.append(a + c + d)
    return TriangleMesh(np.array(tris), None, material)


def flat() -> World:
    """Spheres, rects and triangles only: 5 x 5 touching spheres, two coplanar overlapping xz rects with different
    materials (overlap [-1, 1]^2 at y = -1), an xy and a yz rect, and the lattice mesh."""
    h = HittableList()
    mats = _sphere_mats()
    for i, k in itertools.product(range(5), range(5)):
        h.add(Sphere((i - 2.0, 0.5, k - 2.0), 0.5, mats[(i + 3 * k + 2) % 4]))  # glass at (0, 0.5, 0), (2, 0.5, 2)
    h.add(AARect.new_xz(AARectMetrics(-1.0, (-3.0, 1.0), (-3.0, 1.0)), Lambertian(C32(0.8, 0.2, 0.2))))
    h.add(AARect.new_xz(AARectMetrics(-1.0, (-1.0, 3.0), (-1.0, 3.0)), Lambertian(C32(0.2, 0.8, 0.2))))
    h.add(AARect.new_xy(AARectMetrics(-3.0, (-3.0, 3.0), (-3.0, 3.0)), Lambertian(C32(0.6, 0.6, 0.6))))
    h.add(AARect.new_yz(AARectMetrics(3.0, (-3.0, 3.0), (-3.0, 3.0)), Metal(C32(0.7, 0.7, 0.8))))
    h.add(_lattice_mesh(Lambertian(C32(0.5, 0.5, 0.3))))
    return _world(h)


def _quadric(material, xx=0.0, yy=0.0, zz=0.0, x=0.0, y=0.0, z=0.0, c=0.0) -> Quadric:
    """xx x^2 + yy y^2 + zz z^2 + x x + y y + z z + c = 0 (quadric.rs field order qa .. qj)."""
    return Quadric(xx, 0.0, 0.0, x, yy, 0.0, y, zz, z, c, material)


def nest0() -> World:
    """Leaf objects whose records depend on the range end (reference order), no nesting: boxes that share faces,
    edges and a corner, a box face coplanar with a rect, bare quadrics -- a cylinder, a cone with its apex on the
    lattice point (-2, 1, 2) (quadric_normal's len == 0), a paraboloid (a == 0 for rays along y) and a plane-like
    form without quadratic terms (a == 0 always, b == 0 for rays in the plane) -- and two spheres off the lattice."""
    h = HittableList()
    lam = [Lambertian(C32(0.7, 0.6, 0.5)), Lambertian(C32(0.3, 0.6, 0.4)), Metal(C32(0.8, 0.8, 0.8))]
    h.add(Box((-2.0, -1.0, -1.0), (-1.0, 0.0, 0.0), lam[0]))
    h.add(Box((-1.0, -1.0, -1.0), (0.0, 0.0, 0.0), lam[1]))   # shares the face x = -1
    h.add(Box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), lam[2]))      # shares the corner (0, 0, 0)
    h.add(Box((0.0, -1.0, 0.0), (1.0, 0.0, 1.0), lam[0]))     # shares the face y = 0 / an edge
    h.add(AARect.new_xz(AARectMetrics(-1.0, (-3.0, 1.0), (-2.0, 1.0)), lam[1]))  # coplanar with three box bottoms
    h.add(_quadric(lam[2], xx=1.0, zz=1.0, x=-4.0, z=4.0, c=7.75))       # cylinder (x-2)^2 + (z+2)^2 = 1/4
    # cone (x+2)^2 + (z-2)^2 = (y-1)^2 / 4, apex (-2, 1, 2)
    h.add(_quadric(lam[0], xx=1.0, yy=-0.25, zz=1.0, x=4.0, y=0.5, z=-4.0, c=7.75))
    h.add(_quadric(lam[1], xx=1.0, zz=1.0, x=-4.0, y=-1.0, z=-4.0, c=5.0))  # paraboloid (x-2)^2 + (z-2)^2 = y + 3
    h.add(_quadric(lam[2], y=1.0, c=3.0))                                # the plane y = -3
    h.add(Sphere((1.3, 0.7, -1.1), 0.45, Dielectric(C32(1.0, 1.0, 1.0), 1.5).reflect_curve(Glass())))
    h.add(Sphere((-1.7, 1.9, 0.4), 0.6, lam[2]))
    return _world(h)


def _stack(*tfs) -> TransformStack:
    st = TransformStack()
    for t in tfs:
        st.push(t)
    return st


def nest2() -> World:
    """TfFacade over Intersection(quadric, box) with translate, a rotation by 90 degrees and a scale; a
    Difference(box, sphere); an Intersection whose children touch in one point; a plain sphere and a floor rect."""
    h = HittableList()
    lam = [Lambertian(C32(0.8, 0.7, 0.5)), Lambertian(C32(0.5, 0.8, 0.7)), Metal(C32(0.8, 0.8, 0.8))]
    unit = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    cyl = Intersection(_quadric(None, xx=1.0, zz=1.0, c=-1.0), Box(*unit, None), lam[0])
    h.add(TfFacade(cyl, _stack(Transform.translate((-2.0, 0.0, -1.0)))))
    cone = Intersection(_quadric(None, xx=1.0, yy=-1.0, zz=1.0), Box(*unit, None), lam[1])
    h.add(TfFacade(cone, _stack(Transform.rotate_by_z_axis(math.pi / 2), Transform.translate((2.0, 0.0, 1.0)))))
    ball = Intersection(_quadric(None, xx=1.0, yy=1.0, zz=1.0, c=-1.0), Box((-1.0, -1.0, -1.0), (1.0, 0.5, 1.0), None),
                        lam[2])
    h.add(TfFacade(ball, _stack(Transform.scale((0.5, 1.0, 0.5)), Transform.translate((0.0, 2.0, -2.0)))))
    h.add(Difference(Box((-1.0, -3.0, -1.0), (1.0, -2.0, 1.0), lam[0]), Sphere((0.0, -2.0, 0.0), 0.5, lam[1]), None))
    h.add(Intersection(Sphere((0.0, 0.0, 2.0), 0.5, None), Box((0.5, -0.5, 1.5), (1.5, 0.5, 2.5), None), lam[1]))
    h.add(Sphere((-2.0, 2.0, 2.0), 0.5, Dielectric(C32(1.0, 1.0, 1.0), 1.5).reflect_curve(Glass())))
    h.add(AARect.new_xz(AARectMetrics(-3.0, (-3.0, 3.0), (-3.0, 3.0)), lam[0]))
    return _world(h)


def rich() -> World:
    """The generic mode: ConstantMedium over a box and over a sphere, an Image texture on a sphere (its poles and
    the atan2 seam on lattice rays) and on a rect, so (u, v) are written, BlinnPhong and Perlin materials, a
    Difference."""
    h = HittableList()
    img = scenes.synthetic_image(64, 32, seed=11)
    h.add(ConstantMedium(Box((-2.0, -1.0, -2.0), (0.0, 1.0, 0.0), None), C32(0.2, 0.4, 0.9), 2.0))
    h.add(ConstantMedium(Sphere((1.0, 0.0, 1.0), 1.0, None), C32(0.9, 0.9, 0.9), 1.5))
    h.add(Sphere((2.0, -1.0, -1.0), 1.0, Lambertian(img)))
    h.add(AARect.new_xy(AARectMetrics(-3.0, (-3.0, 3.0), (-3.0, 3.0)), Lambertian(img)))
    h.add(Sphere((-2.0, -2.0, 2.0), 0.5, BlinnPhong(0.5, 4.0, C32(0.99, 0.69, 0.2))))
    h.add(Sphere((1.0, 2.0, -2.0), 0.5, Lambertian(Perlin(64, False, 5).smooth(SmoothType.None_).scale(3.0))))
    h.add(Sphere((-1.0, 2.0, 1.0), 0.5, Lambertian(Perlin(256, True, 2).scale(4.0).marble(5))))
    h.add(Difference(Box((0.0, -3.0, 0.0), (2.0, -2.0, 2.0), Lambertian(C32(0.8, 0.2, 0.2))),
                     Sphere((1.0, -2.0, 1.0), 0.5, None), None))
    return _world(h)


def slanted() -> World:
    """Not one of SCENES (its oracle records hold NaNs): the grid mesh with every odd-odd vertex raised to y = -1,
    45-degree faces that lattice rays run parallel to. Triangle::hit then divides by zero, and its closed range end
    accepts t = +inf against World::hit's range end +inf: a hit at infinity with a NaN point and normal."""
    h = HittableList()
    h.add(_grid_mesh(Lambertian(C32(0.5, 0.5, 0.3)), lambda i, j: -1.0 if (i % 2 == 1 and j % 2 == 1) else -2.0))
    h.add(Sphere((0.0, 0.5, 0.0), 0.5, Metal(C32(0.8, 0.8, 0.7))))
    return _world(h)


SCENES = {"spheres": spheres, "spheres_moving": lambda: spheres(True), "flat": flat, "nest0": nest0, "nest2": nest2,
          "rich": rich}


# ------------------------------------------------------------------------------- rays ----
def d_axis() -> np.ndarray:
    """{-1, -0.0, +0.0, 1}^3 without the eight triples of zero magnitude: 56 directions."""
    d = np.array(list(itertools.product((-1.0, -0.0, 0.0, 1.0), repeat=3)))
    return d[np.any(d != 0.0, axis=1)]


def d_scaled() -> np.ndarray:
    """D_axis x {2^-20, 3, 2^20}: non-unit directions, a != 1 in the sphere and quadric roots (168)."""
    return np.concatenate([d_axis() * s for s in (2.0 ** -20, 3.0, 2.0 ** 20)])


def d_near() -> np.ndarray:
    """D_axis's directions with a zero component, every zero replaced by 2^-k with the zero's sign, k = 30, 60,
    200 (|1/d| > 1e30), 1030 and 1074 (subnormal: 1/d is infinite): 48 x 5 = 240."""
    d = d_axis()
    d = d[np.any(d == 0.0, axis=1)]
    out = []
    for k in (30, 60, 200, 1030, 1074):
        out.append(np.where(d == 0.0, np.copysign(math.ldexp(1.0, -k), d), d))
    return np.concatenate(out)


def _origins() -> np.ndarray:
    g = np.arange(-3.0, 3.25, 0.5)
    return np.array(list(itertools.product(g, g, g)))


def _subsample(n_dirs: int, count: int, step: int, offset: int):
    """count (origin, direction) pairs out of all of them, every step-th one from offset (step is prime and larger
    than every total's factors here, so the walk visits `count` different pairs)."""
    total = 13 ** 3 * n_dirs
    assert math.gcd(step, total) == 1 and count <= total
    p = (offset + step * np.arange(count, dtype=np.int64)) % total
    return p // n_dirs, p % n_dirs


@functools.lru_cache(maxsize=None)
def rays(name: str):
    """The scene's rays: (rays (n, 7) = o d time, family (n,) index into FAMILIES, twins (m, 2)).

    twins: pairs of row indices whose rays differ only in the sign of their zero direction components (every
    axis / scaled ray with a zero component is followed by its twin). The set is the same for every scene; only
    `spheres_moving` has times other than 0 (MOVING_TIMES, cycling; a twin keeps its ray's time)."""
    org = _origins()
    rows, fam, twins = [], [], []
    times = MOVING_TIMES if name == "spheres_moving" else (0.0,)
    k = 0
    for f, (dirs, count, step, off) in enumerate(((d_axis(), 1000, 7919, 11), (d_scaled(), 600, 104729, 5),
                                                  (d_near(), 1200, 15485863, 3))):
        oi, di = _subsample(len(dirs), count, step, off)
        for a, b in zip(oi, di):
            t = times[k % len(times)]
            k += 1
            d = dirs[b]
            rows.append(np.concatenate([org[a], d, [t]]))
            fam.append(f)
            if f < 2 and np.any(d == 0.0):
                rows.append(np.concatenate([org[a], np.where(d == 0.0, -d, d), [t]]))
                fam.append(f)
                twins.append((len(rows) - 2, len(rows) - 1))
    r = np.ascontiguousarray(np.array(rows))
    d = r[:, 3:6]
    assert np.isfinite(r).all() and np.all(np.any(d != 0.0, axis=1))
    r.setflags(write=False)
    return r, np.array(fam), np.array(twins)


# ------------------------------------------------------------------------------- non-finite rays ----
NONFINITE_KINDS = ("nan_dir", "nan_origin", "inf_dir", "nan_component")


@functools.lru_cache(maxsize=None)
def nonfinite_rays(name: str):
    """Rays the path feeds itself after a degenerate level (a NaN refraction, unit(0) of a light sample, the NaN
    point of a hit at infinity), kept apart from rays(): (rays (n, 7), kind (n,) index into NONFINITE_KINDS).

    nan_dir: every direction component NaN, the origin on the lattice. nan_origin: a NaN direction from an origin
    with one or with all components NaN (or infinite, as ray_at(inf) leaves them). inf_dir: one to three
    components +-inf, the others from D_axis. nan_component: one NaN component in a D_axis direction, the lattice
    origin -- not something shading produces, but the case in which the boxes' tests and the objects' disagree most:
    a box test ignores the NaN axis, a rect's bounds test lets the NaN coordinate pass."""
    nan = float("nan")
    org = _origins()[5::37]                                  # 60 lattice origins
    dirs = d_axis()
    times = MOVING_TIMES if name == "spheres_moving" else (0.0,)
    rows, kind = [], []

    def add(o, d, k):
        rows.append(np.concatenate([o, d, [times[len(rows) % len(times)]]]))
        kind.append(k)

    for o in org:
        add(o, (nan, nan, nan), 0)
    for i, o in enumerate(org):
        bad = np.array(o)
        bad[i % 3] = (nan, INF, -INF)[(i // 3) % 3]
        add(bad, (nan, nan, nan), 1)
        add((nan, nan, nan), (nan, nan, nan), 1)
        add(bad, dirs[i % len(dirs)], 1)
    for i, o in enumerate(org):
        for j in range(3):
            d = np.array(dirs[(7 * i + j) % len(dirs)])
            d[j] = INF if (i + j) % 2 else -INF
            add(o, d, 2)
        add(o, ((INF, -INF)[i % 2], INF, -INF), 2)
    for i, o in enumerate(_origins()[3::11]):                # 200 lattice origins
        d = np.array(dirs[(5 * i) % len(dirs)])
        d[i % 3] = nan
        add(o, d, 3)
    r = np.ascontiguousarray(np.array(rows))
    assert not np.isfinite(r).all(axis=1).any()
    r.setflags(write=False)
    return r, np.array(kind)


@functools.lru_cache(maxsize=None)
def nonfinite_reference(name: str, tmin: float) -> np.ndarray:
    rec = oracle_records(oracle(name), nonfinite_rays(name)[0], tmin)
    rec.setflags(write=False)
    return rec


# ------------------------------------------------------------------------------- oracle ----
@functools.lru_cache(maxsize=None)
def _fast_hit():
    """orc_world_hit through a CDLL handle of its own, taking addresses: a call per ray without building ctypes
    arrays (the tie bookkeeping makes ~10^6 calls)."""
    from oracle import binding
    binding.load()
    f = C.CDLL(binding.LIB_PATH).orc_world_hit
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]
    f.restype = C.c_int
    return f


def oracle_records(orc, r: np.ndarray, tmin: float, rows=None) -> np.ndarray:
    """orc.world_hit(o, d, time, tmin, +inf) for the rays `rows` (default: all) as (n, 13) doubles; the rows not
    asked for stay zero."""
    f = _fast_hit()
    out = np.zeros((len(r), 13))
    rb, ob, h = r.ctypes.data, out.ctypes.data, orc.h
    tm = r[:, 6].tolist()
    for i in (range(len(r)) if rows is None else rows):
        rc = f(h, rb + 56 * i, rb + 56 * i + 24, tm[i], tmin, INF, ob + 104 * i)
        assert rc == 0
    return out


def bits(a: np.ndarray) -> np.ndarray:
    """The doubles' bit patterns: keeps the sign of zero and NaN payloads apart, unlike == on floats."""
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def world(name: str) -> World:
    return slanted() if name == "slanted" else SCENES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    from oracle.binding import OracleScene
    return OracleScene(world(name))


@functools.lru_cache(maxsize=None)
def reference(name: str, tmin: float) -> np.ndarray:
    """The oracle's records of the scene's rays at tmin: computed once, shared, read-only."""
    rec = oracle_records(oracle(name), rays(name)[0], tmin)
    rec.setflags(write=False)
    return rec


# ------------------------------------------------------------------------------- ties ----
def leaf_objects(w: World):
    """The world's objects one by one, a mesh as its triangles: [(single object, material id in `w`)]. Material
    ids follow realize(): numbered by first use over hittables, then lights (leaf objects only here)."""
    ids, out = {}, []
    for o in w.hittables.objects:
        m = o.material
        if id(m) not in ids:
            ids[id(m)] = len(ids)
        if isinstance(o, TriangleMesh):
            for k in range(o.positions.shape[0]):
                nrm = None if o.normals is None else o.normals[k:k + 1]
                out.append((TriangleMesh(o.positions[k:k + 1], nrm, m), ids[id(m)]))
        else:
            assert isinstance(o, (Sphere, AARect)), "near-first scenes hold leaf objects only"
            out.append((o, ids[id(m)]))
    return out


def ties(name: str, tmin: float, r=None, ref=None):
    """For a near-first scene: (tied (n_obj, n) bool, recs (n_obj, n, 13)); a fraction of a second and some tens
    of megabytes, so not kept between tests. Object k alone in an oracle world
    gives recs[k] (material id mapped to the full world's); tied[k, i] says its t1 on ray i equals the world
    record's t1 -- bitwise, but for t1 = 0, where +0 and -0 tie: no comparison a traversal makes tells them apart,
    and two spheres touching at the ray's origin (tmin = 0, a tangent ray) give one each. Only rays the world hits
    are evaluated. r, ref: another ray table of the scene and its oracle records (default: rays(), reference())."""
    from oracle.binding import OracleScene
    if r is None:
        r, ref = rays(name)[0], reference(name, tmin)
    w = world(name)
    hit_rows = np.flatnonzero(ref[:, 0] == 1.0).tolist()
    objs = leaf_objects(w)
    recs = np.zeros((len(objs), len(r), 13))
    for k, (o, mat) in enumerate(objs):
        single = World(HittableList().add(o), HittableList(), w.background, w.time_range)
        rk = oracle_records(OracleScene(single), r, tmin, hit_rows)
        rk[rk[:, 0] == 1.0, 12] = float(mat)
        recs[k] = rk
    same_t1 = (bits(recs[:, :, 1]) == bits(ref[:, 1])[None, :]) | ((recs[:, :, 1] == 0.0) & (ref[:, 1] == 0.0)[None, :])
    tied = (recs[:, :, 0] == 1.0) & same_t1 & (ref[:, 0] == 1.0)[None, :]
    return tied, recs


def matches_a_tied_object(rec: np.ndarray, tied: np.ndarray, recs: np.ndarray) -> np.ndarray:
    """(n,) bool: the record (hit, t1 .. mat) equals, in fields 1-12 bitwise, the record of one tied object."""
    same = np.all(bits(recs[:, :, 1:13]) == bits(rec[:, 1:13])[None, :, :], axis=2)
    return np.any(same & tied, axis=0)


def coplanar_rects(name: str):
    """Indices (into leaf_objects) of `flat`'s two coplanar overlapping xz rects."""
    assert name == "flat"
    objs = leaf_objects(world(name))
    idx = [k for k, (o, _) in enumerate(objs) if isinstance(o, AARect) and o.metrics.k == -1.0]
    assert len(idx) == 2
    return idx


# ------------------------------------------------------------------------------- frames ----
FRAME_SCENES = ("spheres", "spheres_moving", "flat", "nest0", "nest2")
# per scene: look_from exactly on a bounding-box plane shared by two objects' boxes, at a sphere's centre, and on a
# sphere's surface point; look_at keeps the view off the axes
FRAME_EYES = {
    "spheres": {"plane": (-0.5, 0.0, 3.0), "centre": (0.0, 0.5, 0.0), "surface": (2.5, 0.5, 2.0)},
    "spheres_moving": {"plane": (-0.5, 0.0, 3.0), "centre": (0.0, 0.5, 0.0), "surface": (2.5, 0.5, 2.0)},
    "flat": {"plane": (0.5, 0.0, 3.0), "centre": (0.0, 0.5, 0.0), "surface": (2.0, 1.0, 2.0)},
    "nest0": {"plane": (-1.0, -0.5, 3.0), "centre": (1.3, 0.7, -1.1), "surface": (1.3, 1.15, -1.1)},
    "nest2": {"plane": (-1.0, 0.0, 3.0), "centre": (-2.0, 2.0, 2.0), "surface": (-2.0, 2.5, 2.0)},
}
FRAME_LOOK_AT = (0.25, -0.75, -0.5)


def frame_camera(name: str, where: str):
    b = CameraBuilder().look_from(FRAME_EYES[name][where]).look_at(FRAME_LOOK_AT).fov(70.0).aperture(0.0) \
        .width(32).height(20)
    if name == "spheres_moving":
        b = b.shutter_speed(1.0)
    return b.build()
