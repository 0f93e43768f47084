"""World::hit far from the coordinate origin and at other scales: tests/edge_rays.py's six worlds and ray families
under x -> s * x + T, and named rays for the three ways the f32 cull of the tree walks used to lose boxes
(raysnail_amd/csrc/rs_cull.h, profiles/cull/README.md).

Translated worlds add T to every coordinate: lattice coordinates stay exact in f64 up to 2^51, so the rays are the
same lattice rays translated, and in the two sphere worlds every o - c is exact, so the oracle's hit flag and t1 are
the untranslated ray's bit for bit. At 2^24 an f32 ulp is 2, wider than a sphere; 2^28 and 2^29 lie on either side
of the magnitude from which an axis-parallel ray's |o| / |d| products left f32.

Scaled worlds multiply every coordinate by 2^k: f32 goes subnormal or to 0 at the bottom and to infinity at the top.
Ray origins are scaled; directions are scaled as well (t unchanged) or not (t scales; tmin = 0). Powers of two
commute with every operation until something under- or overflows: keeps_flags() says which combinations keep the
unscaled world's hit flags on the oracle, and tests/test_far_worlds_cpu.py asserts it.

A plain helper module, like edge_rays.py: tests/test_far_worlds_cpu.py guards these fixtures on the CPU,
tests/test_gpu_far_worlds.py compares the GPU's records with the oracle's on them.
"""
from __future__ import annotations

import functools

import numpy as np

import edge_rays as E
from raysnail_amd import _abi as A
from raysnail_amd.api import (AARect, AARectMetrics, Box, CameraBuilder, ConstantMedium, Difference, HittableList,
                              Intersection, Lambertian, Quadric, Sphere, TfFacade, Transform, TransformStack,
                              TriangleMesh, World)
from raysnail_amd.scenes import C32

NAMES = ("spheres", "spheres_moving", "flat", "nest0", "nest2", "rich")
ROW_STEP = 3   # every third ray of edge_rays.rays(): about 1 500 rays per world, every family and many twins

# ------------------------------------------------------------------------------- the variants ----
# name -> (s, T): x -> s * x + T
TRANSLATED = {f"t{e}": (1.0, (2.0 ** e,) * 3) for e in (20, 24, 28, 29, 31, 40)}
TRANSLATED["t31x"] = (1.0, (2.0 ** 31, 0.0, 0.0))
SCALE_EXPONENTS = (-130, -100, -60, 60, 100, 126, 130)
SCALED = {f"s{k}": (2.0 ** k, (0.0, 0.0, 0.0)) for k in SCALE_EXPONENTS}
VARIANTS = {**TRANSLATED, **SCALED}
DIR_MODES = ("dirs_scaled", "dirs_kept")   # scaled worlds only; dirs_kept is probed with tmin = 0 alone

FLAG_FAMILIES = (0, 1)   # E.FAMILIES "axis" and "scaled": the rays whose hit flags a power-of-two map can keep


def keeps_flags(name: str, variant: str, dir_mode: str = "dirs_scaled") -> bool:
    """Whether the oracle's hit flags of the `axis` and `scaled` rays are the untransformed world's
    (tests/test_far_worlds_cpu.py asserts both halves; the GPU plays no part in it). The `near` family is left out:
    its 2^-1030 and 2^-1074 direction components under- or overflow under any scale. What does not keep them:
      * a scale 2^k, k > 0, or T = 2^40, in every world with rects, boxes or triangles: the 1e-4 the reference pads a
        flat box with vanishes beside the coordinates, the box has zero thickness and the exact test never accepts it;
      * a translation of nest0: its bare quadrics' constant terms hold T^2 and cancel;
      * unscaled directions in `rich` scaled down: a medium's free path is drawn per unit of |d| * t.
    Every combination still has oracle hits in every family."""
    if name in ("spheres", "spheres_moving"):
        return True
    if variant in TRANSLATED:
        return name != "nest0" and variant != "t40"
    if VARIANTS[variant][0] > 1.0:
        return False
    return not (name == "rich" and dir_mode == "dirs_kept")


# Combinations in which the oracle hits nothing at all would have nothing to compare on the GPU: there are none
# (test_far_worlds_cpu.py asserts hits in every family of every combination).
ORACLE_HITS_NOTHING: set = set()


def _map_point(p, s, T):
    return tuple(s * float(p[k]) + T[k] for k in range(3))


def _map_object(o, s, T, memo):
    """The object under x -> s * x + T (s a power of two): every coordinate mapped, materials shared."""
    if id(o) in memo:
        return memo[id(o)]
    if isinstance(o, Sphere):
        n = Sphere(_map_point(o.center, s, T), s * o.radius, o.material)
        if o.speed != (0.0, 0.0, 0.0):
            n.with_speed(tuple(s * v for v in o.speed))
    elif isinstance(o, AARect):
        a, b, k = {A.RS_PLANE_XY: (0, 1, 2), A.RS_PLANE_XZ: (0, 2, 1), A.RS_PLANE_YZ: (1, 2, 0)}[o.plane]
        m = o.metrics
        n = AARect(o.plane, AARectMetrics(s * m.k + T[k], (s * m.a[0] + T[a], s * m.a[1] + T[a]),
                                          (s * m.b[0] + T[b], s * m.b[1] + T[b])), o.material)
    elif isinstance(o, Box):
        n = Box(_map_point(o.p0, s, T), _map_point(o.p1, s, T), o.material)
    elif isinstance(o, TriangleMesh):
        assert o.normals is None
        n = TriangleMesh(o.positions.reshape(-1, 3) * s + np.array(T), None, o.material)
    elif isinstance(o, Quadric):
        # sum a_k x_k^2 + b_k x_k + c = 0 at x = (x' - T) / s, times s^2 (a power of two: nothing rounds for T = 0)
        qa, qb, qc, qd, qe, qf, qg, qh, qi, qj = o.q
        assert qb == 0.0 and qc == 0.0 and qf == 0.0
        a2, b1 = (qa, qe, qh), (qd, qg, qi)
        lin = [s * b1[k] - 2.0 * a2[k] * T[k] for k in range(3)]
        c = s * s * qj + sum(a2[k] * T[k] * T[k] - s * b1[k] * T[k] for k in range(3))
        n = Quadric(qa, 0.0, 0.0, lin[0], qe, 0.0, lin[1], qh, lin[2], c, o.material)
    elif isinstance(o, TfFacade):
        st = TransformStack()
        for t in o.stack.stack:
            st.push(t)
        if s != 1.0:
            st.push(Transform.scale((s, s, s)))
        if any(T):
            st.push(Transform.translate(T))
        n = TfFacade(o.obj, st)
    elif isinstance(o, ConstantMedium):
        n = ConstantMedium(_map_object(o.boundary, s, T, memo), o.color, o.density / s)   # the same optical depth
    elif isinstance(o, Intersection):
        n = Intersection(_map_object(o.o1, s, T, memo), _map_object(o.o2, s, T, memo), o.material)
    elif isinstance(o, Difference):
        n = Difference(_map_object(o.plus, s, T, memo), _map_object(o.minus, s, T, memo), o.material)
    else:
        raise TypeError(type(o))
    memo[id(o)] = n
    return n


def map_world(w: World, s: float, T) -> World:
    memo = {}
    h, lights = HittableList(), HittableList()
    for o in w.hittables.objects:
        h.add(_map_object(o, s, T, memo))
    for o in w.lights.objects:
        lights.add(_map_object(o, s, T, memo))
    return World(h, lights, w.background, w.time_range)


@functools.lru_cache(maxsize=None)
def world(name: str, variant: str) -> World:
    s, T = VARIANTS[variant]
    return map_world(E.world(name), s, T)


@functools.lru_cache(maxsize=None)
def oracle(name: str, variant: str):
    from oracle.binding import OracleScene
    return OracleScene(world(name, variant))


@functools.lru_cache(maxsize=None)
def base_rows(name: str) -> np.ndarray:
    return np.arange(0, len(E.rays(name)[0]), ROW_STEP)


@functools.lru_cache(maxsize=None)
def rays(name: str, variant: str, dir_mode: str = "dirs_scaled"):
    """(rays (n, 7), family (n,)): rows base_rows(name) of edge_rays.rays(name), origins under x -> s * x + T,
    directions times s (dirs_scaled) or as they are (dirs_kept)."""
    s, T = VARIANTS[variant]
    r0, fam, _ = E.rays(name)
    rows = base_rows(name)
    r = np.array(r0[rows])
    r[:, :3] = r[:, :3] * s + np.array(T)
    if dir_mode == "dirs_scaled":
        r[:, 3:6] *= s
    else:
        assert dir_mode == "dirs_kept"
    r = np.ascontiguousarray(r)
    r.setflags(write=False)
    return r, fam[rows]


def tmins(variant: str, dir_mode: str):
    return (0.0,) if dir_mode == "dirs_kept" else E.TMINS


@functools.lru_cache(maxsize=None)
def reference(name: str, variant: str, dir_mode: str, tmin: float) -> np.ndarray:
    rec = E.oracle_records(oracle(name, variant), rays(name, variant, dir_mode)[0], tmin)
    rec.setflags(write=False)
    return rec


def base_reference(name: str, tmin: float) -> np.ndarray:
    """The untransformed world's oracle records of the same rays."""
    return E.reference(name, tmin)[base_rows(name)]


def tied_objects(w: World, r: np.ndarray, ref: np.ndarray, tmin: float, rows):
    """edge_rays.ties() for the rays `rows` of another world: (tied (n_obj, len(rows)), recs (n_obj, len(rows), 13))."""
    from oracle.binding import OracleScene
    rows = [int(i) for i in rows]
    sub = np.ascontiguousarray(r[rows])
    objs = E.leaf_objects(w)
    recs = np.zeros((len(objs), len(rows), 13))
    for k, (o, mat) in enumerate(objs):
        single = World(HittableList().add(o), HittableList(), w.background, w.time_range)
        rk = E.oracle_records(OracleScene(single), sub, tmin)
        rk[rk[:, 0] == 1.0, 12] = float(mat)
        recs[k] = rk
    t1 = ref[rows, 1]
    same_t1 = (E.bits(recs[:, :, 1]) == E.bits(t1)[None, :]) | ((recs[:, :, 1] == 0.0) & (t1 == 0.0)[None, :])
    tied = (recs[:, :, 0] == 1.0) & same_t1 & (ref[rows, 0] == 1.0)[None, :]
    return tied, recs


# ------------------------------------------------------------------------------- named rays ----
# The three classes of boxes the cull lost, as worlds of two objects (a single object has no tree) and the lamp:
# kind "rects" (flat mode: the 4-wide near-first walk, slab4), "spheres" (spheres mode, slab4), "boxes" (a Box makes
# the scene reference-order: walk4_inorder / the binary walk, slab32). name -> (kind, objects, ray (o, d)).
def _lam(i=0):
    return Lambertian(C32(0.7 - 0.2 * i, 0.3 + 0.2 * i, 0.2))


def _named():
    out = {}
    for e in (28, 29, 30, 31):
        T = 2.0 ** e
        ray = ((T, 0.0, 0.0), (0.0, 0.0, 1.0))
        # A: |o_x| * |1 / d_x| leaves f32 (an axis-parallel ray far from the coordinate origin); 2^28 is below it
        out[f"A{e}_rects"] = ("rects", [AARect.new_xy(AARectMetrics(5.0, (T - 1.0, T + 1.0), (-1.0, 1.0)), _lam()),
                                        AARect.new_xy(AARectMetrics(9.0, (T - 1.0, T + 1.0), (-1.0, 1.0)), _lam(1))], ray)
        out[f"A{e}_spheres"] = ("spheres", [Sphere((T, 0.0, 5.0), 1.0, _lam()), Sphere((T, 0.0, 9.0), 1.0, _lam(1))], ray)
        out[f"A{e}_boxes"] = ("boxes", [Box((T - 1.0, -1.0, 4.0), (T + 1.0, 1.0, 6.0), _lam()),
                                        Box((T - 1.0, -1.0, 8.0), (T + 1.0, 1.0, 10.0), _lam(1))], ray)
    B, w, back = 2.0 ** 130, 2.0 ** 90, 2.0 ** 100
    for sign, tag in ((1.0, "p"), (-1.0, "m")):
        # B: the origin itself is beyond the largest float
        ray = ((sign * B - back, 0.0, 0.0), (1.0, 0.0, 0.0))
        # (no B for rects: a rect's box there is its plane +- 1e-4, which 2^130 absorbs -- zero thickness, and the
        # exact test, hence the oracle, never accepts it)
        out[f"B{tag}_spheres"] = ("spheres", [Sphere((sign * B, 0.0, 0.0), w, _lam()),
                                              Sphere((sign * B + 4.0 * w, 0.0, 0.0), w, _lam(1))], ray)
        out[f"B{tag}_boxes"] = ("boxes", [Box((sign * B - w, -B, -B), (sign * B + w, B, B), _lam()),
                                          Box((sign * B + 3.0 * w, -B, -B), (sign * B + 5.0 * w, B, B), _lam(1))], ray)
    # C: 1e30 < |1 / d_z| <= 3e38, the band in which the clamped inv shrank the far plane's t
    ray = ((0.0, 0.0, 0.0), (1.0, 0.0, 1e-33))
    out["C_rects"] = ("rects", [AARect.new_yz(AARectMetrics(5.0, (-1.0, 1.0), (-1.0, 1e-32)), _lam()),
                                AARect.new_yz(AARectMetrics(9.0, (-1.0, 1.0), (-1.0, 1e-32)), _lam(1))], ray)
    out["C_boxes"] = ("boxes", [Box((4.0, -1.0, -1.0), (6.0, 1.0, 1e-32), _lam()),
                                Box((8.0, -1.0, -1.0), (10.0, 1.0, 1e-32), _lam(1))], ray)
    # (no C for spheres: a sphere's box is symmetric about a centre the ray passes within 1e-32 of, which f64 cannot
    # tell from a ray through the centre at these coordinates -- that ray's box is hit by a wide margin)
    return out


NAMED = _named()
NAMED_INFO = {"rects": (2, 0), "spheres": (1, 0), "boxes": (3, 1)}   # kind -> (scene_mode, ref_order)
NAMED_TMIN = 1e-4


@functools.lru_cache(maxsize=None)
def named_world(case: str) -> World:
    h = HittableList()
    for o in NAMED[case][1]:
        h.add(o)
    return E._world(h)


def named_ray(case: str) -> np.ndarray:
    o, d = NAMED[case][2]
    return np.ascontiguousarray(np.array([list(o) + list(d) + [0.0]]))


# ------------------------------------------------------------------------------- frames ----
FRAME_VARIANT = "t29"
FRAME_NAMES = E.FRAME_SCENES   # one per walk: spheres (and moving), flat, nest0, nest2


def frame_camera(name: str):
    """8 x 6, looking along -z from 3.5 in front of the translated world: the central direction is exactly axis-parallel
    and every bounce ray starts 2^29 from the coordinate origin."""
    T = VARIANTS[FRAME_VARIANT][1]
    b = CameraBuilder().look_from((T[0] + 0.25, T[1] + 0.25, T[2] + 3.5)).look_at((T[0] + 0.25, T[1] + 0.25, T[2])) \
        .fov(70.0).aperture(0.0).width(8).height(6)
    if name == "spheres_moving":
        b = b.shutter_speed(1.0)
    return b.build()
