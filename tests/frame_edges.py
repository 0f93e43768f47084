"""Cameras, frame shapes and poisoned worlds for both ends of a path and the frame around it, where ordinary
arithmetic ends: the camera sample (make_camera, camera_sample_xy, camera_ray) under degenerate lenses, focus
distances, fields of view, bases, scales and shutters; the sample order (gen_perm) and the accumulation under frame
shapes no ordinary render has; close_path, the miss branch and into_color under non-finite factors.

The worlds of the camera tables are edge_rays.py's six (one per scene mode, two for the spheres mode). Every number
here is written for this repository: integers, halves and powers of two wherever a value is meant to be exact.

A plain helper module (like edge_rays.py and shade_edges.py): tests/test_frame_edges_cpu.py guards these fixtures on
the oracle, tests/test_gpu_frame_edges.py compares the GPU with the oracle on them.
"""
from __future__ import annotations

import functools
import itertools
import math

import numpy as np

import edge_rays as E
from raysnail_amd import _abi as A
from raysnail_amd.api import (AARect, AARectMetrics, Box, DiffuseLight, Gradient, HittableList, Intersection,
                              Lambertian, Metal, Sphere, World)
from raysnail_amd.scenes import C32

NAN, INF = float("nan"), float("inf")
SEED, PASS = 11, 2
WORLDS = ("spheres", "spheres_moving", "flat", "nest0", "nest2", "rich")   # edge_rays.SCENES
FIELDS = ("o.x", "o.y", "o.z", "d.x", "d.y", "d.z", "time", "rng.x", "rng.y", "rng.z", "rng.w")
SUBNORMAL = math.ldexp(1.0, -1074)

# The well-formed camera every entry departs from in one respect: a 7 x 5 frame, 4 samples, a lens and a shutter.
BASE = dict(look_from=(1.0, 1.5, 5.0), look_at=(0.25, -0.25, 0.0), vup=(0.0, 1.0, 0.0), fov=40.0, aperture=0.25,
            focus=4.0, shutter=0.5, width=7, height=5)
FAMILIES = ("lens", "focus", "fov", "basis", "scale", "shutter", "frame", "samples")
FAMILY_SIZES = {"lens": 8, "focus": 6, "fov": 8, "basis": 12, "scale": 5, "shutter": 6, "frame": 4, "samples": 5}
SCALE_POWERS = (-520, -540, 500, 520)


class Entry:
    """One camera of the table: rs_camera_desc fields written directly (no CameraBuilder), the requested samples and
    a one-line reason."""

    def __init__(self, family, name, reason, samples=4, **fields):
        f = dict(BASE)
        f.update(fields)
        self.family, self.name, self.reason, self.samples, self.fields = family, name, reason, samples, f

    def desc(self, width=None, height=None) -> A.rs_camera_desc:
        f = self.fields
        d = A.rs_camera_desc()
        d.look_from[:] = list(f["look_from"])
        d.look_at[:] = list(f["look_at"])
        d.vup[:] = list(f["vup"])
        d.fov, d.aperture, d.focus, d.shutter = f["fov"], f["aperture"], f["focus"], f["shutter"]
        d.width, d.height = width or f["width"], height or f["height"]
        return d

    def settings(self, samples=None, depth=4, mode=A.RS_MODE_AUTO, gamma=1) -> A.rs_render_settings:
        st = A.rs_render_settings()
        st.samples, st.depth, st.gamma, st.mode = samples or self.samples, depth, gamma, mode
        st.seed, st.pass_ = SEED, PASS
        st.row_begin, st.row_end, st.row_step = 0, 0, 1
        return st


def _scaled(p: int) -> dict:
    """BASE's camera multiplied by 2^p: positions, focus and aperture (exact: powers of two)."""
    k = math.ldexp(1.0, p)
    return dict(look_from=tuple(c * k for c in BASE["look_from"]), look_at=tuple(c * k for c in BASE["look_at"]),
                focus=BASE["focus"] * k, aperture=BASE["aperture"] * k)


def _axis_view(axis: int, sign: float) -> dict:
    """A view from 5 units out on one axis towards the origin; the other two components of look_at - look_from are
    zeros of alternating sign (-0.0 - 0.0 = -0.0, 0.0 - 0.0 = +0.0)."""
    at, frm = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    frm[axis] = 5.0 * sign
    at[(axis + 1) % 3] = -0.0
    vup = (0.0, 1.0, 0.0) if axis != 1 else (0.0, 0.0, -1.0)
    return dict(look_from=tuple(frm), look_at=tuple(at), vup=vup)


def _view_w():
    """BASE's view direction (to rounding: the cross product with it is zero or rounding noise)."""
    d = [a - b for a, b in zip(BASE["look_at"], BASE["look_from"])]
    inv = 1.0 / math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return tuple(c * inv for c in d)


@functools.lru_cache(maxsize=None)
def cameras():
    e = []

    def add(family, name, reason, **kw):
        e.append(Entry(family, name, reason, **kw))

    # ---- lens ----
    add("lens", "ap_pos0", "a pinhole: aperture exactly +0, the lens offset is +0 times the basis", aperture=0.0)
    add("lens", "ap_neg0", "aperture -0: the offset's zeros change sign, the origin must not", aperture=-0.0)
    add("lens", "ap_subnormal", "aperture 2^-1074: aperture / 2 rounds to 0", aperture=SUBNORMAL)
    add("lens", "ap_negative", "aperture -0.5: the lens disk mirrored through its centre", aperture=-0.5)
    add("lens", "ap_wide", "aperture 2 at focus 4: a lens as wide as the scene's spacing", aperture=2.0, focus=4.0)
    add("lens", "ap_huge", "aperture 1e6: origins far outside the scene", aperture=1e6)
    add("lens", "ap_inf", "aperture +inf: inf * disk, a NaN where the disk component is 0", aperture=INF)
    add("lens", "ap_nan", "aperture NaN: every origin and direction NaN", aperture=NAN)
    # ---- focus ----
    add("focus", "focus0_pinhole", "focus +0, aperture 0: lb == origin, every direction is unit(0) = NaN", focus=0.0,
        aperture=0.0)
    add("focus", "focus0_lens", "focus 0, aperture 0.5: F == O, finite rays back through the origin", focus=0.0,
        aperture=0.5)
    add("focus", "focus_negative", "focus -4: the footprint behind the lens (look_at mirrored through look_from, so "
        "the rays still meet the scene), the image turned round", focus=-4.0, look_at=(1.75, 3.25, 10.0))
    add("focus", "focus_tiny", "focus 1e-300: a footprint of size 1e-300 absorbed by look_from", focus=1e-300)
    add("focus", "focus_huge", "focus 1e300: len2 of the direction overflows", focus=1e300)
    add("focus", "focus_inf", "focus inf: lb is inf - inf", focus=INF)
    # ---- field of view ----
    add("fov", "fov0", "fov 0: tan(0) = 0, an empty footprint, every pixel the same ray", fov=0.0)
    add("fov", "fov_tiny", "fov 1e-300: theta underflows towards a subnormal", fov=1e-300)
    add("fov", "fov90", "fov 90: tan(pi / 4) is not 1", fov=90.0)
    add("fov", "fov180", "fov 180: tan(pi / 2) = 1.6e16, finite", fov=180.0)
    add("fov", "fov270", "fov 270: tan negative, the image turned round", fov=270.0)
    add("fov", "fov360", "fov 360: tan(pi) = -1.2e-16", fov=360.0)
    add("fov", "fov_negative", "fov -40: a negative viewport", fov=-40.0)
    add("fov", "fov_nan", "fov NaN", fov=NAN)
    # ---- basis ----
    w = _view_w()
    add("basis", "from_eq_at", "look_from == look_at: w = unit(0), the whole basis NaN", look_at=BASE["look_from"])
    add("basis", "vup_plus_w", "vup = +w: w x vup = 0 (or rounding noise), hu = unit of that", vup=w)
    add("basis", "vup_minus_w", "vup = -w", vup=tuple(-c for c in w))
    add("basis", "vup_zero", "vup = 0: hu = unit(0) = NaN", vup=(0.0, 0.0, 0.0))
    add("basis", "vup_nan", "vup with one NaN component", vup=(0.0, NAN, 0.0))
    t = math.ldexp(1.0, -26)
    add("basis", "vup_near_w", "vup at an angle of 2^-26 to w: |w x vup|^2 = 2^-52, the cross product cancels",
        look_from=(0.0, 0.0, 5.0), look_at=(0.0, 0.0, 0.0), vup=(t, 0.0, -1.0))
    for axis, sign in itertools.product(range(3), (1.0, -1.0)):
        add("basis", f"axis_{'xyz'[axis]}{'+' if sign > 0 else '-'}",
            "a view along an axis: two components of w are signed zeros", **_axis_view(axis, sign))
    # ---- scale ----
    add("scale", "scale_m520", "everything times 2^-520: len2 is subnormal", **_scaled(-520))
    add("scale", "scale_m540", "everything times 2^-540: len2 underflows to 0, 1 / sqrt is inf", **_scaled(-540))
    add("scale", "scale_p500", "everything times 2^500: len2 near the top of the range", **_scaled(500))
    add("scale", "scale_p520", "everything times 2^520: len2 overflows, 1 / sqrt is 0", **_scaled(520))
    add("scale", "far_2p53", "look_from at (2^53, 0, 0): the lens offset is absorbed by the origin",
        look_from=(math.ldexp(1.0, 53), 0.0, 0.0), look_at=(math.ldexp(1.0, 53) - 8.0, 0.0, 0.0))
    # ---- shutter (against spheres_moving's time range (0, 1)) ----
    add("shutter", "shutter_pos0", "shutter +0: every time +0", shutter=0.0)
    add("shutter", "shutter_neg0", "shutter -0: every time -0", shutter=-0.0)
    add("shutter", "shutter_negative", "shutter -1: times before the range the boxes were built for", shutter=-1.0)
    add("shutter", "shutter_huge", "shutter 1e308: centres at 1e308", shutter=1e308)
    add("shutter", "shutter_inf", "shutter inf: time inf, a moving centre at inf, a static one at 0 * inf", shutter=INF)
    add("shutter", "shutter_nan", "shutter NaN", shutter=NAN)
    # ---- frame ----
    add("frame", "frame_1x1", "1 x 1: u in [0, 1], v = (1 - 1 - yo) / 1 below 0", width=1, height=1)
    add("frame", "frame_1x7", "1 x 7: one column", width=1, height=7)
    add("frame", "frame_7x1", "7 x 1: one row, v below 0 for every sample", width=7, height=1)
    add("frame", "frame_2x3", "2 x 3", width=2, height=3)
    # ---- samples ----
    for n in (1, 2, 3, 4, 8):
        add("samples", f"samples_{n}", f"{n} requested samples: floor(sqrt) = {int(math.isqrt(n))} strata a side",
            samples=n)
    assert len({c.name for c in e}) == len(e)
    return tuple(e)


def camera(name: str) -> Entry:
    return {c.name: c for c in cameras()}[name]


def family(fam: str):
    return tuple(c for c in cameras() if c.family == fam)


# ------------------------------------------------------------------------------- the camera probe ----
def probe_rows(entry: Entry) -> np.ndarray:
    """(n, 3) uint32: every pixel of the entry's frame (at most 7 x 5) times every sample."""
    f = entry.fields
    sq = math.isqrt(entry.samples)
    return np.array([(x, y, s) for y in range(f["height"]) for x in range(f["width"]) for s in range(sq * sq)],
                    dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def probe_reference(name: str, centres: bool) -> np.ndarray:
    """The oracle's 11 doubles per probe row: computed once per (camera, flag), shared, read-only."""
    from oracle import binding
    c = camera(name)
    out = binding.camera_sample(c.desc(), c.settings(), probe_rows(c), centres)
    out.setflags(write=False)
    return out


def differing(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """Elementwise: NaN against NaN is equal (by position, not payload or sign), everything else by its bits."""
    nan = np.isnan(ref)
    return (np.isnan(got) != nan) | ((E.bits(got) != E.bits(ref)) & ~nan)


def differing32(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """The same for float32 frames."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    nan = np.isnan(ref)
    return (np.isnan(got) != nan) | ((got.view(np.uint32) != ref.view(np.uint32)) & ~nan)


# ------------------------------------------------------------------------------- camera frames ----
# One camera per line of the issue's table, rendered at 8 x 6, 4 spp, depth 4 through every consumer of camera_ray.
FRAME_CAMERAS = ("ap_pos0", "ap_negative", "ap_wide", "ap_inf", "focus0_pinhole", "focus0_lens", "focus_negative",
                 "fov0", "fov180", "fov270", "from_eq_at", "vup_plus_w", "vup_zero", "axis_y-", "far_2p53",
                 "shutter_negative", "shutter_inf", "frame_7x1", "samples_8")
SCALED_FRAME_CAMERAS = ("scale_m520", "scale_m540", "scale_p500", "scale_p520")   # over scaled_spheres(p)
FRAME_W, FRAME_H = 8, 6
FRAME_WORLDS = ("spheres", "spheres_moving", "nest2")


def frame_desc(name: str) -> A.rs_camera_desc:
    """The table's camera on the 8 x 6 frame (the `frame` family keeps its own shape)."""
    c = camera(name)
    return c.desc() if c.family == "frame" else c.desc(FRAME_W, FRAME_H)


def frame_world_name(name: str, kind: str) -> str:
    """kind 'spheres' or 'nest2'; the shutter family's spheres world is the moving one."""
    return "spheres_moving" if kind == "spheres" and camera(name).family == "shutter" else kind


@functools.lru_cache(maxsize=None)
def scaled_spheres(p: int) -> World:
    """edge_rays.spheres() multiplied by 2^p, its lamp included."""
    k = math.ldexp(1.0, p)
    base = E.spheres()
    h, lights = HittableList(), HittableList()
    lamp = base.lights.objects[0]
    for o in base.hittables.objects:
        s = Sphere(tuple(c * k for c in o.center), o.radius * k, o.material)
        h.add(s)
        if o is lamp:
            lights.add(s)
    return World(h, lights, base.background, (0.0, 0.0))


@functools.lru_cache(maxsize=None)
def frame_world(wname: str) -> World:
    if wname.startswith("scaled"):
        return scaled_spheres(int(wname[6:]))
    if wname in POISON_NAMES:
        return poison_worlds()[wname]
    return E.world(wname)


@functools.lru_cache(maxsize=None)
def frame_oracle(wname: str):
    from oracle.binding import OracleScene
    return OracleScene(frame_world(wname))


def _freeze(img, stats):
    img.setflags(write=False)
    return img, (int(stats.segments), int(stats.samples))


@functools.lru_cache(maxsize=None)
def camera_frame_reference(name: str, wname: str):
    """(frame, (segments, samples)) of the oracle for the camera on the 8 x 6 frame, 4 spp (the entry's own count
    in the samples family), depth 4, gamma on: once per (camera, world); the mode does not enter."""
    c = camera(name)
    return _freeze(*frame_oracle(wname).render(frame_desc(name), c.settings(), threads=8))


@functools.lru_cache(maxsize=None)
def _recorded_oracle(wname: str):
    import spec_features_ref as R
    return R.oracle_scene(frame_world(wname))


@functools.lru_cache(maxsize=None)
def features_reference(name: str, wname: str, max_specular: int):
    """(albedo frame, normal frame, World::hit calls) of the camera's 8 x 6 feature frames: features_ref's
    restatement (max_specular 0) or spec_features_ref's chains, from oracle calls alone; once per key."""
    import features_ref as F
    import spec_features_ref as R
    orc, rec = _recorded_oracle(wname)
    d, st = frame_desc(name), camera(name).settings()
    if max_specular == 0:
        a, n, _ = F.expected(d, st, F.oracle_hits(orc), F.Albedo(rec))
        calls = d.width * d.height * math.isqrt(st.samples) ** 2
    else:
        ch = R.chains(d, st, F.oracle_hits(orc), F.Albedo(rec), max_specular)
        a, n = ch.frames()
        calls = int(ch.calls.sum())
    a.setflags(write=False)
    n.setflags(write=False)
    return a, n, calls


@functools.lru_cache(maxsize=None)
def sample_reference(name: str, wname: str) -> np.ndarray:
    """(H, W, N, 4): the oracle's radiance and World::hit count of every sample of the camera's 8 x 6 frame at
    depth 4 (orc_sample_radiance)."""
    d, st = frame_desc(name), camera(name).settings()
    orc = frame_oracle(wname)
    n = math.isqrt(st.samples) ** 2
    out = np.zeros((d.height, d.width, n, 4))
    for y, x, s in itertools.product(range(d.height), range(d.width), range(n)):
        rad, seg = orc.sample_radiance(d, st, x, y, s)
        out[y, x, s, :3] = rad
        out[y, x, s, 3] = seg
    out.setflags(write=False)
    return out


def sample_mismatches(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """rs_probe_samples against orc_sample_radiance, (..., 4) each: True where a sample misses the probe's documented
    criterion -- equal World::hit counts; non-finite channels of the same class (NaN, +inf, -inf) in the same
    positions; finite channels within 2^-40 max(|oracle|, 1) (the forward form nests the factors the other way)."""
    g, o = got[..., :3], ref[..., :3]
    fin = np.isfinite(o)
    bad = (got[..., 3] != ref[..., 3])[..., None] | (np.isfinite(g) != fin)
    with np.errstate(invalid="ignore"):
        bad |= ~fin & ~((np.isnan(o) & np.isnan(g)) | (o == g))
        bad |= fin & np.isfinite(g) & ~(np.abs(g - o) <= 2.0 ** -40 * np.maximum(np.abs(o), 1.0))
    return bad.any(axis=-1)


# ------------------------------------------------------------------------------- frame shapes ----
class Shape:
    """One frame of the shape table: W x H, samples, the row lattice (begin, end, step), a mask kind and the batch
    size in items handed to set_workspace (0: the default; `planes`: that many sample planes of the lattice)."""

    def __init__(self, name, w, h, samples, rows=(0, 0, 1), mask="none", planes=0, items=0):
        self.name, self.w, self.h, self.samples, self.rows, self.mask_kind = name, w, h, samples, rows, mask
        self.planes, self.items = planes, items

    def lattice_rows(self):
        b, e, s = self.rows
        e = min(e, self.h) if e else self.h
        return list(range(b, e, s))

    def batch_items(self) -> int:
        return self.items or self.planes * len(self.lattice_rows()) * self.w

    def mask(self):
        if self.mask_kind == "none":
            return None
        m = np.zeros((self.h, self.w), np.uint8)
        if self.mask_kind == "last":
            m[self.h - 1, self.w - 1] = 1
        return m

    def desc(self) -> A.rs_camera_desc:
        return camera("ap_wide").desc(self.w, self.h)

    def settings(self, mode=A.RS_MODE_AUTO) -> A.rs_render_settings:
        st = camera("ap_wide").settings(samples=self.samples, depth=3, mode=mode)
        st.row_begin, st.row_end, st.row_step = self.rows
        return st


SHAPES = (
    Shape("1x1_s1", 1, 1, 1),
    Shape("1x1_s121_one_plane", 1, 1, 121, planes=1),
    Shape("1x9_s4", 1, 9, 4),
    Shape("1x9_s9_step2", 1, 9, 9, rows=(1, 0, 2)),
    Shape("9x1_s4", 9, 1, 4),
    Shape("9x1_s36_three_planes", 9, 1, 36, planes=3),
    Shape("7x5_s36", 7, 5, 36),
    Shape("7x5_s100_three_planes", 7, 5, 100, planes=3),
    Shape("7x5_s121_prime", 7, 5, 121, items=211),
    Shape("7x5_s100_step3", 7, 5, 100, rows=(2, 0, 3)),
    Shape("7x5_s9_step_above_height", 7, 5, 9, rows=(1, 0, 9)),
    Shape("7x5_s36_mask_last", 7, 5, 36, mask="last"),
    Shape("13x3_s9_step2", 13, 3, 9, rows=(1, 0, 2)),
    Shape("13x3_s4_one_row", 13, 3, 4, rows=(2, 3, 1)),
    Shape("13x3_s9_mask_zero", 13, 3, 9, mask="zero"),
    Shape("17x11_s9", 17, 11, 9),
    Shape("17x11_s4_step4", 17, 11, 4, rows=(0, 0, 4)),
    Shape("17x11_s9_step7", 17, 11, 9, rows=(3, 0, 7)),
    Shape("17x11_s4_step8", 17, 11, 4, rows=(1, 0, 8)),
    Shape("17x11_s9_end_off_lattice", 17, 11, 9, rows=(1, 8, 3)),
    Shape("17x11_s9_one_plane", 17, 11, 9, planes=1),
    Shape("17x11_s9_prime", 17, 11, 9, items=1009),
    Shape("17x11_s4_mask_last_step2", 17, 11, 4, rows=(0, 0, 2), mask="last"),
)
SHAPE_WORLDS = ("spheres", "flat")


def shape(name: str) -> Shape:
    return {s.name: s for s in SHAPES}[name]


@functools.lru_cache(maxsize=None)
def shape_reference(name: str, wname: str):
    """(frame, (segments, samples)) of the oracle for the shape: once per (shape, world). Rows off the lattice and
    masked pixels are zero, as the library leaves a zeroed frame."""
    s = shape(name)
    out = np.zeros((s.h, s.w, 4), np.float32)
    return _freeze(*frame_oracle(wname).render(s.desc(), s.settings(), threads=8, mask=s.mask(), out=out))


# ------------------------------------------------------------------------------- poisoned worlds ----
POISON_DEPTHS = (0, 1, 2, 5)
POISON_W, POISON_H, POISON_SAMPLES = 8, 6, 4
# (name, what is poisoned): channel values that are +inf, NaN, -1 and 0 in albedos, light colours and multipliers
# and the background. Each factor is ordinary or non-finite by itself (DESIGN section 2 states the limit).
POISON_ALBEDOS = ((INF, 0.5, 0.25), (0.5, NAN, 0.25), (0.5, 0.25, -1.0), (0.0, 0.0, 0.0))
POISON_LIGHTS = (((1.0, 0.0, 0.5), INF), ((1.0, 0.9, 0.8), NAN), ((1.0, 0.9, 0.8), 0.0), ((1.0, 0.9, 0.8), -2.0))
POISON_BACKGROUNDS = (((INF, 0.4, 0.5), (0.7, 0.89, 1.0)), ((0.3, NAN, 0.5), (0.7, 0.89, 1.0)),
                      ((0.3, 0.4, 0.5), (0.7, 0.89, -1.0)))
POISON_NAMES = tuple(f"poison_{mode}_{k}" for mode in ("spheres", "flat", "nest", "rich") for k in range(4)) + \
    ("poison_miss",)


def _poison_objects(mode: str, k: int):
    """The world's objects for one scene mode: a floor, two poisoned spheres (Lambertian and Metal with albedo k),
    two ordinary ones and what forces the mode."""
    alb = POISON_ALBEDOS[k]
    h = HittableList()
    h.add(Sphere((-1.0, 0.0, 0.0), 1.0, Lambertian(C32(*alb))))
    h.add(Sphere((1.0, 0.0, 0.0), 1.0, Metal(C32(*POISON_ALBEDOS[(k + 1) % 4]))))
    h.add(Sphere((0.0, 0.0, -2.0), 1.0, Lambertian(C32(0.7, 0.3, 0.2))))
    h.add(Sphere((0.0, -101.0, 0.0), 100.0, Metal(C32(0.8, 0.8, 0.7))))
    if mode in ("flat", "rich"):
        h.add(AARect.new_xy(AARectMetrics(-4.0, (-4.0, 4.0), (-1.0, 4.0)), Lambertian(C32(*alb))))
    if mode == "nest":
        h.add(Intersection(Sphere((0.0, 2.0, 0.0), 1.0, None), Box((-1.0, 1.5, -1.0), (1.0, 2.5, 1.0), None),
                           Lambertian(C32(*alb))))
    if mode == "rich":
        from raysnail_amd.api import ConstantMedium
        h.add(ConstantMedium(Sphere((0.0, 2.0, 0.0), 1.0, None), C32(*alb), 1.5))
    return h


@functools.lru_cache(maxsize=None)
def poison_worlds():
    """name -> World. World k of a mode: albedo k on its Lambertians, albedo k + 1 on its Metal, light k (colour and
    multiplier), background k % 3. poison_miss: an ordinary world whose background differs in lo and hi, for the
    NaN-direction camera."""
    out = {}
    for mode in ("spheres", "flat", "nest", "rich"):
        for k in range(4):
            h = _poison_objects(mode, k)
            col, mul = POISON_LIGHTS[k]
            lamp = Sphere((0.0, 6.0, 2.0), 2.0, DiffuseLight(C32(*col)).multiplier(mul))
            h.add(lamp)
            lights = HittableList().add(lamp)
            lo, hi = POISON_BACKGROUNDS[k % 3]
            out[f"poison_{mode}_{k}"] = World(h, lights, Gradient(C32(*lo), C32(*hi)), (0.0, 0.0))
    h = HittableList()
    h.add(Sphere((0.0, 0.0, 0.0), 1.0, Lambertian(C32(0.7, 0.3, 0.2))))
    lamp = Sphere((0.0, 6.0, 2.0), 2.0, DiffuseLight(C32(1.0, 0.9, 0.8)).multiplier(4.0))
    h.add(lamp)
    out["poison_miss"] = World(h, HittableList().add(lamp), Gradient(C32(0.125, 0.25, 0.5), C32(1.0, 0.75, 0.625)),
                               (0.0, 0.0))
    return out


POISON_EXPECT_MODE = {"spheres": 1, "flat": 2, "nest": 4, "rich": 0}


def poison_camera() -> Entry:
    return Entry("poison", "poison_cam", "an ordinary camera over the poisoned worlds", look_from=(0.5, 1.5, 6.0),
                 look_at=(0.0, 0.25, 0.0), fov=50.0, aperture=0.125, focus=6.0, shutter=0.0, width=POISON_W,
                 height=POISON_H, samples=POISON_SAMPLES)


@functools.lru_cache(maxsize=None)
def poison_reference(wname: str, depth: int, gamma: int):
    """(frame, (segments, samples)) of the oracle: once per (world, depth, gamma)."""
    c = poison_camera() if wname != "poison_miss" else camera("focus0_pinhole")
    d = c.desc(POISON_W, POISON_H)
    return _freeze(*frame_oracle(wname).render(d, c.settings(samples=POISON_SAMPLES, depth=depth, gamma=gamma), threads=8))


@functools.lru_cache(maxsize=None)
def poison_sample_reference(wname: str, depth: int) -> np.ndarray:
    """(H, W, N, 4): the oracle's radiance and World::hit count of every sample (orc_sample_radiance)."""
    c = poison_camera()
    d, st = c.desc(), c.settings(depth=depth)
    orc = frame_oracle(wname)
    out = np.zeros((POISON_H, POISON_W, POISON_SAMPLES, 4))
    for y, x, s in itertools.product(range(POISON_H), range(POISON_W), range(POISON_SAMPLES)):
        rad, seg = orc.sample_radiance(d, st, x, y, s)
        out[y, x, s, :3] = rad
        out[y, x, s, 3] = seg
    out.setflags(write=False)
    return out
