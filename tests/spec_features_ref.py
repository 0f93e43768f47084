"""Expected specular-chain feature frames (rs_render_features_specular) from the CPU oracle alone.

features_ref's camera rays, hit records and albedo, then per sample the chain of include/raysnail_hip.h: World::hit,
and while the hit's resolved material is Metal or Dielectric and the bounce budget lasts, the material's own next ray:
  Metal       orc_scatter on a Metal twin (solid texture: the ray does not read it). ok = 0 is metal.rs:112's
              below-surface rejection, a terminal hit. The tint is features_ref.Albedo's colour of the hit (the same
              texture.color the scatter record carries).
  Dielectric  orc_scatter on a twin registered without `glass`: reflect_prob is 0 and the draw cannot matter (checked
              by tests/test_spec_features_cpu.py over rng seeds). The tint is texture.even.
Nothing of the chain's ray arithmetic is restated here; only the classification of a Dielectric bounce as a total
internal reflection (refractive * sin_theta > 1.0, dielectric.rs:58-63, in f64) is, for the fixture statistics.
Summed in f64 in sample order from +0.0, divided by N, cast to f32, as features_ref.expected.
"""
import ctypes as C
import functools
import math

import numpy as np

import features_ref as F
from oracle import binding
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

# how a sample's chain ended
MISS, TERMINAL_FIRST, TERMINAL_AFTER, ESCAPE, LIMIT, METAL_REJECTED = range(6)
ENDINGS = ("miss", "terminal at k = 0", "terminal at k >= 1", "escape", "limit", "metal rejection")


class MediumRecorder(F.Recorder):
    """features_ref.Recorder that also keeps the Isotropic material a ConstantMedium creates for itself
    (constant.rs:29-39): both backends give it the next material id, and a chain can end on it inside glass"""

    def __getattr__(self, name):
        f = super().__getattr__(name)
        if name[len(self._prefix):] != "constant_medium":
            return f

        def call(handle, boundary, color, density, out):
            rc = f(handle, boundary, color, density, out)
            if rc == 0:
                d = A.rs_material_desc()
                d.kind, d.texture.kind = A.RS_MAT_ISOTROPIC, A.RS_TEX_SOLID
                d.texture.even[:] = color[:]
                assert sorted(self.materials) == list(range(len(self.materials)))  # ids are dense: the next one
                self.materials[len(self.materials)] = d
            return rc
        return call


def oracle_scene(world):
    """features_ref.oracle_scene with a MediumRecorder"""
    lib = binding.load()
    rec = MediumRecorder(lib, "orc_")
    orc = binding.OracleScene.__new__(binding.OracleScene)
    orc.lib = lib
    orc.h = C.c_void_p(lib.orc_scene_create())
    api.realize(world, rec, orc.h, "orc_")
    api._check(lib, lib.orc_commit(orc.h), "orc_")
    return orc, rec


class Bouncer:
    """hit record + incoming ray -> the specular material's next ray, from orc_scatter on twins living in the Albedo's
    texture-only oracle scene"""

    def __init__(self, albedo):
        self.albedo, self.rec, self.lib, self.h = albedo, albedo.rec, albedo.lib, albedo.h
        self.twin = {}
        for mid, d in self.rec.materials.items():
            if d.kind not in (A.RS_MAT_METAL, A.RS_MAT_DIELECTRIC):
                continue
            t = A.rs_material_desc()
            t.kind, t.glass = d.kind, 0
            t.texture.kind = A.RS_TEX_SOLID
            t.texture.even[:] = d.texture.even[:] if d.kind == A.RS_MAT_DIELECTRIC else (1.0, 1.0, 1.0, 1.0)
            t.refractive, t.multiplier, t.mix_p = d.refractive, 1.0, 0.5
            out = C.c_int32()
            api._check(self.lib, self.lib.orc_material(self.h, C.byref(t), C.byref(out)), "orc_")
            self.twin[mid] = out.value

    def resolve(self, rec13):
        """(material id, descriptor) after MixedMaterial -> material_1, or (-1, None) for the world's default"""
        mid = int(rec13[12])
        if mid < 0:
            return -1, None
        d = self.rec.materials[mid]
        for _ in range(16):
            if d.kind != A.RS_MAT_MIXED:
                break
            mid = d.mix_a
            d = self.rec.materials[mid]
        return mid, d

    def scatter(self, mid, ray7, rec13, rng_seed=1):
        ray = (C.c_double * 7)(*ray7)
        hit = (C.c_double * 8)(rec13[3], rec13[4], rec13[5], rec13[6], rec13[7], rec13[8], rec13[1], rec13[11])
        out = (C.c_double * 16)()
        api._check(self.lib, self.lib.orc_scatter(self.h, self.twin[mid], ray, hit, rng_seed, out), "orc_")
        return list(out)

    def __call__(self, ray7, rec13):
        """None: not a specular kind. Otherwise (next ray or None for Metal's rejection, tint rgb, is a total internal
        reflection)"""
        mid, d = self.resolve(rec13)
        if d is None or d.kind not in (A.RS_MAT_METAL, A.RS_MAT_DIELECTRIC):
            return None
        out = self.scatter(mid, ray7, rec13)
        if d.kind == A.RS_MAT_METAL:
            if out[0] != 1.0:
                return None, None, False
            assert out[2] == 1.0
            return np.array(out[6:12] + [ray7[6]]), self.albedo(rec13), False
        assert out[0] == 1.0 and out[2] == 1.0
        dx, dy, dz = ray7[3:6]
        nx, ny, nz = rec13[6:9]
        cos_theta = (-dx) * nx + (-dy) * ny + (-dz) * nz
        sin_theta = math.sqrt(1.0 - cos_theta * cos_theta) if 1.0 - cos_theta * cos_theta >= 0.0 else float("nan")
        refr = 1.0 / d.refractive if rec13[11] != 0.0 else d.refractive  # dielectric.rs:35-41, :57
        tint = tuple(float(np.float32(c)) for c in d.texture.even[:3])
        return np.array(out[6:12] + [ray7[6]]), tint, bool(refr * sin_theta > 1.0)


class Chains:
    """the per-sample results of a pixel rectangle: vals [n_pix, N, 8], ending / bounces / tir / calls [n_pix, N]"""

    def __init__(self, vals, ending, bounces, tir, calls, w, h):
        self.vals, self.ending, self.bounces, self.tir, self.calls, self.w, self.h = vals, ending, bounces, tir, calls, w, h

    def frames(self):
        """(albedo frame, normal frame), (h, w, 4) float32 each"""
        n_pix, N = self.vals.shape[:2]
        acc = np.zeros((n_pix, 8))
        for s in range(N):  # sample order, from +0.0
            acc = acc + self.vals[:, s]
        with np.errstate(invalid="ignore", divide="ignore"):
            fr = (acc / np.float64(N)).astype(np.float32).reshape(self.h, self.w, 8)
        return np.ascontiguousarray(fr[..., 0:4]), np.ascontiguousarray(fr[..., 4:8])

    def count(self, ending):
        return int((self.ending == ending).sum())

    def hitting(self):
        return self.ending != MISS


def chains(cam, st, hit_fn, albedo, max_specular, x0=0, y0=0, w=None, h=None, bouncer=None):
    """The chains of every sample of the pixel rectangle [x0, x0 + w) x [y0, y0 + h)."""
    w = cam.width - x0 if w is None else w
    h = cam.height - y0 if h is None else h
    pixels = [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
    rays = F.camera_rays(cam, st, pixels)
    n_pix, N = rays.shape[:2]
    vals, ending, bounces, tir, calls = trace(rays.reshape(-1, 7), hit_fn, albedo, bouncer or Bouncer(albedo), max_specular)
    sh = (n_pix, N)
    return Chains(vals.reshape(n_pix, N, 8), ending.reshape(sh), bounces.reshape(sh), tir.reshape(sh), calls.reshape(sh), w, h)


def trace(rays, hit_fn, albedo, bouncer, max_specular):
    """The chains of rays [M, 7], one hit_fn call per chain level over the rays still going: (the 8 channels each
    contributes [M, 8], how it ended, its bounces, those of them that were total internal reflections, its World::hit
    calls)"""
    ray = np.array(rays, dtype=np.float64)
    M = len(ray)
    vals = np.zeros((M, 8))
    T = np.ones((M, 3))
    depth = np.zeros(M)
    n_prev = np.zeros((M, 3))
    ending = np.full(M, MISS)
    bounces, tir, calls = np.zeros(M, int), np.zeros(M, int), np.zeros(M, int)
    going = np.arange(M)
    for k in range(max_specular + 1):
        if len(going) == 0:
            break
        recs = hit_fn(ray[going])
        nxt = []
        for i, r in zip(going, recs):
            calls[i] += 1
            if r[0] != 1.0:
                if k > 0:  # the chain escapes
                    vals[i] = (T[i, 0], T[i, 1], T[i, 2], 1.0, n_prev[i, 0], n_prev[i, 1], n_prev[i, 2], depth[i])
                    ending[i] = ESCAPE
                continue
            depth[i] = r[1] if k == 0 else depth[i] + r[1]
            step = bouncer(ray[i], r)
            specular_kind = step is not None
            if specular_kind and k < max_specular and step[0] is not None:
                nray, tint, is_tir = step
                T[i] = (T[i, 0] * tint[0], T[i, 1] * tint[1], T[i, 2] * tint[2])
                ray[i] = nray
                n_prev[i] = r[6:9]
                bounces[i] += 1
                tir[i] += int(is_tir)
                nxt.append(i)
                continue
            c = albedo(r)
            vals[i] = (T[i, 0] * c[0], T[i, 1] * c[1], T[i, 2] * c[2], 1.0, r[6], r[7], r[8], depth[i])
            if specular_kind and k < max_specular:
                ending[i] = METAL_REJECTED
            elif specular_kind:
                ending[i] = LIMIT
            else:
                ending[i] = TERMINAL_FIRST if k == 0 else TERMINAL_AFTER
        going = np.array(nxt, int)
    return vals, ending, bounces, tir, calls


# ---------------------------------------------------------------- the fixtures of the GPU tests ----
def mesh_glass_scene(width=32, height=20):
    """scenes.mesh_scene's objects and camera (196 triangles) with a Dielectric mesh: a flat mesh tree (mode 2)"""
    pos, nrm = scenes.synthetic_mesh(8, 14)
    hl, lights = api.HittableList(), api.HittableList()
    hl.add(api.TriangleMesh(pos, nrm, api.Dielectric(scenes.C32(0.9, 0.95, 1.0), 1.5).reflect_curve(api.Glass())))
    hl.add(api.Sphere((0.0, -1000.0, 0.0), 1000.0, api.Lambertian(scenes.C32(0.5, 0.5, 0.5))))
    light = api.Sphere((300.0, 400.0, 100.0), 12.0, api.DiffuseLight(scenes.C32(1.0, 0.9, 0.7)).multiplier(1.5))
    lights.add(light)
    hl.add(light)
    cam = api.CameraBuilder().look_from(api.Point3(0.0, 2.0, 5.0)).look_at(api.Point3(0.0, 0.9, 0.0)).fov(40.0) \
        .width(width).height(height).build()
    return cam, api.World(hl, lights, api.Gradient(scenes.C32(0.3, 0.4, 0.5), scenes.C32(0.7, 0.89, 1.0)), (0.0, 0.0))


def hall_of_mirrors(width=16, height=10):
    """two facing Metal rects (z = -2 and z = +3, 2000 x 2000) with the eye between them: every camera ray hits a
    mirror and no chain of 17 walks leaves the gap; the light is behind a mirror"""
    hl, lights = api.HittableList(), api.HittableList()
    big = api.AARectMetrics(-2.0, (-1000.0, 1000.0), (-1000.0, 1000.0))
    hl.add(api.AARect.new_xy(big, api.Metal(scenes.C32(0.9, 0.8, 0.7))))
    hl.add(api.AARect.new_xy(api.AARectMetrics(3.0, big.a, big.b), api.Metal(scenes.C32(0.7, 0.9, 0.8))))
    light = api.Sphere((0.0, 0.0, 60.0), 5.0, api.DiffuseLight(scenes.C32(1.0, 1.0, 1.0)))
    lights.add(light)
    hl.add(light)
    cam = api.CameraBuilder().look_from(api.Point3(0.0, 0.0, 0.0)).look_at(api.Point3(0.3, 0.2, -2.0)).fov(50.0) \
        .width(width).height(height).build()
    return cam, api.World(hl, lights, api.Gradient(scenes.C32(0.3, 0.4, 0.5), scenes.C32(0.7, 0.89, 1.0)), (0.0, 0.0))


def inside_glass(width=16, height=10):
    """the eye inside a glass sphere (radius 1, index 1.5) at 0.8 of its radius, looking along the surface: rays that
    meet it beyond the critical angle reflect inside for good (the limit), the others leave for the sky (escape) or a
    diffuse sphere outside (terminal after bounces)"""
    hl, lights = api.HittableList(), api.HittableList()
    hl.add(api.Sphere((0.0, 0.0, 0.0), 1.0, api.Dielectric(scenes.C32(0.9, 1.0, 0.9), 1.5).reflect_curve(api.Glass())))
    hl.add(api.Sphere((2.5, 1.2, 0.0), 1.0, api.Lambertian(scenes.C32(0.7, 0.3, 0.1))))
    light = api.Sphere((0.0, 40.0, 0.0), 5.0, api.DiffuseLight(scenes.C32(1.0, 1.0, 1.0)))
    lights.add(light)
    hl.add(light)
    cam = api.CameraBuilder().look_from(api.Point3(0.8, 0.0, 0.0)).look_at(api.Point3(1.4, 1.0, 0.0)).fov(90.0) \
        .width(width).height(height).build()
    return cam, api.World(hl, lights, api.Gradient(scenes.C32(0.3, 0.4, 0.5), scenes.C32(0.7, 0.89, 1.0)), (0.0, 0.0))


def rich_glass_scene(width=32, height=20):
    """scenes.materials_scene's world (the rich generic mode: Perlin, Image, BlinnPhong, an Isotropic medium inside a
    glass sphere) under a camera turned to the glass sphere, so that a tenth of the hits and more start a chain"""
    _, world = scenes.materials_scene(width, height)
    cam = api.CameraBuilder().look_from(api.Point3(9.0, 3.0, 7.0)).look_at(api.Point3(2.0, 1.1, -1.0)).fov(14.0) \
        .aperture(0.02).focus(10.0).width(width).height(height).build()
    return cam, world


def marcher_metal(width=16, height=10):
    """scenes.raymarching_test with a Metal Mandelbulb (the oracle has no marcher: hit records from probe_hits)"""
    cam, world, _, _ = scenes.raymarching_test(width, height)
    for obj in world.hittables.objects:
        if isinstance(obj, api.RayMarcher):
            obj.material = api.Metal(scenes.C32(0.9, 0.7, 0.5))
    return cam, world


def _photo(cam, samples, seed, pass_index):
    return cam.take_photo().samples(samples).seed(seed).pass_index(pass_index)


# name -> (scene builder, samples, seed, pass, the max_specular values the GPU tests render, scene mode)
FIXTURES = {
    "features": (lambda: scenes.features_scene(48, 30), 10, 5, 1, (0, 1, 4), None),
    "spheres": (lambda: scenes.rtow_13_1(32, 20, seed=7)[:2], 4, 11, 2, (3,), 1),
    "mesh": (mesh_glass_scene, 4, 11, 2, (3,), 2),
    "rich": (rich_glass_scene, 4, 11, 2, (3,), 0),
    "hall": (hall_of_mirrors, 4, 2, 0, (1, 2, 16), None),
    "tir": (inside_glass, 4, 2, 0, (8,), None),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(camera, world, photo, OracleScene, Albedo, Bouncer) of a fixture, built once per process"""
    build, samples, seed, pass_index, _, _ = FIXTURES[name]
    cam, world = build()
    orc, rec = oracle_scene(world)
    alb = F.Albedo(rec)
    return cam, world, _photo(cam, samples, seed, pass_index), orc, alb, Bouncer(alb)


@functools.lru_cache(maxsize=None)
def fixture_chains(name, max_specular):
    """the oracle's chains of the whole frame of a fixture, computed once per process and shared (read only)"""
    cam, _, photo, orc, alb, bouncer = fixture(name)
    ch = chains(cam.desc, photo.settings(), F.oracle_hits(orc), alb, max_specular, bouncer=bouncer)
    for a in (ch.vals, ch.ending, ch.bounces, ch.tir, ch.calls):
        a.setflags(write=False)
    return ch
