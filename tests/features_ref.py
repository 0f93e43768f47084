"""Expected first-hit feature frames (rs_render_features) from the CPU oracle alone.

Per pixel and sample: orc_stream_key -> orc_camera_ray at the stratum centre -> a World::hit record (orc_world_hit,
or any `hit_fn` with its 13-double layout) -> the albedo of the record's material id: constants for the untextured
kinds, orc_scatter on a Lambertian twin carrying the same texture for Checker / Perlin, image.rs:34-50 restated on
the record's (u, v) for Image. Summed in f64 in sample order from +0.0, divided by N, cast to f32.
"""
import ctypes as C
import math

import numpy as np

from oracle import binding
from raysnail_amd import _abi as A
from raysnail_amd import api

INF = float("inf")
TMIN = 1e-4


class Recorder:
    """A backend library seen through realize(): every call goes to `lib`; the perlin, image and material calls are
    kept (descriptor copies by the id the backend returned)."""

    def __init__(self, lib, prefix):
        self._lib, self._prefix = lib, prefix
        self.perlins, self.images, self.materials = [], {}, {}

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        kind = name[len(self._prefix):]
        if kind not in ("perlin", "image", "material"):
            return f

        def call(handle, *args):
            rc = f(handle, *args)
            if rc != 0:
                return rc
            if kind == "perlin":
                self.perlins.append(A.rs_perlin_desc.from_buffer_copy(args[0]._obj))  # tables stay the world's
                assert args[1]._obj.value == len(self.perlins) - 1
            elif kind == "image":
                ptr, w, h, out = args
                self.images[out._obj.value] = np.frombuffer(C.string_at(ptr, 3 * w * h), np.uint8).reshape(h, w, 3).copy()
            else:
                self.materials[args[1]._obj.value] = A.rs_material_desc.from_buffer_copy(args[0]._obj)
            return rc
        return call


def oracle_scene(world):
    """(OracleScene of the world, the Recorder that saw its materials by oracle id)"""
    lib = binding.load()
    rec = Recorder(lib, "orc_")
    orc = binding.OracleScene.__new__(binding.OracleScene)
    orc.lib = lib
    orc.h = C.c_void_p(lib.orc_scene_create())
    api.realize(world, rec, orc.h, "orc_")
    api._check(lib, lib.orc_commit(orc.h), "orc_")
    return orc, rec


def device_scene(world, devices=None):
    """(DeviceScene of the world, the Recorder that saw its materials by library id); for worlds the oracle cannot
    hold (RayMarcher)"""
    lib = A.load()
    rec = Recorder(lib, "rs_")
    ds = api.DeviceScene.__new__(api.DeviceScene)
    ds.lib = lib
    ds.handle = C.c_void_p()
    api._check(lib, lib.rs_scene_create(C.byref(ds.handle)), "rs_")
    api.realize(world, rec, ds.handle, "rs_")
    if devices is None:
        api._check(lib, lib.rs_scene_commit(ds.handle), "rs_")
    else:
        api._check(lib, lib.rs_scene_commit_devices(ds.handle, (C.c_int * max(1, len(devices)))(*devices), len(devices)), "rs_")
    world._scene = ds
    return ds, rec


class Albedo:
    """material id of a hit record -> f32 rgb (as f64), from a Recorder's descriptors. Checker and Perlin colours
    come from orc_scatter on a Lambertian twin of the material in a texture-only oracle scene."""

    def __init__(self, rec):
        self.rec = rec
        self.lib = binding.load()
        self.h = C.c_void_p(self.lib.orc_scene_create())
        for pd in rec.perlins:
            out = C.c_int32()
            api._check(self.lib, self.lib.orc_perlin(self.h, C.byref(pd), C.byref(out)), "orc_")
        self.twin = {}
        for mid, d in rec.materials.items():
            if d.texture.kind in (A.RS_TEX_CHECKER, A.RS_TEX_PERLIN):
                t = A.rs_material_desc()
                t.kind, t.texture = A.RS_MAT_LAMBERTIAN, d.texture
                t.refractive, t.multiplier, t.mix_p = 1.0, 1.0, 0.5
                out = C.c_int32()
                api._check(self.lib, self.lib.orc_material(self.h, C.byref(t), C.byref(out)), "orc_")
                self.twin[mid] = out.value

    def __del__(self):
        try:
            self.lib.orc_scene_destroy(self.h)
        except Exception:
            pass

    def __call__(self, rec13):
        mid = int(rec13[12])
        if mid < 0:
            return (1.0, 1.0, 1.0)  # world.rs:51: Lambertian(Color(1, 1, 1, 1))
        d = self.rec.materials[mid]
        for _ in range(16):
            if d.kind != A.RS_MAT_MIXED:
                break
            mid = d.mix_a  # material_1, as settings() (mixed_material.rs:56-58)
            d = self.rec.materials[mid]
        if d.kind in (A.RS_MAT_DIELECTRIC, A.RS_MAT_ISOTROPIC) or d.texture.kind == A.RS_TEX_SOLID:
            return tuple(float(np.float32(c)) for c in d.texture.even[:3])
        if d.texture.kind == A.RS_TEX_IMAGE:
            return self.image(self.rec.images[d.texture.data], rec13[9], rec13[10])
        ray = (C.c_double * 7)(0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0)
        hit = (C.c_double * 8)(rec13[3], rec13[4], rec13[5], rec13[6], rec13[7], rec13[8], rec13[1], rec13[11])
        out = (C.c_double * 16)()
        api._check(self.lib, self.lib.orc_scatter(self.h, self.twin[mid], ray, hit, 1, out), "orc_")
        assert out[0] == 1.0
        return (out[3], out[4], out[5])

    @staticmethod
    def image(rgb, u, v):
        """image.rs:34-50 (`as u32` saturates: NaN and negatives give 0)"""
        h, w = rgb.shape[:2]

        def texel(t, n):
            t = t * float(n)
            k = 0 if not t >= 0.0 else (0xFFFFFFFF if t >= 4294967296.0 else int(t))
            return min(k, n - 1)
        px = rgb[texel(1.0 - v, h), texel(u, w)]
        return tuple(float(np.float32(c) / np.float32(255.0)) for c in px)


def camera_rays(cam, st, pixels):
    """rays [len(pixels), N, 7] of the stratum-centre samples of the pixels (x, y)"""
    lib = binding.load()
    W, H = cam.width, cam.height
    sq = int(math.floor(math.sqrt(st.samples)))
    N = sq * sq
    rays = np.zeros((len(pixels), N, 7))
    out = (C.c_double * 7)()
    for k, (x, y) in enumerate(pixels):
        for s in range(N):
            si, sj = s % sq, s // sq
            xo = float(x) + (float(si) + 0.5) / float(sq)
            yo = float(y) + (float(sj) + 0.5) / float(sq)
            u = xo / float(W)
            v = (float(H) - 1.0 - yo) / float(H)
            key = lib.orc_stream_key(st.seed, st.pass_, y * W + x, s)
            lib.orc_camera_ray(C.byref(cam), u, v, key, out)
            rays[k, s] = out[:]
    return rays


def oracle_hits(orc):
    def hit_fn(rays):
        out = np.zeros((len(rays), 13))
        buf = (C.c_double * 13)()
        for k, r in enumerate(rays):
            api._check(orc.lib, orc.lib.orc_world_hit(orc.h, (C.c_double * 3)(*r[0:3]), (C.c_double * 3)(*r[3:6]), r[6], TMIN,
                                                      INF, buf), "orc_")
            out[k] = buf[:]
        return out
    return hit_fn


def probe_hits(ds):
    """World::hit records of the library's own probe (pinned against tests/raymarch_ref.py for the marcher)"""
    def hit_fn(rays):
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        out = np.zeros((len(rays), 13))
        assert ds.lib.rs_probe_world_hit(ds.handle, rays.ctypes.data, len(rays), TMIN, INF, out.ctypes.data) == 0
        return out
    return hit_fn


def expected(cam, st, hit_fn, albedo, x0=0, y0=0, w=None, h=None):
    """(albedo frame, normal frame, hit fraction) of the pixel rectangle [x0, x0 + w) x [y0, y0 + h), each frame
    (h, w, 4) float32. Every pixel of the rectangle is computed: masks and row lattices are the caller's."""
    w = cam.width - x0 if w is None else w
    h = cam.height - y0 if h is None else h
    pixels = [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
    rays = camera_rays(cam, st, pixels)
    n_pix, N = rays.shape[:2]
    recs = hit_fn(rays.reshape(-1, 7)).reshape(n_pix, N, 13)
    vals = np.zeros((n_pix, N, 8))
    for k in range(n_pix):
        for s in range(N):
            r = recs[k, s]
            if r[0] == 1.0:
                vals[k, s, 0:3] = albedo(r)
                vals[k, s, 3] = 1.0
                vals[k, s, 4:7] = r[6:9]
                vals[k, s, 7] = r[1]
    acc = np.zeros((n_pix, 8))
    for s in range(N):  # sample order, from +0.0
        acc = acc + vals[:, s]
    with np.errstate(invalid="ignore", divide="ignore"):
        frames = (acc / np.float64(N)).astype(np.float32).reshape(h, w, 8)
    hit_fraction = float(recs[..., 0].mean()) if N else 0.0
    return np.ascontiguousarray(frames[..., 0:4]), np.ascontiguousarray(frames[..., 4:8]), hit_fraction


def same_bits(a, b):
    """bitwise equality of two float32 arrays, NaNs of any payload comparing equal"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
