"""Expected material-id mattes (rs_render_mattes) and their extraction (rs_matte_extract) from the CPU oracle alone.

features_ref's camera rays and hit records, then per sample the chain of include/raysnail_hip.h as
spec_features_ref walks it (its Bouncer: the specular material's own next ray from orc_scatter, its classification of a
hit); what a sample keeps is not a colour but an id -- the terminal hit's material id exactly as the hit record carries
it (field 12; no MixedMaterial resolution), or the background id when the camera ray or a bounced ray leaves the scene.
Then, per pixel, the contract's counting and ranking restated with a dictionary and a sort.
"""
import numpy as np

import features_ref as F
import spec_features_ref as R
from raysnail_amd import _abi as A

BACKGROUND, EMPTY = A.RS_MATTE_ID_BACKGROUND, A.RS_MATTE_ID_EMPTY
MAX_DISTINCT = A.RS_MATTE_MAX_DISTINCT


def sample_ids(rays, hit_fn, bouncer, max_specular):
    """The ids of rays [M, 7] and each chain's World::hit calls, one hit_fn call per chain level over the rays still
    going (spec_features_ref.trace's loop, keeping the id)."""
    ray = np.array(rays, dtype=np.float64)
    M = len(ray)
    ids = np.full(M, BACKGROUND, np.int64)
    calls = np.zeros(M, int)
    going = np.arange(M)
    for k in range(max_specular + 1):
        if len(going) == 0:
            break
        recs = hit_fn(ray[going])
        nxt = []
        for i, r in zip(going, recs):
            calls[i] += 1
            if r[0] != 1.0:
                continue  # a miss at k = 0, an escape after: the background
            step = bouncer(ray[i], r) if k < max_specular else None
            if step is not None and step[0] is not None:
                ray[i] = step[0]
                nxt.append(i)
                continue
            ids[i] = int(r[12])  # terminal: any other material, a specular one at the limit, Metal's rejection
        going = np.array(nxt, int)
    return ids, calls


def rank_ids(ids, ranks):
    """One pixel: the ids of its N samples -> (ids [ranks] int32, cov [ranks] float32, overflow 0 / 1)"""
    ids = [int(i) for i in ids]
    N = len(ids)
    count = {}
    for i in ids:
        count[i] = count.get(i, 0) + 1
    kept = sorted(count)  # signed ascending
    overflow = 1 if len(kept) > MAX_DISTINCT else 0
    kept = kept[:MAX_DISTINCT]
    order = sorted(kept, key=lambda i: (-count[i], i))
    out_i = np.full(ranks, EMPTY, np.int32)
    out_c = np.zeros(ranks, np.float32)
    for r, i in enumerate(order[:ranks]):
        out_i[r] = i
        out_c[r] = np.float32(np.float64(count[i]) / np.float64(N))
    return out_i, out_c, overflow


def layers(ids, w, h, ranks):
    """sample ids [h * w, N] -> (ids (h, w, ranks) int32, cov (h, w, ranks) float32, overflow (h, w) uint8); N = 0:
    every rank empty"""
    out_i = np.full((h * w, ranks), EMPTY, np.int32)
    out_c = np.zeros((h * w, ranks), np.float32)
    out_o = np.zeros(h * w, np.uint8)
    if ids.shape[1] > 0:
        for p in range(h * w):
            out_i[p], out_c[p], out_o[p] = rank_ids(ids[p], ranks)
    return out_i.reshape(h, w, ranks), out_c.reshape(h, w, ranks), out_o.reshape(h, w)


def frame_ids(cam, st, hit_fn, bouncer, max_specular):
    """(sample ids [H * W, N], World::hit calls [H * W, N]) of the whole frame (every pixel: masks and row lattices
    are the caller's)"""
    pixels = [(x, y) for y in range(cam.height) for x in range(cam.width)]
    rays = F.camera_rays(cam, st, pixels)
    n_pix, N = rays.shape[:2]
    ids, calls = sample_ids(rays.reshape(-1, 7), hit_fn, bouncer, max_specular)
    ids, calls = ids.reshape(n_pix, N), calls.reshape(n_pix, N)
    ids.setflags(write=False)
    calls.setflags(write=False)
    return ids, calls


def matte_extract(ids, cov, wanted):
    """rs_matte_extract restated: per pixel the f32 sum from +0.0, in rank order, of the coverages whose id is wanted
    and not empty"""
    ids, cov = np.asarray(ids, np.int32), np.asarray(cov, np.float32)
    wanted = set(int(i) for i in wanted)
    out = np.zeros(ids.shape[:2], np.float32)
    for r in range(ids.shape[2]):
        take = np.isin(ids[..., r], sorted(wanted)) & (ids[..., r] != EMPTY)
        out = np.where(take, (out + cov[..., r]).astype(np.float32), out)
    return out


# ---------------------------------------------------------------- the special fixtures of the tests ----
def _light(hl, lights):
    from raysnail_amd import api, scenes
    light = api.Sphere((0.0, 400.0, 300.0), 12.0, api.DiffuseLight(scenes.C32(1.0, 1.0, 1.0)))
    lights.add(light)
    hl.add(light)
    return light.material


def tie_scene(left_first, width=5, height=3):
    """A pinhole camera at the origin looking down -z at two coplanar rects (z = -2) that meet on x = 0, the centre
    line of the frame's middle pixel column: with an even sqrt_spp half of such a pixel's stratum centres lie on either
    side and none on the line. left_first: which rect (and so which material) is created first. Returns (camera,
    world, left material, right material)."""
    from raysnail_amd import api, scenes
    hl, lights = api.HittableList(), api.HittableList()
    left = api.AARect.new_xy(api.AARectMetrics(-2.0, (-50.0, 0.0), (-50.0, 50.0)), api.Lambertian(scenes.C32(0.8, 0.2, 0.2)))
    right = api.AARect.new_xy(api.AARectMetrics(-2.0, (0.0, 50.0), (-50.0, 50.0)), api.Lambertian(scenes.C32(0.2, 0.2, 0.8)))
    for o in ((left, right) if left_first else (right, left)):
        hl.add(o)
    _light(hl, lights)
    cam = api.CameraBuilder().look_from(api.Point3(0.0, 0.0, 0.0)).look_at(api.Point3(0.0, 0.0, -1.0)).fov(40.0) \
        .width(width).height(height).build()
    return cam, api.World(hl, lights), left.material, right.material


LATTICE_SAMPLES, LATTICE_SEED, LATTICE_SHIFT = 100, 9, 3


def lattice_scene():
    """A 3 x 2 frame, a pinhole camera with a narrow field of view at z = 10 looking at the plane z = 0, and a 10 x 10
    lattice of small spheres on that plane, each with a material of its own (ids 0 .. 99 in row-major creation order):
    the spheres sit where the 100 stratum-centre rays of pixel (1, 0) meet the plane, moved LATTICE_SHIFT strata to
    the left. So pixel (1, 0) sees 70 spheres and the background through the other 30 strata (71 distinct ids: more
    than RS_MATTE_MAX_DISTINCT), pixel (0, 0) 30 spheres and the background, the other pixels the background alone.
    Returns (camera, world, photo, the spheres' materials)."""
    from raysnail_amd import api, scenes
    cam = api.CameraBuilder().look_from(api.Point3(0.0, 0.0, 10.0)).look_at(api.Point3(0.0, 0.0, 0.0)) \
        .fov(float(np.degrees(2.0 * np.arctan(0.1)))).width(3).height(2).build()
    photo = cam.take_photo().samples(LATTICE_SAMPLES).seed(LATTICE_SEED).pass_index(0)
    rays = F.camera_rays(cam.desc, photo.settings(), [(1, 0)])[0]  # (a pinhole: the stream key does not matter)
    on_plane = rays[:, 0:3] + rays[:, 3:6] * (-rays[:, 2] / rays[:, 5])[:, None]
    pitch = on_plane[1] - on_plane[0]
    hl, lights = api.HittableList(), api.HittableList()
    mats = []
    for p in on_plane:
        c = p - LATTICE_SHIFT * pitch
        mats.append(api.Lambertian(scenes.C32(0.5, 0.5, 0.5)))
        hl.add(api.Sphere((float(c[0]), float(c[1]), 0.0), 0.3 * float(np.linalg.norm(pitch)), mats[-1]))
    _light(hl, lights)
    return cam, api.World(hl, lights), photo, mats
