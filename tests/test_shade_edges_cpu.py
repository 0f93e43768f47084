"""Guards of tests/shade_edges.py's fixtures, on the CPU: the scenes commit into the modes they are meant for, the
material ids and the lights' order are what the rows assume, every family takes both sides of its branch on the oracle,
and the closed forms that hold exactly on the oracle's level do hold -- the independent half of
tests/test_gpu_shade_edges.py, which only compares the GPU with this oracle.

Which branch a row takes is read from the oracle's output where it shows there (a BSDF-branch ray starts at the hit
point, a light-branch ray does not) and from a restatement of the row's RNG stream (shade_edges.Rng, itself checked
against the oracle's state words here) where it does not: the branch draw, the light index, the cosine sample."""
import math

import numpy as np
import pytest

import edge_rays as E
import shade_edges as S
from raysnail_amd.api import DeviceScene, TriangleMesh

PI = 3.14159265358979323846


def _ctx(name, family):
    r, _ = S.rows(name)
    i = S.family_rows(name, family)
    ref = S.reference(name)
    return i, r[i], ref[i], S.light_branch(r[i], ref[i])


def _color(name, material):
    t = S.materials(name == "rich")[material].texture
    return np.array([t.r, t.g, t.b], dtype=np.float64)


def _same(a, b):
    return np.all(E.bits(np.asarray(a, dtype=np.float64)) == E.bits(np.asarray(b, dtype=np.float64)), axis=-1)


def _draws(row: int):
    """(light branch?, light index draw) of a row whose material draws nothing before the branch."""
    g = S.Rng(S.SEED, int(row))
    return g.gen() < 0.5, g.next_u32()


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_scenes(name):
    w = S.world(name)
    assert DeviceScene(w, devices=[]).info().scene_mode == S.EXPECT_MODE[name]
    n_lights = sum(len(o.positions) if isinstance(o, TriangleMesh) else 1 for o in w.lights.objects)
    assert n_lights == S.N_LIGHTS[name]
    assert S.N_LIGHTS["spheres"] == 3                       # a length that is no power of two
    orc = S.oracle(name)
    for k, m in enumerate(S.material_names(name)):           # the tag spheres: material ids in MATERIALS' order
        rec = orc.world_hit((k - 8.0, 1.0, 5.0), (0.0, 0.0, -1.0))
        assert rec[0] == 1.0 and rec[12] == S.ids(name)[m] == k
    assert orc.world_hit((9.0, 1.0, 5.0), (0.0, 0.0, -1.0))[12] == -1.0


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_tables(name):
    r, fam = S.rows(name)
    assert len(r) < 10000
    for f in S.families(name):
        assert 50 <= len(S.family_rows(name, f)) <= 700, f
    ref = S.reference(name)
    assert set(np.unique(ref[:, 0])) == {0.0, 1.0}
    assert not np.isnan(ref[:, 14:18]).any() and (ref[:, 14:18] == np.floor(ref[:, 14:18])).all()
    # NaN outputs in exactly the families built to make them (`generic` shades from lattice points, two of which are
    # a sphere light's centre)
    nan_families = {S.FAMILIES[k] for k in np.unique(fam[np.isnan(ref).any(axis=1)])}
    assert nan_families == {"generic", "diel_nan", "onb_zero", "pdf_floor", "lights", "checker_zero"} | (
        {"blinn_same", "perlin_edges"} if name == "rich" else set())


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_rng_restated(name):
    """shade_edges.Rng against the oracle's state words: Metal draws nothing, a Dielectric one gen(), a Lambertian
    BSDF row gen() + two more."""
    r, _ = S.rows(name)
    ref = S.reference(name)
    I = S.ids(name)
    n = {"metal": 0, "diel": 0, "lam": 0}
    normal = set(S.family_rows(name, "diel_normal").tolist())
    for i in range(len(r)):
        g = S.Rng(S.SEED, i)
        if r[i, 17] == I["metal"]:
            n["metal"] += 1
        elif r[i, 17] == I["diel"] and i in normal:           # (a total reflection returns before the draw)
            n["diel"] += 1
            g.gen()
        elif r[i, 17] == I["lam"] and ref[i, 0] == 1.0 and _same(ref[i, 7:10], r[i, 7:10]):
            n["lam"] += 1
            assert not g.gen() < 0.5
            g.gen(), g.gen()
        else:
            continue
        assert ref[i, 14:18].tolist() == g.words(), i
    assert n["metal"] >= 100 and n["lam"] >= 100 and n["diel"] == 24, n


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_dielectric_families(name):
    I = S.ids(name)
    # normal incidence: `diel` refracts to d itself; `glass` reflects to -d on some rows
    i, r, ref, _ = _ctx(name, "diel_normal")
    assert (ref[:, 0] == 1.0).all() and not np.isnan(ref).any()
    diel = r[:, 17] == I["diel"]
    # (as numbers: r_parallel = (d + n) * refr is +0 on every axis, so a -0 of d comes back as +0)
    assert np.array_equal(ref[diel, 10:13], r[diel, 3:6])
    back = np.all(ref[:, 10:13] == -r[:, 3:6], axis=1)
    assert (np.all(ref[:, 10:13] == r[:, 3:6], axis=1) | back).all() and not back[diel].any()
    assert 3 <= int(back[~diel].sum()) <= 40
    assert set(np.unique(r[:, 14])) == {0.0, 1.0}           # outside == 0 among them
    # total reflection: from inside iff 1.5 * sin_theta > 1 (the reflected ray goes back up), never from outside
    i, r, ref, _ = _ctx(name, "diel_tir")
    cos = -r[:, 4]
    sin = np.sqrt(1.0 - cos * cos)
    tir = (r[:, 14] == 0.0) & (1.5 * sin > 1.0)
    up = ref[:, 11] > 0.0
    diel = r[:, 17] == I["diel"]
    assert np.array_equal(up[diel], tir[diel]) and (up[tir]).all()
    assert 40 <= int(tir.sum()) <= len(r) - 40
    near = np.abs(r[:, 3] - S.TIR_S) < 1e-15                # the neighbours of 2/3, both sides of the branch
    assert int((near & tir).sum()) >= 4 and int((near & ~tir & (r[:, 14] == 0.0)).sum()) >= 4
    # a NaN direction with a finite factor
    i, r, ref, _ = _ctx(name, "diel_nan")
    nan_d = np.isnan(ref[:, 10:13]).any(axis=1)
    assert 10 <= int(nan_d.sum()) <= len(r) - 10
    assert (ref[:, 0] == 1.0).all() and np.isfinite(ref[:, 1:7]).all() and np.isfinite(ref[:, 7:10]).all()
    for m in ("diel", "glass"):
        rows = r[:, 17] == I[m]
        c = S.materials(False)[m].color
        assert _same(ref[rows, 4:7], np.array([c.r, c.g, c.b], dtype=np.float64)).all()


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_metal_family(name):
    """Absorbed iff dot(reflected, n) <= 0, which here is dot(d, n) >= 0 exactly; normal incidence returns -d."""
    I = S.ids(name)
    i, r, ref, _ = _ctx(name, "metal_graze")
    dn = np.sum(r[:, 3:6] * r[:, 10:13], axis=1)             # exact: one non-zero product, or 0 +- 2^-60
    assert np.array_equal(ref[:, 0] == 1.0, dn < 0.0)
    assert int((dn == 0.0).sum()) >= 100 and int((dn < 0.0).sum()) >= 20 and int((dn > 0.0).sum()) >= 8
    normal = _same(r[:, 3:6], -r[:, 10:13]) & (r[:, 17] == I["metal"])
    assert int(normal.sum()) == 6 and _same(ref[normal, 10:13], -r[normal, 3:6]).all()
    absorbed = ref[:, 0] == 0.0                               # no emission, the factor untouched, the ray its own
    assert (ref[absorbed, 1:4] == 0.0).all() and (ref[absorbed, 4:7] == 1.0).all()
    assert _same(ref[absorbed, 7:14], r[absorbed, 0:7]).all()


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_onb_families(name):
    col = _color(name, "lam")
    i, r, ref, light = _ctx(name, "onb_up")
    assert all(S.onb_takes_fallback(n) for n in r[:, 10:13]) and np.isfinite(ref).all()
    assert _same(ref[~light, 4:7], col).all() and 10 <= int(light.sum()) <= len(r) - 10
    # on either side of 1e-8: the restated branch, and the branch as the oracle's direction shows it -- for a normal
    # (eps, 1, 0) the u axis is (0, 0, 1) in the fallback and (0, 0, -1) otherwise, v.z = w.z = 0, so the BSDF ray's
    # d.z is +-(cos(2 pi r1) sqrt(r2)) of the cosine sample
    i, r, ref, light = _ctx(name, "onb_near")
    fb = np.array([S.onb_takes_fallback(n) for n in r[:, 10:13]])
    assert int(fb.sum()) >= 60 and int((~fb).sum()) >= 60 and np.isfinite(ref).all()
    assert _same(ref[~light, 4:7], col).all()
    seen = {True: 0, False: 0}
    for k in np.flatnonzero(~light & (r[:, 12] == 0.0) & (r[:, 11] == 1.0)):
        g = S.Rng(S.SEED, int(i[k]))
        assert not g.gen() < 0.5
        ax = math.cos(2.0 * PI * g.gen())
        if abs(ax) < 1e-6:
            continue
        assert (np.sign(ref[k, 12]) == np.sign(ax)) == bool(fb[k]), (k, r[k, 10:13])
        seen[bool(fb[k])] += 1
    assert min(seen.values()) >= 8, seen


CONSTANT_LIGHTS = ("box", "medium", "csg_box")   # (1, 0, 0): Box, ConstantMedium, a Difference whose first child is a Box


def _light_kinds(name):
    """index in the lights list -> kind (shade_edges._lights' order; the mesh is two entries)."""
    kinds = ["sphere", "sphere", "sphere", "rect", "rect", "rect", "tri", "tri", "quadric", "box", "tf", "tf", "csg",
             "csg_box", "medium"]
    return kinds[:S.N_LIGHTS[name]]


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_zero_vector_families(name):
    """unit(0): NaN directions exactly on the light rows whose drawn light sits at the hit point (a sphere's centre,
    the moving one's too: Sphere::random reads the centre at time 0) or is the quadric seen from the origin."""
    kinds = _light_kinds(name)
    centres = {0: S.SPHERE_LIGHT_CENTRES[0], 1: S.MOVING_LIGHT_CENTRE, 2: S.SPHERE_LIGHT_CENTRES[1]}
    i, r, ref, light = _ctx(name, "onb_zero")
    lam = r[:, 17] == S.ids(name)["lam"]
    at_point = np.any(r[:, 10:13] != 0.0, axis=1)            # the rows with a real normal
    n_nan = 0
    for k in np.flatnonzero(at_point):
        is_light, draw = _draws(i[k])
        assert is_light == bool(light[k])
        li = draw % len(kinds)
        p = tuple(r[k, 7:10])
        expect = is_light and ((li in centres and p == centres[li]) or (kinds[li] == "quadric" and p == (0.0, 0.0, 0.0)))
        assert bool(np.isnan(ref[k, 10:13]).all()) == expect == bool(np.isnan(ref[k]).any()), (k, li, p)
        n_nan += expect
    assert 4 <= n_nan <= int(at_point.sum()) - 8
    zero_n = ~at_point
    assert lam[zero_n].any() and (~lam[zero_n]).any()
    assert np.isnan(ref[zero_n & lam, 4:7]).all()            # a zero normal: the Lambertian's factor is NaN
    assert (ref[zero_n & ~lam, 0] == 0.0).all()              # DiffuseMetal: reflected = d, dot(d, 0) = 0: absorbed


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_light_start_family(name):
    i, r, ref, light = _ctx(name, "light_start")
    t = r[:, 13] - 0.0002
    start = r[:, 0:3] + r[:, 3:6] * t[:, None]               # the axis directions: one rounding, like mul_add
    assert _same(ref[light, 7:10], start[light]).all()
    assert int((light & (t < 0.0)).sum()) >= 10 and int((light & (t >= 0.0)).sum()) >= 5
    assert int((light & (t == 0.0)).sum()) >= 1
    assert _same(ref[~light, 7:10], r[~light, 7:10]).all() and 20 <= int(light.sum()) <= len(r) - 20


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_pdf_floor_family(name):
    """Replaced: a NaN pdf_val (then the factor is NaN / 1e-5) or, BlinnPhong, a negative one (then the factor is
    negative / 1e-5: negative and huge). Not replaced: mult is exactly 1 and the factor the texture colour."""
    I = S.ids(name)
    col = _color(name, "lam")
    i, r, ref, light = _ctx(name, "pdf_floor")
    lam = r[:, 17] == I["lam"]
    bad_n = ~np.isfinite(r[:, 10:13]).all(axis=1) | np.all(r[:, 10:13] == 0.0, axis=1)
    bsdf = lam & (ref[:, 0] == 1.0) & _same(ref[:, 7:10], r[:, 7:10])
    assert int((bsdf & bad_n).sum()) >= 8 and int((bsdf & ~bad_n).sum()) >= 5
    assert np.isnan(ref[bsdf & bad_n, 4:7]).all()
    assert _same(ref[bsdf & ~bad_n, 4:7], col).all()
    if name == "rich":
        blinn = (r[:, 17] == I["blinn"]) & ~light
        neg = blinn & (ref[:, 4] < -1.0)
        one = blinn & _same(ref[:, 4:7], _color(name, "blinn"))
        assert int(neg.sum()) >= 4 and int(one.sum()) >= 4 and np.array_equal(neg | one, blinn)


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_phong_lambert_family(name):
    """The same rows shaded as `lam` (equal colour, phong_factor 0): the same draws and rays; the factor differs
    on light rows only, where phong_highlight is positive, and is the closed form on the twin."""
    I = S.ids(name)
    i, r, ref, light = _ctx(name, "phong_lambert")
    rows = S.rows(name)[0].copy()
    rows[i, 17] = I["lam"]
    twin = S.oracle(name).shade_level(rows, S.SEED)[i]
    assert np.array_equal(E.bits(twin[:, 7:18]), E.bits(ref[:, 7:18])) and np.isfinite(ref).all()
    differ = ~_same(twin[:, 4:7], ref[:, 4:7])
    assert not differ[~light].any()
    assert int(differ.sum()) >= 10 and int((light & ~differ).sum()) >= 10
    assert (ref[differ, 4:7] >= twin[differ, 4:7]).all()
    # a Lambertian light row: mult == max(cos, 0) / pi / 0.3183098861837907, cos the next direction about the normal
    w = np.array([S.unit(n) for n in r[:, 10:13]])
    col = _color(name, "lam")
    for k in np.flatnonzero(light):
        d = ref[k, 10:13]
        c = float(S.Fraction(d[2]) * S.Fraction(w[k, 2]) + S.Fraction(float(S.Fraction(d[0]) * S.Fraction(w[k, 0]) +
                                                                                 S.Fraction(d[1] * w[k, 1]))))
        mult = (0.0 if c < 0.0 else c / PI) / S.COS_PDF
        if mult == 0.0:                                       # (the zero's sign is the cosine's)
            assert (twin[k, 4:7] == 0.0).all(), k
        else:
            assert _same(twin[k, 4:7], col * 1.0 * mult), k


def _checker_odd(p):
    s = [math.sin(2.0 * c) if math.isfinite(c) else S.NAN for c in p]
    return s[0] * s[1] * s[2] < 0.0


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_checker_family(name):
    I = S.ids(name)
    mats = S.materials(False)
    i, r, ref, light = _ctx(name, "checker_zero")
    n = {True: 0, False: 0}
    zero_plane = 0
    for k in range(len(r)):
        p = r[k, 7:10]
        if np.abs(p).max() > 4.0 and np.isfinite(p).all():
            continue                                          # huge arguments: the sign is the correctly rounded sine's
        odd = _checker_odd(p)
        if r[k, 17] == I["light"]:
            t, scale = mats["light"].texture, 4.0
            got = ref[k, 1:4]
            assert ref[k, 0] == 0.0
        elif not light[k]:
            t, scale = mats["checker"].texture, 1.0
            got = ref[k, 4:7]
        else:
            continue
        c = t.odd if odd else t.even
        assert _same(got, np.array([c.r, c.g, c.b], dtype=np.float64) * scale), (k, p)
        n[odd] += 1
        if np.any(p == 0.0):
            assert not odd
            zero_plane += 1
    assert n[True] >= 40 and n[False] >= 150 and zero_plane >= 150
    assert np.signbit(r[:, 7:10][r[:, 7:10] == 0.0]).any()  # -0.0 among the planes


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_lights_family(name):
    """Every entry of the lights list is drawn; the closed forms of the kinds that have one: the Box and
    ConstantMedium lights' (1, 0, 0), the quadric's unit(-origin), the triangles' unit(origin - p0)."""
    kinds = _light_kinds(name)
    i, r, ref, light = _ctx(name, "lights")
    assert 100 <= int(light.sum()) <= len(r) - 100
    drawn = np.zeros(len(kinds), int)
    for k in np.flatnonzero(light):
        is_light, draw = _draws(i[k])
        assert is_light
        li = draw % len(kinds)
        drawn[li] += 1
        p, d = tuple(r[k, 7:10]), ref[k, 10:13]
        if kinds[li] in CONSTANT_LIGHTS:
            assert _same(d, (1.0, 0.0, 0.0))
        elif kinds[li] == "quadric" and any(c != 0.0 for c in p):
            assert _same(d, S.unit(tuple(-c for c in p)))
        elif kinds[li] == "tri" and p != (1.0, 1.0, -3.0):
            assert _same(d, S.unit((p[0] - 1.0, p[1] - 1.0, p[2] + 3.0)))
    assert (drawn >= 3).all(), drawn
    assert set(np.unique(r[:, 6])) == {0.0, 0.5, 1.0}


def test_rich_families():
    name = "rich"
    I = S.ids(name)
    kinds = _light_kinds(name)
    # BlinnPhong's unit(-r_in + d) with d == r_in: NaN exactly on the light rows that drew a light whose direction
    # is the constant (1, 0, 0). With the normal (1, 0, 0) itself the BSDF branch gets there too: no sample of the lobe
    # about the reflected direction (-1, 0, 0) leaves the surface, and the rejection loop's fallback is the normal
    i, r, ref, light = _ctx(name, "blinn_same")
    n_nan = n_lobe = 0
    for k in range(len(r)):
        is_light, draw = _draws(i[k])
        assert is_light == bool(light[k])
        expect = is_light and kinds[draw % len(kinds)] in CONSTANT_LIGHTS
        got = bool(np.isnan(ref[k]).any())
        assert bool(np.isnan(ref[k, 4:7]).all()) == got
        if is_light or r[k, 10] != 1.0:
            assert got == expect
            n_nan += expect
        else:
            n_lobe += got
    assert 5 <= n_nan <= len(r) - 50 and n_lobe >= 3
    # Perlin: grey and finite wherever floor(p) fits an isize's exact range; beyond it (as_isize saturates, p - i is
    # huge, inf or NaN) the interpolated kinds give NaN, while the unsmoothed lookup (index (4 p) as isize & mask,
    # NaN -> 0) stays finite at every coordinate
    i, r, ref, light = _ctx(name, "perlin_edges")
    with np.errstate(invalid="ignore"):
        small_p = np.abs(r[:, 7:10]).max(axis=1) <= 2.0 ** 31
    lookup = r[:, 17] == I["perlin_none"]
    b = ~light & (small_p | lookup)                        # (BSDF rows: the factor is the texture's colour)
    assert np.isfinite(ref[small_p]).all() and np.isfinite(ref[b, 4:7]).all() and (ref[:, 0] == 1.0).all()
    assert int(np.isnan(ref[~small_p & ~lookup & ~light, 4:7]).any(axis=1).sum()) >= 20
    assert int((lookup & ~small_p & ~light).sum()) >= 15 and int((small_p & ~lookup).sum()) >= 60
    assert (ref[b, 4] == ref[b, 5]).all() and (ref[b, 5] == ref[b, 6]).all() and len(np.unique(ref[b, 4])) >= 20
    # Image: the texel Image::color names -- x = (u w) as u32, y = ((1 - v) h) as u32, both clamped to the last one
    i, r, ref, light = _ctx(name, "image_uv")
    img = S.materials(True)["image"].texture.rgb
    h, w = img.shape[:2]

    def as_u32(x):
        return 0 if not x > 0.0 else (0xffffffff if x >= 4294967295.0 else int(x))

    for k in np.flatnonzero(~light):
        x, y = min(as_u32(r[k, 15] * w), w - 1), min(as_u32((1.0 - r[k, 16]) * h), h - 1)
        texel = (img[y, x].astype(np.float32) / np.float32(255.0)).astype(np.float64)
        assert _same(ref[k, 4:7], texel), (k, r[k, 15:17])
    assert int((~light).sum()) >= 40 and np.isfinite(ref).all()
