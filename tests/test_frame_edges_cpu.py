"""Guards of tests/frame_edges.py's fixtures, on the CPU: the table sizes (so a row cannot be dropped silently), that
each degenerate camera really is degenerate in the way its reason says, and the closed forms that hold exactly on
the oracle's camera sample -- the independent half of tests/test_gpu_frame_edges.py, which only compares the GPU
with this oracle."""
import ctypes as C
import math

import numpy as np
import pytest

import edge_rays as E
import frame_edges as X
from oracle import binding
from raysnail_amd.api import DeviceScene


def _ref(name, centres=False):
    return X.probe_reference(name, centres)


def _same(a, b):
    return np.all(E.bits(np.asarray(a, dtype=np.float64)) == E.bits(np.asarray(b, dtype=np.float64)), axis=-1)


# ------------------------------------------------------------------------------- table sizes ----
def test_table_sizes():
    cams = X.cameras()
    assert len(cams) == 54 == sum(X.FAMILY_SIZES.values())
    for fam, n in X.FAMILY_SIZES.items():
        assert len(X.family(fam)) == n, fam
    assert tuple(X.FAMILY_SIZES) == X.FAMILIES
    assert all(c.reason and "\n" not in c.reason for c in cams)
    assert len(X.FRAME_CAMERAS) == 19 and len(X.SCALED_FRAME_CAMERAS) == 4
    assert {X.camera(n).family for n in X.FRAME_CAMERAS + X.SCALED_FRAME_CAMERAS} == set(X.FAMILIES)
    assert len(X.SHAPES) == 23 and len({s.name for s in X.SHAPES}) == 23
    assert len(X.POISON_NAMES) == 17 and set(X.poison_worlds()) == set(X.POISON_NAMES)
    assert X.WORLDS == tuple(E.SCENES)
    rows = sum(len(X.probe_rows(c)) for c in cams)
    assert rows == 6769 and max(len(X.probe_rows(c)) for c in cams) == 140   # per flag and world


def test_listed_values_are_present():
    """Every value the camera families are to hold, by its bits."""
    def vals(fam, field):
        return [c.fields[field] for c in X.family(fam)]

    def has(seq, v):
        return any(_same(x, v) for x in seq)
    for v in (0.0, -0.0, X.SUBNORMAL, -0.5, 2.0, 1e6, X.INF):
        assert has(vals("lens", "aperture"), v), v
    assert any(math.isnan(v) for v in vals("lens", "aperture"))
    assert X.camera("ap_wide").fields["focus"] == 4.0
    for v in (0.0, -4.0, 1e-300, 1e300, X.INF):
        assert has(vals("focus", "focus"), v), v
    assert {(c.fields["focus"], c.fields["aperture"]) for c in X.family("focus")} >= {(0.0, 0.0), (0.0, 0.5)}
    for v in (0.0, 1e-300, 90.0, 180.0, 270.0, 360.0, -40.0):
        assert has(vals("fov", "fov"), v), v
    assert any(math.isnan(v) for v in vals("fov", "fov"))
    for v in (0.0, -0.0, -1.0, 1e308, X.INF):
        assert has(vals("shutter", "shutter"), v), v
    assert any(math.isnan(v) for v in vals("shutter", "shutter"))
    assert {(c.fields["width"], c.fields["height"]) for c in X.family("frame")} == {(1, 1), (1, 7), (7, 1), (2, 3)}
    assert [c.samples for c in X.family("samples")] == [1, 2, 3, 4, 8]
    assert all(c.fields["width"] <= 7 and c.fields["height"] <= 5 or c.family == "frame" for c in X.cameras())


# ------------------------------------------------------------------------------- shapes ----
def test_shape_table_covers_the_listed_cases():
    S = X.SHAPES
    assert {(s.w, s.h) for s in S} == {(1, 1), (1, 9), (9, 1), (7, 5), (13, 3), (17, 11)}
    assert {s.samples for s in S} == {1, 4, 9, 36, 100, 121}
    assert all(s.samples <= 9 or (s.w <= 7 and s.h <= 5) or (s.w, s.h) == (9, 1) for s in S)
    assert all(s.samples <= 36 or (s.w <= 7 and s.h <= 5) for s in S)
    lattices = {s.rows for s in S}
    assert lattices >= {(0, 0, 1), (1, 0, 2), (2, 0, 3), (0, 0, 4), (3, 0, 7), (1, 0, 8)}
    assert any(s.rows[2] > s.h for s in S)                                             # a step above the height
    assert any(s.rows[1] and (s.rows[1] - s.rows[0]) % s.rows[2] for s in S)           # an end off the lattice
    assert any(len(s.lattice_rows()) == 1 and s.h > 1 for s in S)                      # a lattice of one row
    assert all(len(s.lattice_rows()) >= 1 for s in S)
    assert {s.mask_kind for s in S} == {"none", "zero", "last"}
    assert {s.planes for s in S} >= {0, 1, 3}
    for s in S:
        npl = len(s.lattice_rows()) * s.w
        if s.planes == 3:
            assert math.isqrt(s.samples) ** 2 > 3     # a later batch starts at a nonzero plane
        if s.items:
            assert all(s.items % k for k in range(2, s.items)) and s.items % npl != 0 and s.items > npl


@pytest.mark.parametrize("wname", X.SHAPE_WORLDS)
def test_shape_references(wname):
    """The oracle renders every shape; masked and off-lattice pixels stay zero, the others are lit, and the sample
    count is lattice pixels under the mask times floor(sqrt(samples))^2."""
    for s in X.SHAPES:
        img, (seg, smp) = X.shape_reference(s.name, wname)
        live = np.zeros((s.h, s.w), bool)
        live[s.lattice_rows(), :] = True
        if s.mask() is not None:
            live &= s.mask().astype(bool)
        assert smp == int(live.sum()) * math.isqrt(s.samples) ** 2 and seg >= smp, s.name
        assert np.all(img[~live] == 0.0) and np.all(img[live][:, 3] == 1.0), s.name
        assert np.isfinite(img).all(), s.name


# ------------------------------------------------------------------------------- cameras: closed forms ----
def test_pinhole_origin_is_look_from():
    """aperture +0, -0 and 2^-1074: the lens offset is a zero of either sign, and look_from (no zero component)
    absorbs it bit for bit -- both flags, every row."""
    for name in ("ap_pos0", "ap_neg0", "ap_subnormal"):
        for centres in (False, True):
            r = _ref(name, centres)
            assert _same(r[:, 0:3], np.array(X.BASE["look_from"])).all(), name


def test_focus0_pinhole_directions_are_nan():
    for centres in (False, True):
        r = _ref("focus0_pinhole", centres)
        assert np.isnan(r[:, 3:6]).all() and _same(r[:, 0:3], np.array(X.BASE["look_from"])).all()
        assert np.isfinite(r[:, 6:]).all()


def _w(c):
    f = c.fields
    d = np.array(f["look_at"]) - np.array(f["look_from"])
    return d / np.sqrt(np.dot(d, d))


def test_centre_sample_looks_along_w():
    """The stratum centre of the pixel with u = v = 1 / 2 -- x = (W - 1) / 2 and, because v = (H - 1 - yo) / H,
    y = (H - 3) / 2 of the odd 7 x 5 frame -- at one sample through a pinhole looks along w: each component within one
    ulp of 1 (2^-52; the direction is a unit vector) on the base camera, and exactly on the axis views, where every
    product is exact."""
    x, y = 3, 1
    for name in ("samples_1",) + tuple(c.name for c in X.family("basis") if c.name.startswith("axis_")):
        c = X.camera(name)
        e = X.Entry(c.family, name, c.reason, samples=1, **dict(c.fields, aperture=0.0))
        got = binding.camera_sample(e.desc(), e.settings(), np.array([[x, y, 0]], np.uint32), True)[0]
        w = _w(c)
        assert np.all(np.abs(got[3:6] - w) <= 2.0 ** -52), (name, got[3:6] - w)
        if name.startswith("axis_"):
            assert np.array_equal(got[3:6], w) and abs(got[3:6]).sum() == 1.0, (name, got[3:6])


def _words_after(key: int, n_gen: int):
    """The xorshift128 state after n_gen gen() calls: its last four 32-bit outputs (a gen() is two of them)."""
    lib = binding.load()
    out = (C.c_uint32 * (2 * n_gen))()
    lib.orc_rng_u32(key, 2 * n_gen, out)
    return [float(v) for v in out[-4:]]


def _gens(key: int, n: int):
    lib = binding.load()
    out = (C.c_double * n)()
    lib.orc_rng_gen(key, n, out)
    return list(out)


@pytest.mark.parametrize("name", ["samples_8", "ap_nan", "from_eq_at", "frame_7x1", "shutter_inf"])
def test_rng_advances_by_the_draws_of_the_sample(name):
    """2 jitter draws (none under the centre rule), 2 per lens-disk trial and 1 for the time: the state words after
    the sample are those after exactly 2 + 2k + 1 draws (2k + 1), k the trials up to the first inside the unit disk,
    whatever the camera -- and some row needs more than one trial."""
    c = X.camera(name)
    lib = binding.load()
    rows = X.probe_rows(c)
    ks = []
    for centres in (False, True):
        ref = _ref(name, centres)
        for (x, y, s), r in zip(rows.tolist(), ref):
            key = lib.orc_stream_key(X.SEED, X.PASS, y * c.fields["width"] + x, s)
            g = _gens(key, 64)
            i = 0 if centres else 2
            k = 0
            while True:
                k += 1
                px, py = -1.0 + g[i] * 2.0, -1.0 + g[i + 1] * 2.0
                i += 2
                if px * px + py * py < 1.0:
                    break
            ks.append(k)
            assert list(r[7:11]) == _words_after(key, i + 1), (name, centres, x, y, s, k)
    assert max(ks) > 1


def test_jitter_stays_in_its_stratum():
    """samples 8 gives 2 x 2 strata: the centre rule's directions differ from the jittered ones on every row. The
    centre rule starts the lens draw at the stream's start, so its origin differs too -- unless its first trial falls
    outside the disk: its second trial is then the jittered sample's first."""
    a, b = _ref("samples_8", False), _ref("samples_8", True)
    assert len(a) == 7 * 5 * 4 and not _same(a[:, 3:6], b[:, 3:6]).any()
    same_origin = _same(a[:, 0:3], b[:, 0:3])
    assert 0 < same_origin.sum() < len(a) // 2
    assert _same(_ref("samples_4"), a).all()                 # floor(sqrt(8)) = 2: the same 4 samples
    assert len(_ref("samples_3")) == 35 and _same(_ref("samples_3"), _ref("samples_1")).all()
    assert _same(_ref("samples_2"), _ref("samples_1")).all()


# ------------------------------------------------------------------------------- cameras: each is degenerate as said ----
def _frac_nan(name, cols, centres=False):
    return float(np.isnan(_ref(name, centres)[:, cols]).mean())


def test_lens_family():
    base = _ref("samples_4")
    assert not _same(_ref("ap_negative")[:, 0:3], base[:, 0:3]).any()
    # aperture -0.5 against +0.5: the offsets are mirrored through look_from
    e = X.Entry("lens", "p", "", aperture=0.5)
    pos = binding.camera_sample(e.desc(), e.settings(), X.probe_rows(e), False)
    o = np.array(X.BASE["look_from"])
    assert np.allclose(_ref("ap_negative")[:, 0:3] - o, -(pos[:, 0:3] - o), rtol=0, atol=2.0 ** -50)
    assert np.abs(_ref("ap_wide")[:, 0:3] - o).max() > 0.5
    assert np.abs(_ref("ap_huge")[:, 0:3]).max() > 1e5
    r = _ref("ap_inf")
    assert not np.isfinite(r[:, 0:3]).any() and np.isnan(r[:, 3:6]).all()
    assert _frac_nan("ap_nan", slice(0, 6)) == 1.0
    for name in ("ap_inf", "ap_nan"):
        assert np.isfinite(_ref(name)[:, 6:]).all()          # the time and the RNG words do not depend on the lens


def test_focus_family():
    r = _ref("focus0_lens")
    o = np.array(X.BASE["look_from"])
    assert np.isfinite(r).all()
    # F == O: every ray runs from its lens point back through look_from
    back = o - r[:, 0:3]
    back /= np.linalg.norm(back, axis=1)[:, None]
    assert np.allclose(back, r[:, 3:6], rtol=0, atol=1e-12)
    c = X.camera("focus_negative")
    assert np.all(_ref("focus_negative")[:, 3:6] @ _w(c) < -0.8)        # against w: towards the scene
    assert np.isfinite(_ref("focus_tiny")).all()
    assert _frac_nan("focus_inf", slice(3, 6)) == 1.0 and np.isfinite(_ref("focus_inf")[:, 0:3]).all()
    r = _ref("focus_huge")                                              # len2 = inf, 1 / sqrt = 0: d = dir * 0
    assert np.all(r[:, 3:6] == 0.0) and np.isfinite(r[:, 0:3]).all()


def test_fov_family():
    for centres in (False, True):
        r = _ref("fov0", centres)
        # an empty footprint: lb == the focus point, every pixel aims at it (the lens still moves the origin)
        e = X.Entry("fov", "p", "", fov=0.0, aperture=0.0)
        p = binding.camera_sample(e.desc(), e.settings(), X.probe_rows(e), centres)
        assert _same(p[:, 3:6], p[0, 3:6]).all() and np.isfinite(r).all()
    assert np.isfinite(_ref("fov_tiny")).all()
    assert math.tan(math.radians(90.0) / 2.0) != 1.0
    assert np.isfinite(_ref("fov180")).all() and math.tan(math.pi / 2) > 1e16
    # fov 270 and -40: tan < 0, the image is turned round -- pixel (0, 0)'s direction is the base's (6, 3)'s side
    for name in ("fov270", "fov_negative"):
        c = X.camera(name)
        assert math.tan(math.radians(c.fields["fov"]) / 2.0) < 0.0 and np.isfinite(_ref(name)).all()
    assert abs(math.tan(math.pi)) < 1e-15 and np.isfinite(_ref("fov360")).all()
    assert _frac_nan("fov_nan", slice(3, 6)) == 1.0 and np.isfinite(_ref("fov_nan")[:, 0:3]).all()  # hu, vu: no fov


def test_basis_family():
    for name in ("from_eq_at", "vup_zero", "vup_nan"):
        assert _frac_nan(name, slice(0, 6)) == 1.0, name
    for name in ("vup_plus_w", "vup_minus_w"):
        c = X.camera(name)
        assert np.linalg.norm(np.cross(_w(c), np.array(c.fields["vup"]))) < 2.0 ** -50
        r = _ref(name)
        assert np.isnan(r[:, 0:6]).all() or np.isfinite(r[:, 0:6]).all(), name
    c = X.camera("vup_near_w")
    cr = np.cross(_w(c), np.array(c.fields["vup"]))
    assert 0.0 < np.dot(cr, cr) <= 2.0 ** -51 and np.isfinite(_ref("vup_near_w")).all()
    for c in X.family("basis"):
        if c.name.startswith("axis_"):
            d = np.array(c.fields["look_at"]) - np.array(c.fields["look_from"])
            assert sorted(np.abs(d)) == [0.0, 0.0, 5.0] and np.signbit(d[d == 0.0]).tolist() in ([True, False],
                                                                                             [False, True]), c.name
            assert np.isfinite(_ref(c.name)).all()


def test_scale_family():
    for p in X.SCALE_POWERS:
        c = X.camera(f"scale_{'m' if p < 0 else 'p'}{abs(p)}")
        d = np.array(c.fields["look_at"]) - np.array(c.fields["look_from"])
        assert _same(d, (np.array(X.BASE["look_at"]) - np.array(X.BASE["look_from"])) * math.ldexp(1.0, p)).all()
        with np.errstate(over="ignore", under="ignore"):
            l2 = float(np.dot(d, d))
        if p == -520:
            assert 0.0 < l2 < 2.0 ** -1022 and np.isfinite(_ref(c.name)).all()             # subnormal
        elif p == -540:
            assert l2 == 0.0 and _frac_nan(c.name, slice(0, 6)) == 1.0                       # 0 * inf
        elif p == 500:
            assert np.isfinite(l2) and np.isfinite(_ref(c.name)).all()
        else:
            assert l2 == X.INF and _frac_nan(c.name, slice(0, 6)) == 1.0                     # w = 0: unit(0 x vup)
    # the scaled cameras that stay finite give the base camera's directions (powers of two scale exactly) ...
    assert _same(_ref("scale_p500")[:, 3:], _ref("samples_4")[:, 3:]).all()
    # ... and at 2^53 the origin's x absorbs the lens offset: every origin x is look_from's
    r = _ref("far_2p53")
    assert np.all(r[:, 0] == 2.0 ** 53) and np.isfinite(r).all() and len(np.unique(r[:, 1])) > 100


def test_shutter_family():
    base = _ref("samples_4")
    g = base[:, 6] / 0.5                       # the time draw
    assert np.all((g >= 0.0) & (g < 1.0)) and np.all(g > 0.0)
    for name, fn in (("shutter_pos0", lambda t: _same(t, 0.0)), ("shutter_neg0", lambda t: _same(t, -0.0)),
                     ("shutter_negative", lambda t: _same(t, -g)), ("shutter_huge", lambda t: t > 1e300),
                     ("shutter_inf", lambda t: t == X.INF), ("shutter_nan", np.isnan)):
        r = _ref(name)
        assert np.all(fn(r[:, 6])), name
        assert _same(r[:, 0:6], base[:, 0:6]).all() and _same(r[:, 7:], base[:, 7:]).all(), name
    assert E.world("spheres_moving").time_range == (0.0, 1.0)


def test_frame_family():
    for name, (w, h) in (("frame_1x1", (1, 1)), ("frame_1x7", (1, 7)), ("frame_7x1", (7, 1)), ("frame_2x3", (2, 3))):
        c = X.camera(name)
        assert len(X.probe_rows(c)) == w * h * 4 and np.isfinite(_ref(name)).all()
    # H = 1: v = (1 - 1 - yo) / 1 = -yo is below 0 for every sample -- the direction points below the viewport's
    # lower edge: further from `vup` than the direction of the same u at v = 0
    c = X.camera("frame_7x1")
    e = X.Entry("frame", "p", "", samples=1, **dict(c.fields, aperture=0.0))
    got = binding.camera_sample(e.desc(), e.settings(), X.probe_rows(e), True)
    lib = binding.load()
    out = (C.c_double * 7)()
    for (x, y, s), r in zip(X.probe_rows(e).tolist(), got):
        lib.orc_camera_ray(C.byref(e.desc()), (x + 0.5) / 7.0, 0.0, 1, out)
        assert r[4] < out[4]


# ------------------------------------------------------------------------------- worlds ----
def test_camera_frame_references():
    """Every frame camera renders on the oracle over its worlds; the NaN-direction cameras hit nothing (one
    World::hit per sample) and paint the background's NaN-direction value."""
    for name in X.FRAME_CAMERAS:
        for kind in ("spheres", "nest2"):
            img, (seg, smp) = X.camera_frame_reference(name, X.frame_world_name(name, kind))
            assert smp == img.shape[0] * img.shape[1] * 4 and seg >= smp, name
    for p, name in zip(X.SCALE_POWERS, X.SCALED_FRAME_CAMERAS):
        assert DeviceScene(X.frame_world(f"scaled{p}"), devices=[]).info().scene_mode == 1
        img, (seg, smp) = X.camera_frame_reference(name, f"scaled{p}")
        assert smp == 192 and seg >= smp
    assert X.camera_frame_reference("scale_p500", "scaled500")[1][0] > 192      # the scaled scene is seen
    for name in ("focus0_pinhole", "from_eq_at", "ap_inf"):
        img, (seg, smp) = X.camera_frame_reference(name, "spheres")
        assert seg == smp and _same(img.astype(np.float64), img[0, 0].astype(np.float64)).all()


@pytest.mark.parametrize("wname", X.POISON_NAMES)
def test_poison_worlds(wname):
    """The poisoned worlds commit into the modes they are meant for (no value is refused), and their oracle frames
    hold what they are for: non-finite pixels at depth >= 1, NaN from sqrt of a negative mean with gamma only."""
    w = X.frame_world(wname)
    info = DeviceScene(w, devices=[]).info()
    if wname == "poison_miss":
        assert info.scene_mode == 1
        img, (seg, smp) = X.poison_reference(wname, 2, 1)
        lo = np.array([0.125, 0.25, 0.5], np.float32)
        # a NaN direction's gradient parameter clamps to 0 (f64::max / min ignore the NaN): the background is `lo`
        assert seg == smp and np.array_equal(img[..., :3], np.broadcast_to(np.sqrt(lo), img[..., :3].shape))
        return
    assert info.scene_mode == X.POISON_EXPECT_MODE[wname.split("_")[1]]
    img0, (seg0, smp0) = X.poison_reference(wname, 0, 1)
    assert seg0 == 0 and np.all(img0[..., :3] == 0.0)         # depth 0: no World::hit, a black frame
    for depth in X.POISON_DEPTHS[1:]:
        a, b = X.poison_reference(wname, depth, 0)[0], X.poison_reference(wname, depth, 1)[0]
        assert a.shape == (X.POISON_H, X.POISON_W, 4)
        assert np.isnan(b).sum() >= np.isnan(a).sum()


def test_poison_worlds_reach_their_ends():
    """Over all poisoned worlds the oracle's frames hold +inf, NaN and negative means, and gamma turns negative means
    into NaN; the per-sample radiances hold non-finite channels at depth 1 (a light's own emission or the background)
    and at the deeper limits."""
    seen = {"inf": 0, "nan": 0, "neg": 0, "sqrt_neg": 0}
    for wname in X.POISON_NAMES[:-1]:
        for depth in X.POISON_DEPTHS[1:]:
            a, b = X.poison_reference(wname, depth, 0)[0][..., :3], X.poison_reference(wname, depth, 1)[0][..., :3]
            seen["inf"] += int(np.isinf(a).sum())
            seen["nan"] += int(np.isnan(a).sum())
            seen["neg"] += int((a < 0).sum())
            seen["sqrt_neg"] += int((np.isnan(b) & (a < 0)).sum())
    assert min(seen.values()) > 0, seen
    for wname in ("poison_spheres_0", "poison_spheres_1"):
        for depth in (1, 5):
            s = X.poison_sample_reference(wname, depth)
            assert (~np.isfinite(s[..., :3])).any(), (wname, depth)
            assert s[..., 3].max() <= depth and s[..., 3].min() >= 1


def test_feature_and_sample_references():
    """The restatements evaluate every frame camera (the oracle can evaluate each input, or it would not belong in
    the table): a first-hit frame costs one World::hit per sample, a chain frame at least that, and the per-sample
    radiances sum to the frame's World::hit count."""
    for name in X.FRAME_CAMERAS:
        for kind in ("spheres", "nest2"):
            wname = X.frame_world_name(name, kind)
            a0, n0, calls0 = X.features_reference(name, wname, 0)
            a2, n2, calls2 = X.features_reference(name, wname, 2)
            img, (seg, smp) = X.camera_frame_reference(name, wname)
            assert calls0 == smp <= calls2 and a0.shape == img.shape == a2.shape
            s = X.sample_reference(name, wname)
            assert int(s[..., 3].sum()) == seg, (name, wname)
            assert not X.sample_mismatches(s, s).any()
    # the criterion itself: a flipped class, a moved NaN and a last-bit difference
    s = np.array([[1.0, X.INF, X.NAN, 3.0]])
    assert X.sample_mismatches(np.array([[1.0, -X.INF, X.NAN, 3.0]]), s).all()
    assert X.sample_mismatches(np.array([[1.0, X.NAN, X.INF, 3.0]]), s).all()
    assert X.sample_mismatches(np.array([[1.0, X.INF, X.NAN, 4.0]]), s).all()
    assert not X.sample_mismatches(np.array([[1.0 + 2.0 ** -41, X.INF, X.NAN, 3.0]]), s).any()
    assert X.sample_mismatches(np.array([[1.0 + 2.0 ** -39, X.INF, X.NAN, 3.0]]), s).all()
