"""Both ends of a path and the frame around it on the GPU against the oracle, on tests/frame_edges.py's tables.

The camera sample: rs_probe_camera runs each scene mode's own compile of camera_sample_xy / camera_ray (and the
feature kernels' stratum-centre rule) on every pixel and sample of 54 degenerate cameras; all 11 outputs -- origin,
direction, time and the four RNG words after the sample, so a missing or an extra draw fails -- are orc_camera_sample's.
A subset of the cameras is then rendered through every consumer of camera_ray: rs_render in megakernel, wavefront and
auto mode, rs_render_features, rs_render_features_specular and rs_probe_samples.

Frame shapes: frames narrower and lower than a tile of the sample order, one column, one row, row lattices with every
tile-shape class of steps, masks, plane counts up to 121 and batches of one plane, three planes and a prime number of
items, equal to the oracle with equal World::hit counts.

The path's far end: worlds with +inf, NaN, negative and zero albedos, light colours, multipliers and backgrounds at
depth 0, 1, 2 and 5 with and without gamma -- close_path at absorption and at the depth limit with a non-finite
throughput, the miss branch, sqrt of negative means, non-finite sums through the accumulation over several batches.

Everything is compared bit for bit; NaNs have no portable bit pattern and are compared by position. No tolerance but
rs_probe_samples' own documented one, no excluded rows. tests/test_frame_edges_cpu.py guards the fixtures."""
import ctypes as C

import numpy as np
import pytest

import frame_edges as X
from raysnail_amd import _abi as A

pytestmark = pytest.mark.gpu

MODES = {"mega": A.RS_MODE_MEGAKERNEL, "wavefront": A.RS_MODE_WAVEFRONT, "auto": A.RS_MODE_AUTO}
DEFAULT_BATCH_ITEMS = 32 << 20   # rs_scene_set_workspace's default (rs_host.cpp max_items_per_batch)


# ------------------------------------------------------------------------------- the camera probe ----
def _probe(ds, entry, centres):
    rows = X.probe_rows(entry)
    out = np.full((len(rows), 11), -7.0)
    d, st = entry.desc(), entry.settings()
    rc = ds.lib.rs_probe_camera(ds.handle, C.byref(d), C.byref(st), rows.ctypes.data, len(rows), int(centres),
                                out.ctypes.data)
    assert rc == 0, ds.lib.rs_last_error()
    return rows, out


@pytest.mark.parametrize("fam", X.FAMILIES)
@pytest.mark.parametrize("wname", X.WORLDS)
def test_camera_sample_exact(gpu, wname, fam):
    """Every camera of the family, every pixel, every sample, both sampling rules, through the scene mode's own
    instantiation of k_probe_camera: all 11 outputs are the oracle's."""
    ds = X.frame_world(wname).device_scene()
    assert ds.info().scene_mode == X.E.EXPECT_INFO[wname][0]
    n = 0
    for entry in X.family(fam):
        for centres in (False, True):
            rows, got = _probe(ds, entry, centres)
            ref = X.probe_reference(entry.name, centres)
            bad = X.differing(got, ref)
            i = np.flatnonzero(bad.any(axis=1))
            assert len(i) == 0, (entry.name, entry.reason, centres, len(i), len(rows), rows[i[0]].tolist(),
                                 [X.FIELDS[k] for k in np.flatnonzero(bad[i[0]])], got[i[0]].tolist(), ref[i[0]].tolist())
            n += len(rows)
    print(f"{wname} / {fam}: {n} rows equal")


def test_camera_probe_checks_its_arguments(gpu):
    ds = X.frame_world("spheres").device_scene()
    e = X.camera("samples_4")
    d, st = e.desc(), e.settings()
    out = np.zeros((2, 11))

    def call(rows, n=2, cam=d, sett=st, o=out):
        rows = np.array(rows, np.uint32)
        return ds.lib.rs_probe_camera(ds.handle, C.byref(cam) if cam is not None else None,
                                      C.byref(sett) if sett is not None else None, rows.ctypes.data, n, 0,
                                      o.ctypes.data if o is not None else None)
    assert call([[0, 0, 0], [6, 4, 3]]) == 0
    assert call([[0, 0, 0], [7, 4, 3]]) == A.RS_E_INVALID        # x outside the frame
    assert call([[0, 0, 0], [6, 5, 3]]) == A.RS_E_INVALID        # y outside
    assert call([[0, 0, 0], [6, 4, 4]]) == A.RS_E_INVALID        # sample beyond floor(sqrt(samples))^2
    assert call([[0, 0, 0], [0, 0, 0]], cam=None) == A.RS_E_INVALID
    assert call([[0, 0, 0], [0, 0, 0]], sett=None) == A.RS_E_INVALID
    assert call([[0, 0, 0], [0, 0, 0]], o=None) == A.RS_E_INVALID
    assert ds.lib.rs_probe_camera(ds.handle, C.byref(d), C.byref(st), None, 0, 0, out.ctypes.data) == A.RS_E_INVALID
    empty = X.camera("samples_4").desc()
    empty.width = 0
    assert call([[0, 0, 0], [0, 0, 0]], cam=empty) == A.RS_E_INVALID


# ------------------------------------------------------------------------------- camera frames ----
def _frame_mismatch(img, ref):
    bad = X.differing32(img, ref).any(axis=-1)
    return int(bad.sum()), [(int(y), int(x), img[y, x].tolist(), ref[y, x].tolist()) for y, x in np.argwhere(bad)[:3]]


def _render_and_compare(ds, d, st, ref, segs, mask=None, times=1, what=None, collect=None):
    """The frame and the World::hit count are the oracle's (and, without a mask, the sample count: under a mask
    rs_render_stats.samples counts the lattice's samples, masked or not). collect: a list that takes the mismatches
    instead of an assertion, so that a caller can report every mode."""
    for k in range(times):
        out = np.zeros((d.height, d.width, 4), np.float32)
        img, stats = ds.render(d, st, mask, out=out)
        n, where = _frame_mismatch(img, ref)
        got = (stats.segments, stats.samples if mask is None else segs[1])
        if collect is not None:
            if n or got != segs:
                collect.append((what, k, f"{n} of {d.width * d.height} pixels differ", where[:1], got, segs))
            continue
        assert n == 0, (what, k, n, where)
        assert got == segs, (what, k, got, segs)


def _camera_frames(name, wname, times):
    e = X.camera(name)
    ds = X.frame_world(wname).device_scene()
    ref, segs = X.camera_frame_reference(name, wname)
    bad = []
    for mode_name, mode in MODES.items():
        _render_and_compare(ds, X.frame_desc(name), e.settings(mode=mode), ref, segs, times=times,
                            what=(name, wname, mode_name), collect=bad)
    assert not bad, (e.reason, len(bad), bad[::times])


@pytest.mark.parametrize("kind", ["spheres", "nest2"])
@pytest.mark.parametrize("name", X.FRAME_CAMERAS)
def test_camera_frames(gpu, name, kind):
    """8 x 6, 4 spp, depth 4 through the megakernel, the wavefront and the auto mode: the frame and the World::hit
    count are the oracle's. A spheres-world frame is rendered four times per mode, so the fourth runs on the first
    one's frame slot with the candidate records that frame built (test_gpu_cam_candidates.py).

    shutter_inf is the case that found a bug: with every time inf, Sphere::center_at (sphere.rs:50-52, center +
    speed * t) gives a sphere without speed the centre c + 0 * inf = NaN and the reference misses every sphere, while
    the traversal took c + 0 * t for c at every t (sphere_t_trav) and a static scene's path records dropped the time
    (WfState::tagw): 43 of 48 pixels differed over spheres_moving (465 World::hit calls against 192) and 28 of 48 over
    nest2, in the wavefront and the auto mode. Fixed in ray_consts and tag_in_ray."""
    _camera_frames(name, X.frame_world_name(name, kind), 4 if kind == "spheres" else 1)


@pytest.mark.parametrize("name,p", list(zip(X.SCALED_FRAME_CAMERAS, X.SCALE_POWERS)))
def test_scaled_camera_frames(gpu, name, p):
    """The camera and the spheres world multiplied by 2^p together: len2 under- and overflows on both sides alike."""
    _camera_frames(name, f"scaled{p}", 4)


@pytest.mark.parametrize("kind", ["spheres", "nest2"])
@pytest.mark.parametrize("name", X.FRAME_CAMERAS)
def test_camera_feature_frames(gpu, name, kind):
    """The same cameras through k_features and k_features_spec (max_specular 2): all 8 channels of every pixel are
    the restatements' (features_ref.py, spec_features_ref.py), and so is the World::hit count."""
    wname = X.frame_world_name(name, kind)
    ds = X.frame_world(wname).device_scene()
    d, st = X.frame_desc(name), X.camera(name).settings()
    for m in (0, 2):
        exp_a, exp_n, calls = X.features_reference(name, wname, m)
        got_a, got_n, stats = ds.render_features(d, st, max_specular=m)
        for what, got, exp in (("albedo", got_a, exp_a), ("normal", got_n, exp_n)):
            n, where = _frame_mismatch(got, exp)
            assert n == 0, (name, wname, m, what, n, where)
        assert stats.segments == calls, (name, wname, m, stats.segments, calls)


def _probe_samples(ds, d, st, n):
    got = np.zeros((d.height, d.width, n, 4))
    for y in range(d.height):
        for x in range(d.width):
            g = np.full((n, 4), -7.0)
            assert ds.lib.rs_probe_samples(ds.handle, C.byref(d), C.byref(st), x, y, 0, n, g.ctypes.data) == 0, \
                ds.lib.rs_last_error()
            got[y, x] = g
    return got


@pytest.mark.parametrize("kind", ["spheres", "nest2"])
@pytest.mark.parametrize("name", X.FRAME_CAMERAS)
def test_camera_per_sample_radiance(gpu, name, kind):
    """The same cameras through k_probe_sample, every sample of every pixel, under the probe's documented criterion
    (frame_edges.sample_mismatches)."""
    wname = X.frame_world_name(name, kind)
    ds = X.frame_world(wname).device_scene()
    d, st = X.frame_desc(name), X.camera(name).settings()
    ref = X.sample_reference(name, wname)
    got = _probe_samples(ds, d, st, ref.shape[2])
    bad = np.argwhere(X.sample_mismatches(got, ref))
    assert len(bad) == 0, (name, wname, len(bad), [(tuple(i), got[tuple(i)].tolist(), ref[tuple(i)].tolist()) for i in bad[:3]])


# ------------------------------------------------------------------------------- frame shapes ----
@pytest.mark.parametrize("wname", X.SHAPE_WORLDS)
@pytest.mark.parametrize("shape", [s.name for s in X.SHAPES])
def test_frame_shapes(gpu, shape, wname):
    """Depth 3 through the auto mode (the streaming kernels over the spheres world, the bounce-synchronous ones over
    the flat world) and the megakernel: the frame -- zero off the lattice and under the mask -- and the World::hit
    count are the oracle's."""
    s = X.shape(shape)
    ds = X.frame_world(wname).device_scene()
    ref, segs = X.shape_reference(shape, wname)
    try:
        if s.batch_items():
            ds.set_workspace(max_batch_items=s.batch_items())
        for mode_name in ("auto", "mega"):
            _render_and_compare(ds, s.desc(), s.settings(MODES[mode_name]), ref, segs, mask=s.mask(),
                                times=2 if mode_name == "auto" else 1, what=(shape, wname, mode_name))
    finally:
        ds.set_workspace(max_batch_items=DEFAULT_BATCH_ITEMS)


# ------------------------------------------------------------------------------- the path's far end ----
@pytest.mark.parametrize("gamma", [1, 0])
@pytest.mark.parametrize("depth", X.POISON_DEPTHS)
@pytest.mark.parametrize("wname", X.POISON_NAMES[:-1])
def test_poisoned_frames(gpu, wname, depth, gamma):
    """8 x 6, 4 spp in three modes, the auto mode also with one sample plane per batch (non-finite sums through
    k_accumulate across four batches): the frame and the World::hit count are the oracle's. Depth 0 is k_finalize
    over zero radiance; depth 1 ends every path in the launch that generated it."""
    ds = X.frame_world(wname).device_scene()
    assert ds.info().scene_mode == X.POISON_EXPECT_MODE[wname.split("_")[1]]
    c = X.poison_camera()
    ref, segs = X.poison_reference(wname, depth, gamma)
    for mode_name, mode in MODES.items():
        _render_and_compare(ds, c.desc(), c.settings(depth=depth, mode=mode, gamma=gamma), ref, segs,
                            what=(wname, depth, gamma, mode_name))
    try:
        ds.set_workspace(max_batch_items=X.POISON_W * X.POISON_H)
        _render_and_compare(ds, c.desc(), c.settings(depth=depth, gamma=gamma), ref, segs,
                            what=(wname, depth, gamma, "auto, one plane per batch"))
    finally:
        ds.set_workspace(max_batch_items=DEFAULT_BATCH_ITEMS)


@pytest.mark.parametrize("depth", X.POISON_DEPTHS)
@pytest.mark.parametrize("wname", X.POISON_NAMES[:-1])
def test_poisoned_per_sample_radiance(gpu, wname, depth):
    """rs_probe_samples on the same pixels: finite channels within the probe's documented 2^-40, non-finite ones of
    the same class in the same positions, equal World::hit counts."""
    ds = X.frame_world(wname).device_scene()
    c = X.poison_camera()
    ref = X.poison_sample_reference(wname, depth)
    got = _probe_samples(ds, c.desc(), c.settings(depth=depth), X.POISON_SAMPLES)
    bad = np.argwhere(X.sample_mismatches(got, ref))
    assert len(bad) == 0, (wname, depth, len(bad), [(tuple(i), got[tuple(i)].tolist(), ref[tuple(i)].tolist()) for i in bad[:3]])


@pytest.mark.parametrize("gamma", [1, 0])
def test_miss_branch_with_nan_directions(gpu, gamma):
    """The focus-0 pinhole (every direction NaN) over a world whose background differs in lo and hi: every path is
    one miss, and the background of a NaN direction is the oracle's (the clamp ignores the NaN: `lo`)."""
    ds = X.frame_world("poison_miss").device_scene()
    c = X.camera("focus0_pinhole")
    ref, segs = X.poison_reference("poison_miss", 2, gamma)
    for mode_name, mode in MODES.items():
        _render_and_compare(ds, c.desc(X.POISON_W, X.POISON_H),
                            c.settings(samples=X.POISON_SAMPLES, depth=2, mode=mode, gamma=gamma), ref, segs, times=4,
                            what=("poison_miss", gamma, mode_name))
