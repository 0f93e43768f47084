"""Guards of tests/edge_rays.py's fixtures, on the CPU: the scenes commit into the modes they are meant for, the
oracle is well defined on every ray (no NaN), every (scene, family, tmin) cell both hits and misses, and the
near-first scenes hold enough exact ties -- so that tests/test_gpu_edge_rays.py cannot go vacuous."""
import numpy as np
import pytest

import edge_rays as E
from raysnail_amd.api import DeviceScene


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_scene_modes(name):
    inf = DeviceScene(E.world(name), devices=[]).info()
    mode, arity, ref_order = E.EXPECT_INFO[name]
    assert inf.scene_mode == mode
    assert inf.ref_order == ref_order
    if arity is not None:
        assert inf.tree_arity == arity


def test_ray_families():
    assert len(E.d_axis()) == 56 and len(E.d_scaled()) == 168 and len(E.d_near()) == 240
    near = np.abs(E.d_near())
    assert (near > 0.0).all()                                   # no zero left
    assert (near[near < 1.0] < 2.0 ** -29).all()
    assert (near == 2.0 ** -1074).any() and (near == 2.0 ** -200).any()
    with np.errstate(divide="ignore", over="ignore"):
        assert np.isinf(1.0 / near[near < 2.0 ** -1023]).all()  # the subnormal components: 1 / d overflows
    for name in E.SCENES:
        r, fam, twins = E.rays(name)
        assert 8000 <= len(r) * len(E.TMINS) <= 15000
        d = r[:, 3:6]
        assert np.isfinite(r).all() and np.all(np.any(d != 0.0, axis=1))
        assert set(np.unique(r[:, :3])) <= set(np.arange(-3.0, 3.25, 0.5))
        a, b = r[twins[:, 0]], r[twins[:, 1]]
        assert np.array_equal(a, b) and not np.array_equal(E.bits(a), E.bits(b))  # equal up to the sign of zero
        assert np.array_equal(np.signbit(a[:, 3:6]) != np.signbit(b[:, 3:6]), a[:, 3:6] == 0.0)
        assert len(twins) >= 1000
        times = set(np.unique(r[:, 6]))
        assert times == (set(E.MOVING_TIMES) if name == "spheres_moving" else {0.0})


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_oracle_defined_and_cells_mixed(name):
    _, fam, _ = E.rays(name)
    for tmin in E.TMINS:
        ref = E.reference(name, tmin)
        assert not np.isnan(ref).any()
        assert set(np.unique(ref[:, 0])) == {0.0, 1.0}
        hit = ref[:, 0] == 1.0
        assert np.isfinite(ref[hit, 1]).all() and (ref[hit, 1] >= tmin).all()
        for f, fname in enumerate(E.FAMILIES):
            frac = float(np.mean(hit[fam == f]))
            assert 0.15 <= frac <= 0.85, (name, fname, tmin, frac)


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_oracle_signed_zero_twins(name):
    """A direction's +0 components and their -0 twins give the same oracle record, bit for bit -- except where the
    record's own t1 is a zero (tmin = 0, the origin on the surface): its sign follows the direction's."""
    _, _, twins = E.rays(name)
    for tmin in E.TMINS:
        ref = E.reference(name, tmin)
        a, b = ref[twins[:, 0]], ref[twins[:, 1]]
        differ = np.any(E.bits(a) != E.bits(b), axis=1)
        assert np.array_equal(a[differ], b[differ])            # equal as numbers: only signs of zeros differ
        assert (a[differ, 1] == 0.0).all()
        if tmin > 0.0:
            assert not differ.any()


def test_slanted_mesh_hits_at_infinity():
    """The one fixture with NaNs, kept apart: lattice rays parallel to a 45-degree triangle get a hit at t1 = +inf
    with a NaN point from the oracle (Triangle::hit's closed range end)."""
    inf = DeviceScene(E.world("slanted"), devices=[]).info()
    assert inf.scene_mode == 2 and inf.ref_order == 0
    n = 0
    for tmin in E.TMINS:
        ref = E.reference("slanted", tmin)
        at_inf = (ref[:, 0] == 1.0) & (ref[:, 1] == np.inf)
        assert np.array_equal(at_inf, np.isnan(ref).any(axis=1))
        assert np.isnan(ref[at_inf, 3:9]).any(axis=1).all()
        n += int(at_inf.sum())
    assert n >= 20, n


@pytest.mark.parametrize("name", ["spheres", "flat"])
def test_ties(name):
    """Exact ties between objects, found with single-object oracle worlds: enough of them, enough with records that
    differ between the tied objects, and the oracle's own record always one tied object's."""
    n_tie = n_differ = n_rects = 0
    for tmin in E.TMINS:
        ref = E.reference(name, tmin)
        tied, recs = E.ties(name, tmin)
        if name == "flat":
            a, b = E.coplanar_rects(name)
            n_rects += int((tied[a] & tied[b]).sum())
        hit = ref[:, 0] == 1.0
        count = tied.sum(axis=0)
        assert (count[hit] >= 1).all() and (count[~hit] == 0).all()
        assert E.matches_a_tied_object(ref, tied, recs)[hit].all()
        for i in np.flatnonzero(count >= 2):
            b = E.bits(recs[tied[:, i], i, 1:12])
            n_tie += 1
            n_differ += int(np.any(b != b[0]))
    print(f"{name}: {n_tie} tie rays, {n_differ} with differing tied records")
    assert n_tie >= 300 and n_differ >= 100, (n_tie, n_differ)
    if name == "flat":  # the coplanar rects' overlap is among them
        assert n_rects >= 100, n_rects


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_nonfinite_family(name):
    """The non-finite rays, apart from rays(): every ray has a NaN or an infinity, every kind is there, and the
    oracle is defined on them -- a NaN or an infinite direction component alone never hits (every object's t is NaN,
    or the root box's range is empty), while a NaN origin coordinate or a single NaN direction component does hit
    rects, boxes and triangles' planes wherever the scene has them, with NaNs in the record."""
    r, kind = E.nonfinite_rays(name)
    assert not np.isfinite(r).all(axis=1).any() and np.isfinite(E.rays(name)[0]).all()
    assert [int((kind == k).sum()) for k in range(len(E.NONFINITE_KINDS))] == [60, 180, 240, 200]
    d = r[:, 3:6]
    assert np.isnan(d[kind == 0]).all() and np.isfinite(r[kind == 0, :3]).all()
    assert np.isinf(d[kind == 2]).any(axis=1).all() and not np.isnan(r[kind == 2]).any()
    assert (np.isnan(d[kind == 3]).sum(axis=1) == 1).all()
    for tmin in E.TMINS:
        ref = E.nonfinite_reference(name, tmin)
        assert set(np.unique(ref[:, 0])) <= {0.0, 1.0}
        assert (ref[(kind == 0) | (kind == 2), 0] == 0.0).all()
        hits = (ref[:, 0] == 1.0) & ((kind == 1) | (kind == 3))
        if name in ("spheres", "spheres_moving"):
            assert not hits.any()
        else:
            assert int(hits.sum()) >= 40 and np.isnan(ref[hits, 3:6]).any(axis=1).all()
            if name != "rich":                                  # (a ConstantMedium's t1 can itself be NaN)
                assert np.isfinite(ref[hits, 1]).all()
