"""The adaptive pass loop without a GPU: the numpy restatement of its kernels (tests/adaptive_ref.py) against an
independent float64 computation, the loop's invariants on a synthetic frame source, and the quality of the header's
defaults on oracle renders (the four cells of tools/adaptive_quality.py)."""
import numpy as np
import pytest

import adaptive_ref as R
from raysnail_amd import _abi as A

EPS = 2.0 ** -23  # f32 epsilon (twice the unit roundoff: every bound below counts roundings generously)


# ------------------------------------------------------------- restatement against float64 ----
@pytest.fixture(scope="module")
def frames():
    return {size: R.pass_frames(size[0], size[1], 40 + i) for i, size in enumerate([(37, 23), (149, 67)])}


def moments64(frames, gamma):
    """two-pass mean and variance of the mean in float64 over the contributing frames"""
    xs = np.stack([np.asarray(f, np.float64)[..., :3] for f in frames])
    if gamma:
        xs = xs * xs
    take = np.stack([(f[..., 3] != 0) & np.isfinite(f[..., :3]).all(axis=-1) for f in frames])
    n = take.sum(axis=0)
    xs = np.where(take[..., None], xs, 0.0)
    with np.errstate(all="ignore"):
        mu = xs.sum(axis=0) / n[..., None]
        d = np.where(take[..., None], xs - mu, 0.0)
        var = (d * d).sum(axis=0) / (n * (n - 1))[..., None]
    return n, mu, var


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 5, 64])
@pytest.mark.parametrize("size", [(37, 23), (149, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_against_float64(frames, size, k, gamma):
    """Counts exact. Tolerances, from K and the f32 epsilon, with X the largest sample value (3, or 9 when the frames
    are squared): one Welford step rounds d, d / n1 and the sum, each within eps X / 2 of values below X, so after K
    steps the mean is within 2 K eps X of the exact mean (the squaring under gamma adds eps X / 2 per sample, which the
    mean divides down: 2 K eps X covers it). A step's d e is then off by at most (2 K + 2) eps X^2 (both factors carry
    the mean's error, the product and the sum round once more), so M2 is within K (2 K + 2) eps X^2, and the variance
    of the mean within that over n (n - 1)."""
    fs = frames[size][:k]
    acc, m2 = R.moments_update(*R.empty_state(*size), fs, gamma)
    mean, var = R.moments_resolve(acc, m2, gamma)
    n, mu, v = moments64(fs, gamma)
    assert np.array_equal(var[..., 3], n.astype(np.float32)) and np.array_equal(acc[..., 3], n.astype(np.float32))
    X = 9.0 if gamma else 3.0
    lin = R.linear(mean, gamma)
    some = n >= 1
    assert (np.abs(lin[some] - mu[some]) <= 2 * k * EPS * X + (2 * EPS * X if gamma else 0)).all()  # (+ the sqrt and its square)
    two = n >= 2
    bound = (k * (2 * k + 2) * EPS * X * X / (n * (n - 1.0))[two])[..., None]
    assert (np.abs(var[..., :3][two].astype(np.float64) - v[two]) <= bound).all()
    assert (var[..., :3][~two] == 0).all() and (mean[~some] == 0).all() and (mean[..., 3][some] == 1).all()
    h = size[1]
    assert (acc[h - 2, 1] == 0).all() and (m2[h - 2, 1] == 0).all()  # masked in every frame: the empty state


def test_update_in_two_calls_equals_one(frames):
    for size, fs in frames.items():
        for gamma in (0, 1):
            a = R.moments_update(*R.empty_state(*size), fs[:5], gamma)
            b = R.moments_update(*R.moments_update(*R.empty_state(*size), fs[:2], gamma), fs[2:5], gamma)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
            assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# -------------------------------------------------------------------------- loop invariants ----
W, H, MIN_P, MAX_P, TOL, FLOOR = 60, 20, 3, 12, 0.05, 0.1


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_loop_invariants(radius):
    frame, bands = R.synthetic_frame_source(W, H, 11)
    yy, xx = np.mgrid[0:H, 0:W]
    base = ((xx + 2 * yy) % 7 != 0).astype(np.uint8)
    acc, m2, reports = R.render_adaptive(frame, W, H, 0, MIN_P, MAX_P, TOL, FLOOR, radius, base=base)
    n = acc[..., 3]
    hot, opened, _, _, _ = R.hot_map(acc, m2, base, MIN_P, MAX_P, TOL, FLOOR)
    mask, stats = R.adaptive_mask(acc, m2, base, MIN_P, MAX_P, TOL, FLOOR, radius)
    assert stats["active"] == 0 and not mask.any()
    near_hot = R.dilate(hot, radius)
    on = base != 0
    assert ((n[on] == MAX_P) | ~near_hot[on]).all()
    assert (acc[~on] == 0).all() and (m2[~on] == 0).all()  # no pixel with base == 0 has n > 0
    assert n.max() <= len(reports) <= MAX_P
    # the noise-free band, away from the next band's dilation, stops at exactly min_passes
    quiet = on & (bands[None, :] == 0) & (xx < W // 3 - radius)
    assert quiet.any() and (n[quiet] == MIN_P).all()
    # the loud band runs to max_passes, the middle one stops in between somewhere
    loud = on & (bands[None, :] == 2)
    assert (n[loud] == MAX_P).mean() > 0.9
    assert reports[0]["active"] == int(on.sum()) and reports[0]["hot"] == int(on.sum())
    for r in reports:
        assert r["active"] == int(r["mask"].sum()) and (r["mask"][~on] == 0).all()


def test_masks_of_two_radii_differ_exactly_by_the_dilation():
    frame, _ = R.synthetic_frame_source(W, H, 12)
    state = R.moments_update(*R.empty_state(W, H), [frame(p) for p in range(4)], 0)
    state[0][5, 50, 3] = MAX_P  # a finished pixel inside a hot neighbourhood (the loud band)
    m0, s0 = R.adaptive_mask(*state, None, MIN_P, MAX_P, TOL, FLOOR, 0)
    m2, s2 = R.adaptive_mask(*state, None, MIN_P, MAX_P, TOL, FLOOR, 2)
    hot, opened, _, _, _ = R.hot_map(*state, None, MIN_P, MAX_P, TOL, FLOOR)
    assert np.array_equal(m0 != 0, hot) and s0["hot"] == s2["hot"] == s0["active"]
    assert np.array_equal(m2 != 0, opened & R.dilate(m0 != 0, 2))
    assert 0 < s0["active"] < s2["active"] < W * H and m2[5, 50] == 0 and R.dilate(hot, 2)[5, 50]


# ---------------------------------------------------------------------------------- quality ----
def test_defaults_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "raysnail_adaptive.h")).read()
    got = {k: float(v) for k, v in re.findall(r"#define RS_ADAPTIVE_(\w+)\s+\(\((?:uint32_t|float)\)([\d.e-]+)\)", text)}
    assert got == dict(MIN_PASSES=A.RS_ADAPTIVE_MIN_PASSES, MAX_PASSES=A.RS_ADAPTIVE_MAX_PASSES,
                       RADIUS=A.RS_ADAPTIVE_RADIUS, TOLERANCE=A.RS_ADAPTIVE_TOLERANCE, FLOOR=A.RS_ADAPTIVE_FLOOR)


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("name", R.QUALITY_SCENES)
def test_quality_with_the_defaults(name, gamma):
    """tools/adaptive_quality.py's cell with the header's defaults: the adaptive mean is strictly closer to the 1024-spp
    frame, in the relative metric the criterion targets, than the uniform mean of ceil(total / (W H)) passes, which
    spends at least as many samples; and at least half the pixels stop before max passes
    (profiles/adaptive/quality.txt: the smallest margin of the four cells is +0.0945, rtiow gamma 0)."""
    passes, ref = R.quality_inputs(name, gamma)
    q = R.quality_cell(passes, ref, gamma, A.RS_ADAPTIVE_MIN_PASSES, A.RS_ADAPTIVE_TOLERANCE, A.RS_ADAPTIVE_FLOOR,
                       A.RS_ADAPTIVE_RADIUS, A.RS_ADAPTIVE_MAX_PASSES)
    print(name, gamma, q)
    assert q["uniform_passes"] * R.QUALITY_W * R.QUALITY_H >= q["total"]
    assert q["early"] >= 0.5
    assert q["rel"] < q["rel_uniform"]
