"""rs_moments_update, rs_moments_resolve, rs_adaptive_mask and rs_render_adaptive's loop restated in numpy float32 from
their contracts in include/raysnail_adaptive.h: loops over frames and window offsets, vectorised over pixels, every
intermediate an np.float32 (array), every operation rounded once, in the header's order. And the seeded frames, states
and quality inputs the tests and tools/adaptive_quality.py share."""
import math

import numpy as np

F = np.float32


# ------------------------------------------------------------------------------------ kernels ----
def empty_state(w, h):
    return np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)


def moments_update(acc, m2, frames, gamma=1):
    """the (acc, m2) rs_moments_update_device leaves (new arrays; the inputs are not modified)"""
    assert 1 <= len(frames) <= 64 and gamma in (0, 1)
    acc = np.array(acc, F)
    m2 = np.array(m2, F)
    mu, n, M2 = acc[..., 0:3].copy(), acc[..., 3].copy(), m2[..., 0:3].copy()
    any_take = np.zeros(n.shape, bool)
    with np.errstate(all="ignore"):
        for f in frames:
            f = np.ascontiguousarray(f, F)
            take = (f[..., 3] != 0) & np.isfinite(f[..., 0:3]).all(axis=-1)
            x = f[..., 0:3]
            if gamma:
                x = x * x
            n1 = n + F(1.0)
            d = x - mu
            mu1 = mu + d / n1[..., None]
            e = x - mu1
            M21 = M2 + d * e
            t3 = take[..., None]
            mu = np.where(t3, mu1, mu)
            M2 = np.where(t3, M21, M2)
            n = np.where(take, n1, n)
            any_take |= take
    out_acc, out_m2 = acc.copy(), m2.copy()
    out_acc[..., 0:3] = mu
    out_acc[..., 3] = n
    out_m2[..., 0:3] = M2
    out_m2[..., 3] = np.where(any_take, F(0.0), m2[..., 3])  # (a pixel no frame contributes to is not written)
    return out_acc, out_m2


def moments_resolve(acc, m2, gamma=1):
    """(mean, var) frames rs_moments_resolve_device writes"""
    acc, m2 = np.ascontiguousarray(acc, F), np.ascontiguousarray(m2, F)
    n = acc[..., 3]
    with np.errstate(all="ignore"):
        m = np.sqrt(acc[..., 0:3]) if gamma else acc[..., 0:3]
        den = n * (n - F(1.0))
        v = m2[..., 0:3] / den[..., None]
    mean = np.zeros(acc.shape, F)
    mean[..., 0:3] = np.where((n >= 1)[..., None], m, F(0.0))
    mean[..., 3] = np.where(n >= 1, F(1.0), F(0.0))
    var = np.zeros(acc.shape, F)
    var[..., 0:3] = np.where((n >= 2)[..., None], v, F(0.0))
    var[..., 3] = n
    return mean, var


def hot_map(acc, m2, base, min_n, max_n, tolerance, floor):
    """(hot, open, fin, err2, counted): hot(q); open(q) = base != 0 and n < max_n; fin(q); err2(q) where it is read
    (0 elsewhere); counted = the pixels max_err2 ranges over"""
    acc, m2 = np.ascontiguousarray(acc, F), np.ascontiguousarray(m2, F)
    tol2 = F(tolerance) * F(tolerance)
    n = acc[..., 3]
    based = np.ones(n.shape, bool) if base is None else (np.asarray(base).reshape(n.shape) != 0)
    fin = np.isfinite(acc[..., 0:3]).all(axis=-1) & np.isfinite(m2[..., 0:3]).all(axis=-1)
    with np.errstate(all="ignore"):
        t = (m2[..., 0] + m2[..., 1]) + m2[..., 2]
        v = t / (n * (n - F(1.0)))
        L = (acc[..., 0] + acc[..., 1]) + acc[..., 2]
        Dn = np.maximum(L, F(floor))
        err2 = v / (Dn * Dn)
        opened = based & (n < F(max_n))
        hot = opened & ((n < F(min_n)) | (fin & (err2 > tol2)))
        counted = based & fin & (n >= F(2.0)) & (err2 > F(0.0))
    return hot, opened, fin, np.where(counted, err2, F(0.0)).astype(F), counted


def dilate(hot, radius):
    """some q with |dx|, |dy| <= radius inside the frame has hot(q)"""
    h, w = hot.shape
    pad = np.zeros((h + 2 * radius, w + 2 * radius), bool)
    pad[radius:radius + h, radius:radius + w] = hot
    out = np.zeros((h, w), bool)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


def adaptive_mask(acc, m2, base, min_n, max_n, tolerance, floor, radius):
    """(mask (H, W) uint8, stats dict) of rs_adaptive_mask_device"""
    hot, opened, fin, err2, counted = hot_map(acc, m2, base, min_n, max_n, tolerance, floor)
    mask = (opened & dilate(hot, radius)).astype(np.uint8)
    based = np.ones(hot.shape, bool) if base is None else (np.asarray(base).reshape(hot.shape) != 0)
    stats = dict(active=int(mask.sum()), hot=int(hot.sum()), nonfinite=int((based & ~fin).sum()),
                 max_err2=F(err2.max()) if counted.any() else F(0.0))
    return mask, stats


# --------------------------------------------------------------------------------------- loop ----
def lattice_base(w, h, base, rows):
    """the base mask with the rows off the render's lattice rows = (begin, end or 0 = h, step) switched off"""
    begin, end, step = rows
    end, step = (min(end, h) if end else h), max(step, 1)
    on = np.zeros((h, w), bool)
    on[begin:end:step] = True
    return (on if base is None else on & (np.asarray(base).reshape(h, w) != 0)).astype(np.uint8)


def render_adaptive(frame, w, h, gamma, min_passes, max_passes, tolerance, floor, radius, base=None, state=None,
                    rows=None):
    """rs_render_adaptive_device's loop. frame(p) returns the full (maskless) frame of this call's p-th pass; the mask is
    applied here (an unmasked pixel of a masked render is bit for bit the maskless frame's pixel). Returns (acc, m2,
    reports): one dict(active, hot, max_err2, mask) per rendered pass."""
    acc, m2 = empty_state(w, h) if state is None else (np.array(state[0], F), np.array(state[1], F))
    if rows is not None:  # the render settings' row lattice is part of the base mask
        base = lattice_base(w, h, base, rows)
    reports = []
    p = 0
    while True:
        mask, stats = adaptive_mask(acc, m2, base, min_passes, max_passes, tolerance, floor, radius)
        if stats["active"] == 0 or p == max_passes:
            break
        f = np.where((mask != 0)[..., None], np.ascontiguousarray(frame(p), F), F(0.0)).astype(F)
        acc, m2 = moments_update(acc, m2, [f], gamma)
        reports.append(dict(stats, mask=mask))
        p += 1
    return acc, m2, reports


# ------------------------------------------------------------------------------ shared frames ----
def pass_frames(w, h, seed):
    """test_gpu_denoise_var.py's seeded pass-frame recipe: 64 frames; frame k masked on a checkerboard for odd k (loud
    values under alpha 0 for k % 4 == 1); one NaN pixel in frame 2 at a tile edge (x = 63 | w - 1: the last column of a
    64-wide tile or of the frame; y = 3), one Inf pixel in frame 0 at x = min(64, w - 2) (the first column of
    the second 64-wide tile, or the frame's last but one) and (added here) a -Inf pixel in frame 4 in the frame's last
    column, one pixel masked in all frames. Read-only."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (xx + yy) % 2 == 1
    frames = []
    for k in range(64):
        f = np.ones((h, w, 4), F)
        f[..., :3] = rng.random((h, w, 3), dtype=F) * F(3.0)
        if k % 2 == 1:
            f[board] = [5.0, 5.0, 5.0, 0.0] if k % 4 == 1 else 0.0
        f[h - 2, 1] = 0.0
        frames.append(f)
    nx = 63 if w > 64 else w - 1
    frames[2][3, nx, 1] = np.array([0x7FC00321], np.uint32).view(F)[0]
    frames[0][4, min(64, w - 2), 0] = np.inf
    frames[4][5, w - 1, 2] = -np.inf  # (the frame's last column at either size)
    for f in frames:
        f.setflags(write=False)
    return frames


def synthetic_frame_source(w, h, seed, sigmas=(0.0, 0.02, 0.6)):
    """frame(p) for the loop tests: a constant image of level 0.5 plus seeded Gaussian noise whose sigma is constant over
    each of len(sigmas) vertical bands (the first band is noise-free); linear (gamma 0), alpha 1. The same p gives the
    same frame."""
    bands = np.minimum((np.arange(w) * len(sigmas)) // w, len(sigmas) - 1)
    sigma = np.asarray(sigmas, np.float64)[bands][None, :, None]

    def frame(p):
        rng = np.random.default_rng([seed, p])
        f = np.ones((h, w, 4), F)
        f[..., :3] = (0.5 + sigma * rng.standard_normal((h, w, 3))).astype(F)
        return f
    return frame, bands


# ------------------------------------------------------------------------------ quality inputs ----
QUALITY_W, QUALITY_H, QUALITY_SPP, QUALITY_MAX_PASSES = 64, 40, 4, 32
QUALITY_SCENES = ("rtiow", "features")


def quality_inputs(name, gamma):
    """oracle renders of denoise_var_ref.quality_inputs' scene `name` at 64 x 40, depth 8: (the 32 pass frames of 4 spp
    at seed 1, pass k; the 1024-spp frame at seed 2), both with this gamma"""
    from oracle.binding import OracleScene
    from raysnail_amd import scenes
    if name == "rtiow":
        cam, world, _, _ = scenes.rtow_13_1(QUALITY_W, QUALITY_H, seed=7)
    else:
        cam, world = scenes.features_scene(QUALITY_W, QUALITY_H)
    orc = OracleScene(world)
    hi = cam.take_photo().samples(1024).depth(8).seed(2).gamma(bool(gamma))
    ref = orc.render(cam.desc, hi.settings(), threads=8)[0]
    passes = [orc.render(cam.desc, cam.take_photo().samples(QUALITY_SPP).depth(8).seed(1).gamma(bool(gamma))
                         .pass_index(k).settings(), threads=8)[0] for k in range(QUALITY_MAX_PASSES)]
    return passes, ref


def linear(frame, gamma):
    x = np.asarray(frame, np.float64)[..., :3]
    return x * x if gamma else x


def rmse(mean, ref, gamma):
    """plain RMSE over linear rgb"""
    e = linear(mean, gamma) - linear(ref, gamma)
    return math.sqrt(float(np.mean(e * e)))


def rel_error(mean, ref, gamma, floor):
    """the relative error the criterion targets: the root mean of |x - ref|^2 / max(L_ref, floor)^2 over pixels, with
    |.|^2 summed over rgb and L_ref = ref's channel sum, all in linear radiance"""
    x, r = linear(mean, gamma), linear(ref, gamma)
    e2 = ((x - r) ** 2).sum(axis=-1)
    den = np.maximum(r.sum(axis=-1), floor)
    return math.sqrt(float(np.mean(e2 / (den * den))))


def quality_cell(passes, ref, gamma, min_passes, tolerance, floor, radius, max_passes=QUALITY_MAX_PASSES):
    """one cell of the quality grid: dict(total pass-pixels, uniform passes = ceil(total / (W H)), the adaptive and the
    uniform mean's rmse and relative error, the share of pixels that stopped before max_passes)"""
    h, w = ref.shape[:2]
    acc, m2, reports = render_adaptive(lambda p: passes[p], w, h, gamma, min_passes, max_passes, tolerance, floor, radius)
    mean, var = moments_resolve(acc, m2, gamma)
    total = int(sum(r["active"] for r in reports))
    k_uni = -(-total // (w * h))
    uacc, um2 = empty_state(w, h)
    uacc, um2 = moments_update(uacc, um2, passes[:k_uni], gamma)
    umean, _ = moments_resolve(uacc, um2, gamma)
    return dict(total=total, uniform_passes=k_uni, early=float((var[..., 3] < max_passes).mean()),
                rmse=rmse(mean, ref, gamma), rmse_uniform=rmse(umean, ref, gamma),
                rel=rel_error(mean, ref, gamma, floor), rel_uniform=rel_error(umean, ref, gamma, floor))
