"""rs_denoise restated in numpy float32 from the contract in include/raysnail_hip.h: loops over levels and taps,
vectorised over pixels, every intermediate an np.float32 (array), every operation rounded once, in the header's order.
And the seeded synthetic frames the denoiser's tests share.
"""
import numpy as np

F = np.float32
K = [F(1.0) / F(16.0), F(4.0) / F(16.0), F(6.0) / F(16.0), F(4.0) / F(16.0), F(1.0) / F(16.0)]


def constants(levels, sigma_color, sigma_normal, sigma_depth):
    """(ic_i for each level, inv_n, inv_d), in f32"""
    sc, sn, sd = F(sigma_color), F(sigma_normal), F(sigma_depth)
    ic = []
    for i in range(levels):
        si = sc * F(2.0 ** -i)
        ic.append(F(1.0) / (si * si))
    return ic, F(1.0) / (sn * sn), F(1.0) / (sd * sd)


def modulation(albedo):
    """m of the prepare step: max(albedo.rgb + (1 - albedo.w), 1e-3) per channel"""
    u = F(1.0) - albedo[..., 3]
    return np.maximum(albedo[..., 0:3] + u[..., None], F(1e-3))


def prepare(beauty, albedo, normal, gamma):
    """(level 0's colours (H, W, 3), usable (H, W) bool, m or None)"""
    c = beauty[..., 0:3].copy()
    usable = (beauty[..., 3] != 0) & np.isfinite(beauty[..., 0:3]).all(axis=-1)
    if gamma:
        c = c * c
    m = None
    if albedo is not None:
        usable &= np.isfinite(albedo).all(axis=-1)
        m = modulation(albedo)
        c = c / m
    if normal is not None:
        usable &= np.isfinite(normal).all(axis=-1)
    usable &= np.isfinite(c).all(axis=-1)
    return c, usable, m


def _shifted(a, ox, oy, fill):
    """b[y, x] = a[y + oy, x + ox] where that is inside the frame, else fill"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys0, ys1 = max(0, -oy), min(H, H - oy)
    xs0, xs1 = max(0, -ox), min(W, W - ox)
    if ys0 < ys1 and xs0 < xs1:
        b[ys0:ys1, xs0:xs1] = a[ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return b


def level(c, usable, g, s, ic, inv_n, inv_d):
    """one a-trous level with step s: the new colours (pixels that are not usable keep theirs)"""
    H, W = usable.shape
    acc = np.zeros((H, W, 3), F)  # +0.0
    wsum = np.zeros((H, W), F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            h = K[dx + 2] * K[dy + 2]
            if dx == 0 and dy == 0:
                take = np.ones((H, W), bool)
                cq = c
                w = np.full((H, W), h, F)
            else:
                take = _shifted(usable, s * dx, s * dy, False)
                cq = _shifted(c, s * dx, s * dy, F(0.0))
                d = cq - c
                dc2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                A = F(1.0) + dc2 * ic
                if g is not None:
                    gq = _shifted(g, s * dx, s * dy, F(0.0))
                    n = gq[..., 0:3] - g[..., 0:3]
                    dn2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
                    dd = gq[..., 3] - g[..., 3]
                    M = np.maximum(np.maximum(np.abs(g[..., 3]), np.abs(gq[..., 3])), F(1e-6))
                    M2 = M * M
                    B = F(1.0) + dn2 * inv_n
                    D = M2 + (dd * dd) * inv_d
                    w = h * (M2 / ((A * B) * D))
                else:
                    w = h * (F(1.0) / A)
            # a skipped tap leaves the sums as they are
            acc = np.where(take[..., None], acc + w[..., None] * cq, acc)
            wsum = np.where(take, wsum + w, wsum)
    new = acc / wsum[..., None]
    return np.where(usable[..., None], new, c)


def denoise(beauty, albedo=None, normal=None, levels=5, sigma_color=0.3, sigma_normal=0.25, sigma_depth=0.1, gamma=1):
    """the frame rs_denoise writes for these (H, W, 4) float32 frames"""
    beauty = np.ascontiguousarray(beauty, F)
    albedo = None if albedo is None else np.ascontiguousarray(albedo, F)
    normal = None if normal is None else np.ascontiguousarray(normal, F)
    assert 1 <= levels <= 8 and gamma in (0, 1)
    ic, inv_n, inv_d = constants(levels, sigma_color, sigma_normal, sigma_depth)
    with np.errstate(all="ignore"):
        c, usable, m = prepare(beauty, albedo, normal, gamma)
        for i in range(levels):
            c = level(c, usable, normal, 1 << i, ic[i], inv_n, inv_d)
        if m is not None:
            c = c * m
        if gamma:
            c = np.sqrt(c)
    out = beauty.copy()
    out[..., 0:3] = np.where(usable[..., None], c, beauty[..., 0:3])
    return out


def synthetic(w, h, seed):
    """seeded frames: colour in [0, 4); albedo in flat regions, exact 0 and coverage < 1 among them; normals from a
    handful of directions; depths on three planes plus background 0. Guides premultiplied by coverage."""
    rng = np.random.default_rng(seed)
    beauty = np.ones((h, w, 4), np.float32)
    beauty[..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(4.0)
    region = ((np.arange(h)[:, None] * 5 // h) + 2 * (np.arange(w)[None, :] * 4 // w)) % 6
    alb_of = np.array([[0.8, 0.6, 0.2], [0.0, 0.0, 0.0], [0.25, 0.5, 0.75], [1.0, 1.0, 1.0], [0.0, 0.9, 0.0],
                       [0.5, 0.5, 0.5]], np.float32)
    cov_of = np.array([1.0, 1.0, 0.5, 1.0, 0.75, 0.0], np.float32)
    dirs = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0.0, 0.8], [0.0, -0.6, 0.8], [0, 0, 0]], np.float32)
    depth_of = np.array([2.5, 2.5, 7.0, 40.0, 7.0, 0.0], np.float32)
    cov = cov_of[region]
    albedo = np.concatenate([alb_of[region] * cov[..., None], cov[..., None]], axis=-1).astype(np.float32)
    normal = np.concatenate([dirs[region] * cov[..., None], (depth_of[region] * cov)[..., None]], axis=-1).astype(np.float32)
    return beauty, albedo, normal
