"""rs_pass_robust restated in numpy float32 from its contract in include/raysnail_hip.h: loops over frames, vectorised
over pixels, every intermediate an np.float32 array, every operation rounded once, in the header's order. The ranks come
from a stable argsort on the key, which is the header's total order (key, then frame index). And a float64 computation
of the same statistics, for the restatement's own error."""
import numpy as np

F = np.float32
AUTO = None  # trim: the Gini-driven trim


def _values(frames, gamma):
    """(x (K, H, W, 3) f32, key (K, H, W) f32, contributes (K, H, W) bool)"""
    fs = np.stack([np.ascontiguousarray(f, F) for f in frames])
    rgb = fs[..., 0:3]
    with np.errstate(all="ignore"):
        x = rgb * rgb if gamma else rgb.copy()
        s = (x[..., 0] + x[..., 1]) + x[..., 2]
    c = (fs[..., 3] != 0) & np.isfinite(rgb).all(axis=-1) & np.isfinite(s)
    return x, s, c


def _ranks(s, c):
    """r_k: the number of contributing j before k in (key, frame index) order; meaningless where k does not contribute"""
    key = np.where(c, s, F(np.inf))  # the frames that do not contribute go last: before no contributing frame
    order = np.argsort(key, axis=0, kind="stable")
    return np.argsort(order, axis=0, kind="stable").astype(np.int32)  # the inverse permutation


def trim_count(s, c, r, trim):
    """(n, t) (H, W) int32 of the keys s, the contributing flags c and the ranks r (K, H, W)"""
    K = s.shape[0]
    n = c.sum(axis=0).astype(np.int32)
    fn = n.astype(F)
    t_max = np.where(n >= 2, (n - 2) // 2, 0).astype(np.int32)
    with np.errstate(all="ignore"):
        if trim is AUTO:
            ss = np.zeros(n.shape, F)
            ng = np.zeros(n.shape, F)
            for k in range(K):
                ss = np.where(c[k], ss + s[k], ss)
                ng = np.where(c[k], ng + (2 * r[k] - (n - 1)).astype(F) * s[k], ng)
            G = np.where(ss > 0, ng / (fn * ss), F(0.0)).astype(F)
            G = np.fmin(np.fmax(G, F(0.0)), F(1.0))  # fmaxf / fminf: a NaN becomes 0
            cut = np.floor((G * fn) * F(0.5))
        else:
            assert 0.0 <= trim <= 0.5
            cut = np.floor(F(trim) * fn)
    t = np.minimum(t_max, cut.astype(np.int32)).astype(np.int32)
    return n, t


def pass_robust(frames, gamma=1, trim=AUTO):
    """(mean, var, trimmed) rs_pass_robust writes for these K (H, W, 4) float32 frames"""
    assert 1 <= len(frames) <= 64 and gamma in (0, 1)
    x, s, c = _values(frames, gamma)
    K, H, W = s.shape
    r = _ranks(s, c)
    n, t = trim_count(s, c, r, trim)
    fn = n.astype(F)
    h = n - 2 * t
    top = n - 1 - t
    with np.errstate(all="ignore"):
        S = np.zeros((H, W, 3), F)
        xlo = np.zeros((H, W, 3), F)
        xhi = np.zeros((H, W, 3), F)
        for k in range(K):
            kept = c[k] & (r[k] >= t) & (r[k] <= top)
            S = np.where(kept[..., None], S + x[k], S)
            xlo = np.where((c[k] & (r[k] == t))[..., None], x[k], xlo)
            xhi = np.where((c[k] & (r[k] == top))[..., None], x[k], xhi)
        fh = h.astype(F)
        mu = S / fh[..., None]
        w = [np.where((r[k] < t)[..., None], xlo, np.where((r[k] > top)[..., None], xhi, x[k])) for k in range(K)]
        Sw = np.zeros((H, W, 3), F)
        for k in range(K):
            Sw = np.where(c[k][..., None], Sw + w[k], Sw)
        mw = Sw / fn[..., None]
        Q = np.zeros((H, W, 3), F)
        for k in range(K):
            d = w[k] - mw
            Q = np.where(c[k][..., None], Q + d * d, Q)
        den = fh * (h - 1).astype(F)
        v = Q / den[..., None]
        m = np.sqrt(mu) if gamma else mu
    mean = np.zeros((H, W, 4), F)
    mean[..., 0:3] = np.where((n >= 1)[..., None], m, F(0.0))
    mean[..., 3] = np.where(n >= 1, F(1.0), F(0.0))
    var = np.zeros((H, W, 4), F)
    var[..., 0:3] = np.where((n >= 2)[..., None], v, F(0.0))
    var[..., 3] = fn
    return mean, var, t.astype(np.uint8)


def pass_robust_f64(frames, gamma, t):
    """(mu, v) (H, W, 3) float64: the trimmed mean and its Winsorised variance of the same frames with the trim counts
    t (H, W) given, the f32 inputs (and their f32 keys' order) taken as exact; NaN where undefined"""
    x32, s, c = _values(frames, gamma)
    fs = np.stack([np.asarray(f, np.float64) for f in frames])[..., 0:3]
    x = fs * fs if gamma else fs
    K = len(frames)
    r = _ranks(s, c)
    n = c.sum(axis=0)
    h, top = n - 2 * t, n - 1 - t
    with np.errstate(all="ignore"):
        kept = c & (r >= t) & (r <= top)
        mu = np.where(kept[..., None], x, 0.0).sum(axis=0) / h[..., None]
        xlo = np.where((c & (r == t))[..., None], x, 0.0).sum(axis=0)
        xhi = np.where((c & (r == top))[..., None], x, 0.0).sum(axis=0)
        w = np.where((r < t)[..., None], xlo[None], np.where((r > top)[..., None], xhi[None], x))
        w = np.where(c[..., None], w, 0.0)
        mw = w.sum(axis=0) / n[..., None]
        Q = np.where(c[..., None], (w - mw[None]) ** 2, 0.0).sum(axis=0)
        v = Q / (h * (h - 1.0))[..., None]
    return mu, v
