"""rs_moments_update_device, rs_moments_resolve_device, rs_adaptive_mask_device and rs_render_adaptive[_device] on the
GPU, bit for bit (uint32 views) against the numpy restatement of the header's contracts (tests/adaptive_ref.py): the
seeded pass frames of test_gpu_denoise_var.py's recipe and a seeded state at 37 x 23 (smaller than any tile and than the
radius-4 reach) and 149 x 67 (several tiles each way with a remainder), and the loop on a rendered scene, driven by the
GPU's own maskless pass frames. Outputs and state sit between guard zones."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as R
import denoise_ref as D
import denoise_var_ref as V
from raysnail_amd import _abi as A
from raysnail_amd import api, scenes

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (149, 67)]
SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")
SENTINEL = -123.25
GUARD = 4096  # elements on each side of a guarded buffer
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same(got, exp):
    ok = (_bits(got) == _bits(exp)).all(axis=-1)
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (len(bad), [(int(y), int(x), got[y, x].tolist(), exp[y, x].tolist()) for y, x in bad[:4]])


class Guarded:
    """n elements of device memory between two guard zones that must come back untouched (as test_gpu_denoise_var's)"""

    def __init__(self, torch, n, init=None, dtype=None):
        dtype = dtype or torch.float32
        self.fill = SENTINEL if dtype == torch.float32 else 0xA5
        self.torch, self.n = torch, n
        self.arena = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.arena[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        assert bool((self.arena[:GUARD] == self.fill).all()) and bool((self.arena[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        self.check()
        return bool((self.t == self.fill).all())

    def numpy(self, shape):
        return self.t.cpu().numpy().reshape(shape)


@pytest.fixture(scope="module")
def pass_frames():
    """per size: the 64 seeded pass frames (read-only; NaN and Inf pixels on tile edges and in the last column)"""
    return {size: R.pass_frames(size[0], size[1], 40 + i) for i, size in enumerate(SIZES)}


# ------------------------------------------------------------------------------------ update ----
def run_update(torch, state, frames, gamma, stream=None):
    """rs_moments_update_device on guarded copies of the state; the frames must come back as they went in"""
    h, w = frames[0].shape[:2]
    acc, m2 = Guarded(torch, w * h * 4, state[0]), Guarded(torch, w * h * 4, state[1])
    dev = [torch.from_numpy(np.array(f, F)).cuda() for f in frames]
    keep = [t.clone() for t in dev]
    torch.cuda.synchronize()
    api.moments_update_device(acc.ptr(), m2.ptr(), [t.data_ptr() for t in dev], w, h, gamma,
                              0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    acc.check(); m2.check()
    for t, k in zip(dev, keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    return acc.numpy((h, w, 4)), m2.numpy((h, w, 4))


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 5, 64])
@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_update_from_empty(gpu, pass_frames, size, k, gamma):
    frames = pass_frames[size][:k]
    acc, m2 = run_update(gpu, R.empty_state(*size), frames, gamma)
    exp_acc, exp_m2 = R.moments_update(*R.empty_state(*size), frames, gamma)
    assert_same(acc, exp_acc)
    assert_same(m2, exp_m2)
    h = size[1]
    assert (_bits(acc)[h - 2, 1] == 0).all() and (_bits(m2)[h - 2, 1] == 0).all()  # masked in every frame
    if k >= 5:
        assert np.isfinite(acc).all() and np.isfinite(m2).all()  # the NaN and Inf samples reached nothing


@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_update_split_untouched_pixels_and_side_stream(gpu, pass_frames, size):
    """5 frames as 2 + 3 in two calls = one call of 5; a pixel no frame contributes to keeps a loud state bit for bit,
    m2.w included; one run on a side stream"""
    torch = gpu
    frames = pass_frames[size][:5]
    h = size[1]
    for gamma in (0, 1):
        one = run_update(torch, R.empty_state(*size), frames, gamma)
        two = run_update(torch, run_update(torch, R.empty_state(*size), frames[:2], gamma), frames[2:], gamma)
        assert np.array_equal(_bits(one[0]), _bits(two[0])) and np.array_equal(_bits(one[1]), _bits(two[1]))
    state = R.empty_state(*size)
    state[0][h - 2, 1] = [1.5, np.nan, -2.0, 3.0]
    state[1][h - 2, 1] = [4.0, 5.0, np.inf, 7.0]
    state[1][0, 0, 3] = 9.0  # a contributing pixel's m2.w is written as +0.0
    acc, m2 = run_update(torch, state, frames, 1, stream=torch.cuda.Stream())
    exp = R.moments_update(*state, frames, 1)
    assert_same(acc, exp[0])
    assert_same(m2, exp[1])
    assert np.array_equal(_bits(acc)[h - 2, 1], _bits(state[0])[h - 2, 1])
    assert np.array_equal(_bits(m2)[h - 2, 1], _bits(state[1])[h - 2, 1]) and _bits(m2)[0, 0, 3] == 0


# ----------------------------------------------------------------------------------- resolve ----
def run_resolve(torch, state, gamma, want=(True, True)):
    h, w = state[0].shape[:2]
    acc, m2 = Guarded(torch, w * h * 4, state[0]), Guarded(torch, w * h * 4, state[1])
    mean = Guarded(torch, w * h * 4) if want[0] else None
    var = Guarded(torch, w * h * 4) if want[1] else None
    torch.cuda.synchronize()
    api.moments_resolve_device(acc.ptr(), m2.ptr(), w, h, mean.ptr() if mean else 0, var.ptr() if var else 0, gamma)
    torch.cuda.synchronize()
    for g in (acc, m2, mean, var):
        if g is not None:
            g.check()
    assert np.array_equal(_bits(acc.numpy((h, w, 4))), _bits(state[0]))  # the state is read only
    assert np.array_equal(_bits(m2.numpy((h, w, 4))), _bits(state[1]))
    return (mean.numpy((h, w, 4)) if mean else None), (var.numpy((h, w, 4)) if var else None)


@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_resolve(gpu, pass_frames, size):
    """each output alone and both together; n = 0 (masked in all frames), 1 and 2 (the checkerboard) are present"""
    state = R.moments_update(*R.empty_state(*size), pass_frames[size][:3], 1)
    state[0][2, 2, 3] = 1.0  # (a pixel with one sample, whatever the frames gave it)
    n = state[0][..., 3]
    assert {0.0, 1.0, 2.0, 3.0} >= set(np.unique(n)) >= {0.0, 1.0, 2.0}
    for gamma in (0, 1):
        exp_mean, exp_var = R.moments_resolve(*state, gamma)
        mean, var = run_resolve(gpu, state, gamma)
        assert_same(mean, exp_mean)
        assert_same(var, exp_var)
        mean, none = run_resolve(gpu, state, gamma, want=(True, False))
        assert none is None
        assert_same(mean, exp_mean)
        none, var = run_resolve(gpu, state, gamma, want=(False, True))
        assert none is None
        assert_same(var, exp_var)
    # what rs_pass_moments defines for n <= 1
    assert (_bits(exp_var)[..., :3][n < 2] == 0).all() and (exp_mean[n == 0] == 0).all()


def test_resolve_feeds_denoise_var(gpu, pass_frames):
    """the resolved frames go into rs_denoise_var_device unchanged: the result is the numpy chain's"""
    torch = gpu
    w, h = size = SIZES[1]
    state = R.moments_update(*R.empty_state(*size), pass_frames[size][:6], 1)
    _, albedo, normal = D.synthetic(w, h, 11)
    exp_mean, exp_var = R.moments_resolve(*state, 1)
    st = api.DenoiseVarSettings()
    exp, _ = V.denoise_var(exp_mean, exp_var, albedo, normal, gamma=1, levels=st.levels, k_color=st.k_color,
                           sigma_normal=st.sigma_normal, sigma_depth=st.sigma_depth)
    dev = [torch.from_numpy(np.array(a, F)).cuda() for a in (state[0], state[1], albedo, normal)]
    mean, var, out = (torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3))
    work = Guarded(torch, 4 * w * h * 4)
    torch.cuda.synchronize()
    api.moments_resolve_device(dev[0].data_ptr(), dev[1].data_ptr(), w, h, mean.data_ptr(), var.data_ptr(), True)
    api.denoise_var_device(mean.data_ptr(), var.data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), w, h, out.data_ptr(), 0,
                           work.ptr(), st, True)
    torch.cuda.synchronize()
    work.check()
    assert_same(out.cpu().numpy(), exp)


# -------------------------------------------------------------------------------------- mask ----
MIN_N, MAX_N, TOLERANCE, FLOOR = 2, 8, 0.5, 0.5  # tol2 = 0.25 exactly


def seeded_state(size, frames):
    """six frames' state (n = 6, or 3 on the checkerboard) with planted pixels: hot (n = 1) in the four corners and on
    the seams of the 32 x 8 tiles; a block of loud M2 across a seam; a pixel at n = max_n inside it; a non-finite mean
    with n >= min_n (never hot) and a non-finite M2 with n < min_n (hot all the same), both counted; err2 exactly tol2
    (not hot) next to one a single ulp above (hot)"""
    w, h = size
    acc, m2 = R.moments_update(*R.empty_state(w, h), frames[:6], 0)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (7, 31), (8, 32), (7, 32), (8, 31), (15, 12), (16, 12)):
        acc[y, x, 3] = 1.0
    m2[10:14, 28:36, :3] *= F(40.0)
    acc[12, 33, 3] = MAX_N
    acc[18, 5] = [np.nan, 1.0, 1.0, 4.0]
    m2[18, 20] = [np.inf, 1.0, 1.0, 0.0]
    acc[18, 20, 3] = 1.0
    acc[20, 9] = [1.0, 0.0, 0.0, 2.0]
    m2[20, 9] = [0.5, 0.0, 0.0, 0.0]  # t / 2 = 0.25, Dn = max(1, floor) = 1: err2 == tol2
    acc[20, 15] = [1.0, 0.0, 0.0, 2.0]
    m2[20, 15] = [np.nextafter(F(0.5), F(1.0)), 0.0, 0.0, 0.0]
    return acc, m2


def base_mask(size):
    w, h = size
    yy, xx = np.mgrid[0:h, 0:w]
    base = ((xx + 3 * yy) % 5 != 0).astype(np.uint8)
    base[base != 0] = 1 + (xx + yy)[base != 0] % 3  # any non-zero byte counts
    for y, x in ((0, 0), (20, 9), (20, 15), (12, 33), (18, 5)):
        base[y, x] = 1
    base[h - 1, w - 1] = 0  # one planted corner switched off
    return base


def run_mask(torch, state, base, radius, stats=True, stream=None):
    h, w = state[0].shape[:2]
    acc, m2 = Guarded(torch, w * h * 4, state[0]), Guarded(torch, w * h * 4, state[1])
    d_base = None if base is None else Guarded(torch, w * h, base, torch.uint8)
    mask = Guarded(torch, w * h, dtype=torch.uint8)
    torch.cuda.synchronize()
    out = api.adaptive_mask_device(acc.ptr(), m2.ptr(), d_base.ptr() if d_base else 0, w, h, MIN_N, MAX_N, TOLERANCE,
                                   FLOOR, radius, mask.ptr(), 0 if stream is None else stream.cuda_stream, stats)
    (stream or torch.cuda.current_stream()).synchronize()
    for g in (acc, m2, mask, d_base):
        if g is not None:
            g.check()
    assert np.array_equal(_bits(acc.numpy((h, w, 4))), _bits(state[0]))
    return mask.numpy((h, w)), out


@pytest.mark.parametrize("with_base", [False, True], ids=["all", "base"])
@pytest.mark.parametrize("radius", [0, 1, 4])
@pytest.mark.parametrize("size", SIZES, **SIZE_IDS)
def test_mask(gpu, pass_frames, size, radius, with_base):
    state = seeded_state(size, pass_frames[size])
    base = base_mask(size) if with_base else None
    exp, exp_stats = R.adaptive_mask(*state, base, MIN_N, MAX_N, TOLERANCE, FLOOR, radius)
    hot, _, fin, _, _ = R.hot_map(*state, base, MIN_N, MAX_N, TOLERANCE, FLOOR)
    # the planted cases are what they are meant to be
    assert hot[0, 0] and hot[7, 31] and hot[8, 32] and hot[12, 32] and not hot[12, 33] and exp[12, 33] == 0
    assert not fin[18, 5] and not hot[18, 5] and not fin[18, 20] and hot[18, 20] and exp_stats["nonfinite"] == 2
    assert not hot[20, 9] and hot[20, 15]
    assert 0 < exp_stats["hot"] <= exp_stats["active"] < size[0] * size[1] and exp_stats["max_err2"] > 0.25
    mask, stats = run_mask(gpu, state, base, radius)
    assert np.array_equal(mask, exp), np.argwhere(mask != exp)[:8]
    assert (stats.active, stats.hot, stats.nonfinite) == (exp_stats["active"], exp_stats["hot"], exp_stats["nonfinite"])
    assert np.array([stats.max_err2], F).view(np.uint32)[0] == np.array([exp_stats["max_err2"]], F).view(np.uint32)[0]
    quiet, none = run_mask(gpu, state, base, radius, stats=False, stream=gpu.cuda.Stream() if radius == 1 else None)
    assert none is None and np.array_equal(quiet, exp)


def test_mask_of_the_empty_state_and_of_a_finished_one(gpu):
    w, h = SIZES[0]
    mask, stats = run_mask(gpu, R.empty_state(w, h), None, 1)
    assert (mask == 1).all() and (stats.active, stats.hot, stats.nonfinite, stats.max_err2) == (w * h, w * h, 0, 0.0)
    acc, m2 = R.empty_state(w, h)
    acc[..., 3] = MAX_N
    m2[..., :3] = 100.0
    mask, stats = run_mask(gpu, (acc, m2), None, 4)
    assert (mask == 0).all() and (stats.active, stats.hot) == (0, 0) and stats.max_err2 > 0


# -------------------------------------------------------------------------------------- loop ----
LW, LH, LOOP = 48, 32, dict(min_passes=2, max_passes=8, tolerance=0.2, floor=0.03, radius=1)
# (tolerance 0.2: on the oracle's frames of this scene the restatement's per-pass active counts run 1536, 1536, 974,
# 702, 483, 315, 177, 102 -- a third of the frame stops at 2 passes, 94 pixels reach 8)


@pytest.fixture(scope="module")
def loop_scene(gpu):
    """the scene, the photo, the GPU's own maskless frames of passes 0 .. 11, and the restatement's run on them"""
    cam, world, _, _ = scenes.rtow_13_1(LW, LH)
    photo = cam.take_photo().samples(4).depth(8).seed(1)
    frames = [cam.take_photo().samples(4).depth(8).seed(1).pass_index(p).shot(None, world) for p in range(12)]
    for f in frames:
        f.setflags(write=False)
    exp = R.render_adaptive(lambda p: frames[p], LW, LH, 1, base=None, **LOOP)
    return cam, world, photo, frames, exp


def test_loop_shot_adaptive(loop_scene):
    cam, world, photo, frames, (acc, m2, reports) = loop_scene
    exp_mean, exp_var = R.moments_resolve(acc, m2, 1)
    n = exp_var[..., 3]
    assert len(reports) == 8 and (n == 2).mean() > 0.2 and 0 < (n == 8).mean() < 0.2  # part of the frame stops early
    mean, var, passes, got = photo.shot_adaptive(world, api.AdaptiveSettings(**LOOP))
    assert [r.active for r in got] == [r["active"] for r in reports]
    assert [r.hot for r in got] == [r["hot"] for r in reports]
    assert [_bits(r.max_err2).item() for r in got] == [_bits(r["max_err2"]).item() for r in reports]
    assert_same(mean, exp_mean)
    assert_same(var, exp_var)
    assert np.array_equal(passes, n.astype(np.int32))
    for r, e in zip(got, reports):  # a masked pixel traces nothing: at most depth + 1 world.hit calls per live sample
        assert 4 * e["active"] <= r.stats.segments <= 4 * e["active"] * 9
    assert photo.last_stats.segments == got[-1].stats.segments and photo.settings().pass_ == 0


def test_loop_device_entry_base_mask_and_continuation(gpu, loop_scene):
    """rs_render_adaptive_device on guarded buffers gives rs_render_adaptive's frames; under a base mask with every
    fifth diagonal off those pixels stay [0,0,0,0] with n = 0; a finished state continued with max_passes raised to 12
    renders only the still-hot pixels"""
    torch = gpu
    cam, world, photo, frames, (acc0, m20, reports0) = loop_scene
    ds = world.device_scene()
    npx = LW * LH

    def run(settings, base, state, first_pass):
        acc, m2 = Guarded(torch, npx * 4, state[0]), Guarded(torch, npx * 4, state[1])
        work, wmask = Guarded(torch, npx * 4), Guarded(torch, npx, dtype=torch.uint8)
        d_base = None if base is None else Guarded(torch, npx, base, torch.uint8)
        torch.cuda.synchronize()
        st = cam.take_photo().samples(4).depth(8).seed(1).pass_index(first_pass).settings()
        got = ds.render_adaptive_device(cam.desc, st, settings, acc.ptr(), m2.ptr(), work.ptr(), wmask.ptr(),
                                        d_base.ptr() if d_base else 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for g in (acc, m2, work, wmask, d_base):
            if g is not None:
                g.check()
        return acc.numpy((LH, LW, 4)), m2.numpy((LH, LW, 4)), got

    acc, m2, got = run(api.AdaptiveSettings(**LOOP), None, R.empty_state(LW, LH), 0)
    assert_same(acc, acc0)
    assert_same(m2, m20)
    assert [r.active for r in got] == [r["active"] for r in reports0]
    # the host-buffer entry gave the same frames (test_loop_shot_adaptive compares it with the same restatement)

    yy, xx = np.mgrid[0:LH, 0:LW]
    base = ((xx + yy) % 5 != 0).astype(np.uint8)
    exp = R.render_adaptive(lambda p: frames[p], LW, LH, 1, base=base, **LOOP)
    acc, m2, got = run(api.AdaptiveSettings(**LOOP), base, R.empty_state(LW, LH), 0)
    assert_same(acc, exp[0])
    assert_same(m2, exp[1])
    assert (_bits(acc)[base == 0] == 0).all() and (_bits(m2)[base == 0] == 0).all()
    mean, var, _ = ds.render_adaptive(cam.desc, photo.settings(), api.AdaptiveSettings(**LOOP), base)
    exp_mean, exp_var = R.moments_resolve(exp[0], exp[1], 1)
    assert_same(mean, exp_mean)
    assert_same(var, exp_var)
    assert (_bits(mean)[base == 0] == 0).all() and (_bits(var)[base == 0] == 0).all()

    more = dict(LOOP, max_passes=12)
    exp = R.render_adaptive(lambda p: frames[8 + p], LW, LH, 1, base=None, state=(acc0, m20), **more)
    acc, m2, got = run(api.AdaptiveSettings(**more), None, (acc0, m20), 8)
    assert_same(acc, exp[0])
    assert_same(m2, exp[1])
    assert [r.active for r in got] == [r["active"] for r in exp[2]]
    assert 0 < got[0].active < reports0[-1]["active"] and len(got) <= 4
    unchanged = acc0[..., 3] < 8
    assert np.array_equal(_bits(acc)[unchanged], _bits(acc0)[unchanged])  # a pixel that had stopped stays stopped


@pytest.mark.parametrize("rows", [(3, 21, 1), (1, 0, 3), (0, 1, 1), (5, 5, 1)], ids=lambda r: "rows%d-%d-%d" % r)
def test_loop_on_a_row_lattice(gpu, loop_scene, rows):
    """photo.rows(begin, end, step): rs_render_device leaves rows off the lattice untouched, so the loop treats them as
    base == 0 -- never sampled, n = 0, a loud earlier state kept bit for bit -- and stops early on the others as the
    restatement does; row 0 off the lattice (the mask's counters live in the work frame's first pixel) and on it
    alone; an empty lattice renders nothing. The work frame starts as garbage."""
    torch = gpu
    cam, world, _, frames, _ = loop_scene
    ds = world.device_scene()
    npx = LW * LH
    on = R.lattice_base(LW, LH, None, rows) != 0
    exp = R.render_adaptive(lambda p: frames[p], LW, LH, 1, rows=rows, **LOOP)
    photo = cam.take_photo().samples(4).depth(8).seed(1).rows(*rows)
    mean, var, passes, got = photo.shot_adaptive(world, api.AdaptiveSettings(**LOOP))
    exp_mean, exp_var = R.moments_resolve(exp[0], exp[1], 1)
    assert [r.active for r in got] == [r["active"] for r in exp[2]]
    assert_same(mean, exp_mean)
    assert_same(var, exp_var)
    assert (_bits(mean)[~on] == 0).all() and (_bits(var)[~on] == 0).all()
    if on.any():
        assert got[0].active == int(on.sum()) and 2 <= len(got) <= 8 and got[-1].active <= got[0].active
        assert (passes[on] >= 2).all()
    else:
        assert got == []
    # the device entry on a loud work frame, continuing a state whose off-lattice pixels must come back bit for bit
    state = R.empty_state(LW, LH)
    state[0][~on] = [1.5, np.nan, -2.0, 1.0]
    state[1][~on] = [4.0, 5.0, np.inf, 7.0]
    exp = R.render_adaptive(lambda p: frames[p], LW, LH, 1, rows=rows, state=state, **LOOP)
    acc, m2 = Guarded(torch, npx * 4, state[0]), Guarded(torch, npx * 4, state[1])
    work, wmask = Guarded(torch, npx * 4), Guarded(torch, npx, dtype=torch.uint8)
    torch.cuda.synchronize()
    got = ds.render_adaptive_device(cam.desc, photo.settings(), api.AdaptiveSettings(**LOOP), acc.ptr(), m2.ptr(),
                                    work.ptr(), wmask.ptr())
    torch.cuda.synchronize()
    for g in (acc, m2, work, wmask):
        g.check()
    assert [r.active for r in got] == [r["active"] for r in exp[2]]
    assert_same(acc.numpy((LH, LW, 4)), exp[0])
    assert_same(m2.numpy((LH, LW, 4)), exp[1])
    assert np.array_equal(_bits(acc.numpy((LH, LW, 4)))[~on], _bits(state[0])[~on])
    assert np.array_equal(_bits(m2.numpy((LH, LW, 4)))[~on], _bits(state[1])[~on])
    w4 = work.numpy((LH, LW, 4))
    assert (_bits(w4)[~on] == 0).all() and (_bits(w4)[0, 0] == 0).all()


# ------------------------------------------------------------------------- invalid arguments ----
def test_invalid_arguments_leave_the_buffers_alone(gpu, loop_scene):
    torch = gpu
    w, h = SIZES[0]
    n = w * h * 4
    acc, m2, frame, mean, var = (Guarded(torch, n) for _ in range(5))
    mask = Guarded(torch, w * h, dtype=torch.uint8)
    torch.cuda.synchronize()
    inf, nan = float("inf"), float("nan")

    def invalid(fn, *args, **kw):
        with pytest.raises(api.RaysnailError) as e:
            fn(*args, **kw)
        assert e.value.code == A.RS_E_INVALID, e.value

    up = api.moments_update_device
    invalid(up, 0, m2.ptr(), [frame.ptr()], w, h, 1)
    invalid(up, acc.ptr(), 0, [frame.ptr()], w, h, 1)
    invalid(up, acc.ptr(), m2.ptr(), [], w, h, 1)
    invalid(up, acc.ptr(), m2.ptr(), [frame.ptr()] * 65, w, h, 1)
    invalid(up, acc.ptr(), m2.ptr(), [frame.ptr(), 0], w, h, 1)
    invalid(up, acc.ptr(), m2.ptr(), [frame.ptr()], w, h, 2)
    invalid(up, acc.ptr(), m2.ptr(), [frame.ptr()], 0, h, 1)
    invalid(up, acc.ptr(), m2.ptr(), [frame.ptr()], 0x10000, 0x8000, 1)  # W H = 2^31
    lib = A.load()
    assert lib.rs_moments_update_device(acc.ptr(), m2.ptr(), None, 1, w, h, 1, None) == A.RS_E_INVALID
    rs = api.moments_resolve_device
    invalid(rs, 0, m2.ptr(), w, h, mean.ptr(), var.ptr(), 1)
    invalid(rs, acc.ptr(), 0, w, h, mean.ptr(), var.ptr(), 1)
    invalid(rs, acc.ptr(), m2.ptr(), w, h, 0, 0, 1)
    invalid(rs, acc.ptr(), m2.ptr(), w, h, mean.ptr(), var.ptr(), 2)
    invalid(rs, acc.ptr(), m2.ptr(), w, 0, mean.ptr(), var.ptr(), 1)
    invalid(rs, acc.ptr(), m2.ptr(), 0x10000, 0x8000, mean.ptr(), var.ptr(), 1)
    mk = api.adaptive_mask_device
    good = dict(min_n=2, max_n=8, tolerance=0.1, floor=0.03, radius=1)
    for bad in (dict(min_n=1), dict(min_n=0), dict(max_n=1), dict(min_n=9), dict(max_n=4097), dict(tolerance=nan),
                dict(tolerance=inf), dict(tolerance=1e-7), dict(tolerance=2e4), dict(floor=nan), dict(floor=0.0),
                dict(floor=-1.0), dict(floor=2e4), dict(radius=5)):
        for stats in (True, False):
            invalid(mk, acc.ptr(), m2.ptr(), 0, w, h, d_mask_ptr=mask.ptr(), stats=stats, **dict(good, **bad))
    invalid(mk, 0, m2.ptr(), 0, w, h, d_mask_ptr=mask.ptr(), **good)
    invalid(mk, acc.ptr(), 0, 0, w, h, d_mask_ptr=mask.ptr(), **good)
    invalid(mk, acc.ptr(), m2.ptr(), 0, w, h, d_mask_ptr=0, **good)
    invalid(mk, acc.ptr(), m2.ptr(), 0, 0, h, d_mask_ptr=mask.ptr(), **good)
    invalid(mk, acc.ptr(), m2.ptr(), 0, 0x10000, 0x8000, d_mask_ptr=mask.ptr(), **good)
    # the loop: a bad setting, or a missing buffer, before anything is rendered
    cam, world, photo, _, _ = loop_scene
    ds = world.device_scene()
    npx = LW * LH
    lacc, lm2, lwork = (Guarded(torch, npx * 4) for _ in range(3))
    lmask = Guarded(torch, npx, dtype=torch.uint8)
    torch.cuda.synchronize()
    ok = api.AdaptiveSettings(**LOOP)
    for bad in (dict(min_passes=1), dict(max_passes=1), dict(max_passes=4097), dict(tolerance=nan), dict(floor=0.0),
                dict(radius=5)):
        st = api.AdaptiveSettings(**dict(LOOP, **bad))
        invalid(ds.render_adaptive_device, cam.desc, photo.settings(), st, lacc.ptr(), lm2.ptr(), lwork.ptr(), lmask.ptr())
        invalid(ds.render_adaptive, cam.desc, photo.settings(), st)
    invalid(ds.render_adaptive_device, cam.desc, photo.settings(), ok, 0, lm2.ptr(), lwork.ptr(), lmask.ptr())
    invalid(ds.render_adaptive_device, cam.desc, photo.settings(), ok, lacc.ptr(), 0, lwork.ptr(), lmask.ptr())
    invalid(ds.render_adaptive_device, cam.desc, photo.settings(), ok, lacc.ptr(), lm2.ptr(), 0, lmask.ptr())
    invalid(ds.render_adaptive_device, cam.desc, photo.settings(), ok, lacc.ptr(), lm2.ptr(), lwork.ptr(), 0)
    assert lib.rs_render_adaptive(ds.handle, C.byref(cam.desc), C.byref(photo.settings()), C.byref(ok.desc()), None, None,
                                  None, None, None) == A.RS_E_INVALID
    torch.cuda.synchronize()
    for g in (acc, m2, frame, mean, var, mask, lacc, lm2, lwork, lmask):
        assert g.untouched()
