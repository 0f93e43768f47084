#!/usr/bin/env python
"""dev: time the adaptive pass loop's kernels -- rs_moments_update_device (1 and 4 frames), rs_moments_resolve_device
(both outputs), rs_adaptive_mask_device (radius 1, no statistics: the launch alone) -- in the same process as
rs_pass_moments_device (K = 4) and rs_denoise_var_device (defaults, both guides), at 800 x 500 and 1920 x 1080; then the
bench scene (RTIOW 13.1, 800 x 500, 64 spp per pass, depth 8) through shot_adaptive's device entry with the default
settings against the same number of uniform passes of rs_render_device, and one masked pass at several live shares.

HIP events around each call on torch's current stream; per shape `rounds` rounds after `warmup` calls of every variant,
the variants alternating call by call inside a round (`reps` timed calls each per round). Reported per variant: the
median over all timed calls, the range of the round medians, and the bytes the kernel moves per call (the state is 32 B
per pixel, a frame 16 B; the mask kernel reads 32 B per tile cell, halo included: (34 x 10) / (32 x 8) of the pixels at
radius 1) with the rate that gives.
usage: python tools/adaptive_bench.py [--rounds 5] [--reps 40] [--warmup 10] [--out FILE.jsonl] [--no-scene]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec


def kernels(args, torch, api, emit):
    st_var = api.DenoiseVarSettings()
    for w, h in ((800, 500), (1920, 1080)):
        g = torch.Generator(device="cuda").manual_seed(w)
        passes = []
        for _ in range(4):
            f = torch.rand((h, w, 4), generator=g, device="cuda") * 2.0
            f[..., 3] = 1.0
            passes.append(f)
        acc, m2 = torch.zeros_like(passes[0]), torch.zeros_like(passes[0])
        mean, var, out = torch.empty_like(acc), torch.empty_like(acc), torch.empty_like(acc)
        albedo = torch.rand((h, w, 4), generator=g, device="cuda")
        albedo[..., 3] = 1.0
        normal = torch.rand((h, w, 4), generator=g, device="cuda")
        normal[..., 3] = 2.0 + 8.0 * (torch.arange(w, device="cuda")[None, :] * 4 // w).float()
        work = torch.empty((4 * w * h * 4,), dtype=torch.float32, device="cuda")
        mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ptrs = [f.data_ptr() for f in passes]
        n = w * h
        cells = ((w + 31) // 32) * ((h + 7) // 8) * 34 * 10  # (cells off the frame load nothing: an upper bound)
        variants = {
            # (n grows with every update: the state stays finite, and the mask's answer does not change its traffic)
            "moments_update_1": (lambda: api.moments_update_device(acc.data_ptr(), m2.data_ptr(), ptrs[:1], w, h, True, stream),
                                 n * (64 + 16)),
            "moments_update_4": (lambda: api.moments_update_device(acc.data_ptr(), m2.data_ptr(), ptrs, w, h, True, stream),
                                 n * (64 + 64)),
            "moments_resolve": (lambda: api.moments_resolve_device(acc.data_ptr(), m2.data_ptr(), w, h, mean.data_ptr(),
                                                                   var.data_ptr(), True, stream), n * (32 + 32)),
            "adaptive_mask_r1": (lambda: api.adaptive_mask_device(acc.data_ptr(), m2.data_ptr(), 0, w, h, 2, 4096, 0.1, 0.03, 1,
                                                                  mask.data_ptr(), stream, stats=False), cells * 32 + n),
            "pass_moments_K4": (lambda: api.pass_moments_device(ptrs, w, h, mean.data_ptr(), var.data_ptr(), True, stream),
                                n * 16 * (4 + 2)),
            "denoise_var": (lambda: api.denoise_var_device(mean.data_ptr(), var.data_ptr(), albedo.data_ptr(),
                                                           normal.data_ptr(), w, h, out.data_ptr(), 0, work.data_ptr(),
                                                           st_var, True, stream), None),
        }
        for _ in range(args.warmup):
            for call, _ in variants.values():
                call()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            ev = {name: [] for name in variants}
            for _ in range(args.reps):
                for name, (call, _) in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    call()
                    b.record()
                    ev[name].append((a, b))
            torch.cuda.synchronize()
            for name in variants:
                times[name].append([a.elapsed_time(b) for a, b in ev[name]])
        for name, (_, nbytes) in variants.items():
            med = statistics.median(t for r in times[name] for t in r)
            rmed = [statistics.median(r) for r in times[name]]
            rec = {"shape": f"{w}x{h}", "variant": name, "calls": args.rounds * args.reps, "ms_median": round(med, 5),
                   "ms_round_medians_min": round(min(rmed), 5), "ms_round_medians_max": round(max(rmed), 5)}
            if nbytes:
                rec.update(bytes=nbytes, TBps=round(nbytes / (med * 1e-3) / 1e12, 3),
                           hbm_peak_fraction=round(nbytes / (med * 1e-3) / HBM_PEAK, 4))
            emit(rec)


def scene(args, torch, api, emit):
    from raysnail_amd import scenes
    w, h, spp = 800, 500, 64
    cam, world, _, _ = scenes.rtow_13_1(w, h)
    ds = world.device_scene()
    photo = cam.take_photo().samples(spp).depth(8).seed(1)
    acc, m2 = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    work = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    wmask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    settings = api.AdaptiveSettings()

    def adaptive(reports):
        acc.zero_(); m2.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ds.render_adaptive_device(cam.desc, photo.settings(), settings, acc.data_ptr(), m2.data_ptr(), work.data_ptr(),
                                      wmask.data_ptr(), 0, stream, reports=reports)
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def uniform(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in range(k):
            ds.render_device(cam.desc, photo.pass_index(p).settings(), work.data_ptr(), stream, stats=False)
        photo.pass_index(0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    reports, _ = adaptive(True)  # (warm-up, and the per-pass reports)
    n_passes = len(reports)
    uniform(2)
    ad = sorted(adaptive(False)[1] for _ in range(5))
    un = sorted(uniform(n_passes) for _ in range(5))
    total = sum(r.active for r in reports)
    emit({"scene": "rtow_13_1 800x500", "spp_per_pass": spp, "settings": settings.__dict__, "passes": n_passes,
          "active_per_pass": [r.active for r in reports], "pass_ms": [round(r.stats.ms, 3) for r in reports],
          "total_pass_pixels": total, "max_passes_x_pixels": settings.max_passes * w * h,
          "share_of_max": round(total / (settings.max_passes * w * h), 4),
          "adaptive_wall_ms_median_of_5": round(ad[2], 3), "adaptive_wall_ms_min_max": [round(ad[0], 3), round(ad[-1], 3)],
          "uniform_same_passes_wall_ms_median_of_5": round(un[2], 3),
          "uniform_wall_ms_min_max": [round(un[0], 3), round(un[-1], 3)]})
    # one masked pass at several live shares: a seeded random mask (scattered pixels) and a block of whole rows
    import numpy as np
    rng = np.random.default_rng(3)
    u = rng.random((h, w))
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    for share in (1.0, 0.5, 0.25, 0.1, 0.03, 0.01):
        for kind in ("scattered", "rows"):
            m = (u < share) if kind == "scattered" else (np.arange(h)[:, None] < share * h) & np.ones((1, w), bool)
            d_mask = torch.from_numpy(m.astype(np.uint8)).cuda()
            ts = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ds.render_device(cam.desc, photo.settings(), out.data_ptr(), stream, d_mask.data_ptr(), stats=False)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = sorted(ts[2:])
            emit({"masked_pass": kind, "live_share": round(float(m.mean()), 4), "wall_ms_median_of_5": round(ts[2], 3),
                  "wall_ms_min_max": [round(ts[0], 3), round(ts[-1], 3)]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scene", action="store_true")
    args = ap.parse_args()

    import torch
    from raysnail_amd import api
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    kernels(args, torch, api, emit)
    if not args.no_scene:
        scene(args, torch, api, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
