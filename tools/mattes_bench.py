#!/usr/bin/env python
"""dev: what the matte pass's count-and-rank costs, and what rs_matte_extract_device moves.

1. rs_render_mattes_device (ranks 4 and 8) against rs_render_features_specular_device with the same max_specular (0 and
   4) on the benchmark's scene (RTIOW 13.1 at 800 x 500) at 16 and 64 spp, in one process: the two walk the same rays,
   so the difference is the reduction's (the feature kernel's is eight f64 sums per pixel through LDS). HIP events
   around each call on torch's current stream, stats off (asynchronous calls); `rounds` rounds after `warmup` calls of
   every variant, the variants alternating call by call inside a round (`reps` timed calls each per round). Reported
   per variant: the median over all timed calls, the range of the round medians, and for the matte variants the
   ratio to the feature pass and the difference in ms.
2. rs_matte_extract_device at 800 x 500 and 1920 x 1080 on rendered-like layers (ranks 4 and 8; 1, 8 and 64 wanted
   ids): the compulsory traffic (8 ranks + 4 bytes per pixel) over the median as a fraction of the 8 TB/s HBM peak.
usage: python tools/mattes_bench.py [--rounds 5] [--reps 10] [--warmup 3] [--out FILE.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec


def timed(torch, variants, rounds, reps, warmup):
    """{name: [[ms of each timed call] per round]}, the variants alternating call by call"""
    for _ in range(warmup):
        for call in variants.values():
            call()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        ev = {name: [] for name in variants}
        for _ in range(reps):
            for name, call in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        for name in variants:
            times[name].append([a.elapsed_time(b) for a, b in ev[name]])
    return times


def summary(times, name):
    rmed = [statistics.median(r) for r in times[name]]
    return {"calls": sum(len(r) for r in times[name]), "ms_median": round(statistics.median(t for r in times[name] for t in r), 5),
            "ms_round_medians_min": round(min(rmed), 5), "ms_round_medians_max": round(max(rmed), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from raysnail_amd import api, scenes
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    w, h = 800, 500
    cam, world, _, _ = scenes.rtow_13_1(w, h)
    ds = world.device_scene()
    stream = torch.cuda.current_stream().cuda_stream
    alb = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    nrm = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty((h, w, 8), dtype=torch.int32, device="cuda")
    cov = torch.empty((h, w, 8), dtype=torch.float32, device="cuda")
    ovf = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    for spp in (16, 64):
        st = cam.take_photo().samples(spp).seed(1).settings()
        for m in (0, 4):
            variants = {
                "features": lambda m=m, st=st: ds.render_features_device(cam.desc, st, alb.data_ptr(), nrm.data_ptr(), stream,
                                                                         stats=False, max_specular=m),
                "mattes_r4": lambda m=m, st=st: ds.render_mattes_device(cam.desc, st, ids.data_ptr(), cov.data_ptr(),
                                                                        ovf.data_ptr(), 4, m, stream, stats=False),
                "mattes_r8": lambda m=m, st=st: ds.render_mattes_device(cam.desc, st, ids.data_ptr(), cov.data_ptr(),
                                                                        ovf.data_ptr(), 8, m, stream, stats=False),
            }
            times = timed(torch, variants, args.rounds, args.reps, args.warmup)
            base = summary(times, "features")["ms_median"]
            for name in variants:
                rec = {"what": "pass", "shape": f"{w}x{h}", "spp": spp, "max_specular": m, "variant": name}
                rec.update(summary(times, name))
                if name != "features":
                    rec["over_features"] = round(rec["ms_median"] / base, 4)
                    rec["ms_more_than_features"] = round(rec["ms_median"] - base, 5)
                emit(rec)

    for w, h in ((800, 500), (1920, 1080)):
        g = torch.Generator(device="cuda").manual_seed(w)
        out = torch.empty((h, w), dtype=torch.float32, device="cuda")
        for ranks in (4, 8):
            lid = torch.randint(-2, 40, (h, w, ranks), generator=g, device="cuda", dtype=torch.int32)
            lcv = torch.rand((h, w, ranks), generator=g, device="cuda")
            variants = {f"extract_r{ranks}_w{k}": (lambda k=k: api.matte_extract_device(lid.data_ptr(), lcv.data_ptr(), w, h,
                                                                                         ranks, list(range(k)), out.data_ptr(),
                                                                                         stream))
                        for k in (1, 8, 64)}
            times = timed(torch, variants, args.rounds, args.reps * 2, args.warmup)
            for name in variants:
                rec = {"what": "extract", "shape": f"{w}x{h}", "ranks": ranks, "variant": name}
                rec.update(summary(times, name))
                rec["hbm_bytes"] = w * h * (8 * ranks + 4)
                rec["hbm_peak_fraction"] = round(rec["hbm_bytes"] / (rec["ms_median"] * 1e-3) / HBM_PEAK, 4)
                emit(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
