#!/usr/bin/env python
"""dev: time the feature passes on the bench scene (RTIOW 13.1, seed 7, 800 x 500) into device-resident frames, at 16
and at 64 spp: rs_render_features_device (the first-hit kernel) and rs_render_features_specular_device at max_specular
1 / 2 / 4 / 8, in one process.

HIP events around each asynchronous call on torch's current stream; `rounds` rounds after `warmup` calls of every
variant, the variants alternating call by call inside a round (`reps` timed calls each per round). Per variant: the
median over all timed calls, the range of the round medians, the World::hit calls of one frame (from a call with
statistics) and segments per second at the median.
--root DIR: import the package of another tree (the parent commit's, built); --first-hit-only: time only what that
tree has. Run the two trees alternately to compare the first-hit kernel across them.
usage: python tools/spec_features_bench.py [--rounds 5] [--reps 20] [--warmup 5] [--out FILE.jsonl] [--tag NAME]
"""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--first-hit-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch
    from raysnail_amd import scenes
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    W, H = 800, 500
    cam, world, _, _ = scenes.rtow_13_1(W, H)
    ds = world.device_scene()
    stream = torch.cuda.current_stream().cuda_stream
    a = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    n = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    budgets = [0] if args.first_hit_only else [0, 1, 2, 4, 8]
    lines = []
    for spp in (16, 64):
        st = cam.take_photo().samples(spp).depth(8).seed(1).settings()

        def variant(m):
            kw = {"max_specular": m} if m else {}
            return lambda stats=False: ds.render_features_device(cam.desc, st, a.data_ptr(), n.data_ptr(), stream,
                                                                 stats=stats, **kw)
        variants = {m: variant(m) for m in budgets}
        for _ in range(args.warmup):
            for call in variants.values():
                call()
        torch.cuda.synchronize()
        times = {m: [] for m in budgets}
        for _ in range(args.rounds):
            ev = {m: [] for m in budgets}
            for _ in range(args.reps):
                for m, call in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    ev[m].append((e0, e1))
            torch.cuda.synchronize()
            for m in budgets:
                times[m].append([e0.elapsed_time(e1) for e0, e1 in ev[m]])
        for m, call in variants.items():
            s = call(True)
            med = statistics.median(t for r in times[m] for t in r)
            rmed = [statistics.median(r) for r in times[m]]
            rec = {"tag": args.tag, "scene": f"rtow_13_1 {W}x{H}", "spp": spp, "max_specular": m,
                   "entry": "rs_render_features_device" if m == 0 else "rs_render_features_specular_device",
                   "calls": args.rounds * args.reps, "ms_median": round(med, 4),
                   "ms_round_medians_min": round(min(rmed), 4), "ms_round_medians_max": round(max(rmed), 4),
                   "samples": int(s.samples), "segments": int(s.segments),
                   "segments_per_sample": round(s.segments / s.samples, 4),
                   "Gsegments_per_s": round(s.segments / (med * 1e-3) / 1e9, 3),
                   "kernel_ms_of_the_call_with_stats": round(s.kernel_ms, 4)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
