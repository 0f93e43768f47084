#!/usr/bin/env python
"""dev: time rs_pass_robust_device (K = 4, 16 and 64; trim 0, 0.1 and automatic) against rs_pass_moments_device at the
same K in the same process, at 800 x 500 and 1920 x 1080. The yardstick is that existing kernel: it reads the same bytes.

HIP events around each call on torch's current stream; per shape and K `rounds` rounds after `warmup` calls of every
variant, the four variants alternating call by call inside a round (`reps` timed calls each per round). The frames are
seeded noise in [0, 2) with a firefly of 1e3 in one frame of every 16th pixel, so the automatic trim cuts in some waves
and not in others. Reported per variant: the median over all timed calls and the range of the round medians; the
compulsory traffic (K frame reads and the two frame stores, 16 (K + 2) B per pixel, plus 1 B per pixel of trim counts)
over the median as a fraction of the 8 TB/s HBM peak; for the robust variants the ratio to rs_pass_moments_device.
usage: python tools/robust_bench.py [--rounds 5] [--reps 20] [--warmup 5] [--out FILE.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from raysnail_amd import api
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    lines = []
    for w, h in ((800, 500), (1920, 1080)):
        g = torch.Generator(device="cuda").manual_seed(w)
        passes = []
        for k in range(64):
            f = torch.rand((h, w, 4), generator=g, device="cuda") * 2.0
            f[..., 3] = 1.0
            passes.append(f)
        flat = passes[5].view(-1, 4)
        flat[::16, :3] = 1e3
        mean, var = torch.empty_like(passes[0]), torch.empty_like(passes[0])
        trimmed = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ptrs = [f.data_ptr() for f in passes]
        n = w * h
        for K in (4, 16, 64):
            def robust(trim, K=K):
                return lambda: api.pass_robust_device(ptrs[:K], w, h, mean.data_ptr(), var.data_ptr(), trimmed.data_ptr(),
                                                      True, trim, stream)
            variants = {
                f"pass_moments_K{K}": lambda K=K: api.pass_moments_device(ptrs[:K], w, h, mean.data_ptr(), var.data_ptr(),
                                                                          True, stream),
                f"pass_robust_K{K}_trim0": robust(0.0),
                f"pass_robust_K{K}_trim0.1": robust(0.1),
                f"pass_robust_K{K}_auto": robust(None),
            }
            for _ in range(args.warmup):
                for call in variants.values():
                    call()
            torch.cuda.synchronize()
            times = {name: [] for name in variants}
            for _ in range(args.rounds):
                ev = {name: [] for name in variants}
                for _ in range(args.reps):
                    for name, call in variants.items():
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        call()
                        b.record()
                        ev[name].append((a, b))
                torch.cuda.synchronize()
                for name in variants:
                    times[name].append([a.elapsed_time(b) for a, b in ev[name]])
            med = {name: statistics.median(t for r in times[name] for t in r) for name in variants}
            base = med[f"pass_moments_K{K}"]
            for name in variants:
                rmed = [statistics.median(r) for r in times[name]]
                is_robust = name.startswith("pass_robust")
                hbm = n * (16 * (K + 2) + (1 if is_robust else 0))
                rec = {"shape": f"{w}x{h}", "variant": name, "calls": args.rounds * args.reps,
                       "ms_median": round(med[name], 5), "ms_round_medians_min": round(min(rmed), 5),
                       "ms_round_medians_max": round(max(rmed), 5), "hbm_bytes": hbm,
                       "hbm_peak_fraction": round(hbm / (med[name] * 1e-3) / HBM_PEAK, 4)}
                if is_robust:
                    rec["over_pass_moments"] = round(med[name] / base, 3)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
