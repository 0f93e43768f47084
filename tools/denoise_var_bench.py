#!/usr/bin/env python
"""dev: time rs_pass_moments_device (K = 4 and 16) and rs_denoise_var_device (default settings, both guides, gamma 1)
against rs_denoise_device at the same shape in the same process, at 800 x 500 and 1920 x 1080.

HIP events around each call on torch's current stream; per shape `rounds` rounds after `warmup` calls of every variant,
the variants alternating call by call inside a round (`reps` timed calls each per round). Reported per variant: the
median over all timed calls and the range of the round medians (the run-to-run spread); for the moments kernel its
compulsory traffic (K frame reads, the second sweep from cache, and two stores: 16 (K + 2) B per pixel from / to HBM,
16 (2 K + 2) B per pixel through the caches) as fractions of the HBM peak; for the filters their ratio.
usage: python tools/denoise_var_bench.py [--rounds 5] [--reps 40] [--warmup 10] [--out FILE.jsonl]
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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from raysnail_amd import api
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    st_fixed, st_var = api.DenoiseSettings(), api.DenoiseVarSettings()
    lines = []
    for w, h in ((800, 500), (1920, 1080)):
        g = torch.Generator(device="cuda").manual_seed(w)
        passes = []
        for _ in range(16):
            f = torch.rand((h, w, 4), generator=g, device="cuda") * 2.0
            f[..., 3] = 1.0
            passes.append(f)
        beauty, var = torch.empty_like(passes[0]), torch.empty_like(passes[0])
        albedo = torch.rand((h, w, 4), generator=g, device="cuda")
        albedo[..., 3] = 1.0
        normal = torch.rand((h, w, 4), generator=g, device="cuda")
        normal[..., 3] = 2.0 + 8.0 * (torch.arange(w, device="cuda")[None, :] * 4 // w).float()  # four depth planes
        work = torch.empty((4 * w * h * 4,), dtype=torch.float32, device="cuda")
        out, out_var = torch.empty_like(beauty), torch.empty_like(beauty)
        mean16, var16 = torch.empty_like(beauty), torch.empty_like(beauty)
        stream = torch.cuda.current_stream().cuda_stream
        ptrs = [f.data_ptr() for f in passes]

        variants = {
            # (the K = 4 moments write the frames the two filters read)
            "pass_moments_K4": lambda: api.pass_moments_device(ptrs[:4], w, h, beauty.data_ptr(), var.data_ptr(), True, stream),
            "pass_moments_K16": lambda: api.pass_moments_device(ptrs, w, h, mean16.data_ptr(), var16.data_ptr(), True, stream),
            "denoise": lambda: api.denoise_device(beauty.data_ptr(), albedo.data_ptr(), normal.data_ptr(), w, h,
                                                  out.data_ptr(), work.data_ptr(), st_fixed, True, stream),
            "denoise_var": lambda: api.denoise_var_device(beauty.data_ptr(), var.data_ptr(), albedo.data_ptr(),
                                                          normal.data_ptr(), w, h, out.data_ptr(), out_var.data_ptr(),
                                                          work.data_ptr(), st_var, True, stream),
        }
        for _ in range(args.warmup):
            for call in variants.values():
                call()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}  # per variant, per round: the round's call times, ms
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
        n = w * h
        med = {}
        for name in variants:
            med[name] = statistics.median(t for r in times[name] for t in r)
            rmed = [statistics.median(r) for r in times[name]]
            rec = {"shape": f"{w}x{h}", "variant": name, "calls": args.rounds * args.reps, "ms_median": round(med[name], 5),
                   "ms_round_medians_min": round(min(rmed), 5), "ms_round_medians_max": round(max(rmed), 5)}
            if name.startswith("pass_moments"):
                k = int(name.split("K")[1])
                hbm, cache = n * 16 * (k + 2), n * 16 * (2 * k + 2)
                rec.update(hbm_bytes=hbm, hbm_peak_fraction=round(hbm / (med[name] * 1e-3) / HBM_PEAK, 4),
                           load_store_bytes=cache, load_store_TBps=round(cache / (med[name] * 1e-3) / 1e12, 3))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        lines.append(json.dumps({"shape": f"{w}x{h}", "denoise_var_over_denoise": round(med["denoise_var"] / med["denoise"], 3)}))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
