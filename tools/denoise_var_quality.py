#!/usr/bin/env python
"""dev: the quality grid behind RS_DENOISE_VAR_K_COLOR / RS_DENOISE_VAR_LEVELS, on the CPU (the numpy restatements in
tests/ on oracle renders; no GPU).

Two scenes (RTIOW, features) at 64 x 40, depth 8; the noisy frame is pass_moments' mean of K passes of N spp (seed 1,
passes 0 .. K-1), the reference 1024 spp at seed 2, the guides features_ref's at 16 spp -- the inputs of
tests/test_denoise_var_cpu.py's quality test. Per cell (scene, K x N, gamma): RMSE over rgb of the mean, of rs_denoise
with its defaults on the mean, and of rs_denoise_var at every grid point (k_color, levels). Per grid point: the
smallest margin over the 16 cells, margin = 1 - rmse(denoise_var) / min(rmse(mean), rmse(denoise)); the default is the
point with the largest smallest margin.
usage: python tools/denoise_var_quality.py [--out profiles/denoise_var/quality.txt]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KS = [1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 6.0, 8.0]
LEVELS = [4, 5]


def rmse(a, b):
    import numpy as np
    e = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return math.sqrt(float(np.mean(e * e)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import denoise_ref as D
    import denoise_var_ref as V

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    points = [(k, lv) for lv in LEVELS for k in KS]
    worst = {pt: (math.inf, None) for pt in points}
    emit("# RMSE over rgb against 1024 spp; columns: mean, rs_denoise defaults on the mean, then rs_denoise_var (k, levels)")
    emit("# cell".ljust(26) + "mean     denoise  " + " ".join(f"k{k:g}/L{lv}".rjust(8) for k, lv in points))
    for name in ("rtiow", "features"):
        frames, albedo, normal = V.quality_inputs(name)
        for K, N in V.QUALITY_CELLS:
            for gamma in (0, 1):
                ref = frames[gamma]["ref"]
                mean, var = V.pass_moments(frames[gamma][(K, N)], gamma)
                e_mean = rmse(mean, ref)
                e_dn = rmse(D.denoise(mean, albedo, normal, gamma=gamma), ref)
                row = []
                for k, lv in points:
                    out, _ = V.denoise_var(mean, var, albedo, normal, levels=lv, k_color=k, gamma=gamma)
                    e = rmse(out, ref)
                    row.append(e)
                    margin = 1.0 - e / min(e_mean, e_dn)
                    if margin < worst[(k, lv)][0]:
                        worst[(k, lv)] = (margin, f"{name} {K}x{N} g{gamma}")
                emit(f"{name} {K}x{N} gamma {gamma}".ljust(26) + f"{e_mean:.5f}  {e_dn:.5f}  " + " ".join(f"{e:8.5f}" for e in row))
    emit("# smallest margin over the 16 cells, 1 - rmse(denoise_var) / min(rmse(mean), rmse(denoise)), and its cell")
    for pt in points:
        emit(f"k {pt[0]:g} levels {pt[1]}: {worst[pt][0]:+.4f}  ({worst[pt][1]})")
    for lv in LEVELS:
        best = max((pt for pt in points if pt[1] == lv), key=lambda pt: worst[pt][0])
        emit(f"# largest smallest margin at levels {lv}: k {best[0]:g} ({worst[best][0]:+.4f})")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
