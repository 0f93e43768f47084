#!/usr/bin/env python
"""dev: what the rank-trimmed pass combine (rs_pass_robust) does to the image, on the CPU (the numpy restatements in
tests/ on oracle renders; no GPU).

Three scenes at 64 x 40, depth 8, gamma 1: RTIOW and the features scene (the two of tools/denoise_var_quality.py) and
one built here with a small bright light behind a glass sphere, the firefly case. Cells of passes x spp: 16 x 4, 32 x 2
and 8 x 8 (64 spp each), at two seeds (1 and 3, passes 0 .. K-1); the baseline is 1024 spp at seed 2; the guides are
features_ref's at 16 spp. Estimators: the plain mean (rs_pass_moments), trim 0.05, 0.1, 0.25 and the automatic trim,
each alone and after rs_denoise_var with its defaults. Metrics, all in linear radiance: RMSE over rgb; the relative
error of tools/adaptive_quality.py (root mean of |x - ref|^2 / max(L_ref, 0.03)^2); and the ratio of the mean levels,
mean(x) / mean(ref) -- the darkening: a trimmed mean of a right-skewed distribution is biased low.
Then, per estimator, the cells it wins against the plain mean after the denoiser by more than the two seeds differ.
usage: python tools/robust_quality.py [--out profiles/robust/quality.txt]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CELLS = [(16, 4), (32, 2), (8, 8)]
SEEDS = [1, 3]
ESTIMATORS = [("mean", "plain"), ("t0.05", 0.05), ("t0.1", 0.1), ("t0.25", 0.25), ("auto", None)]
FLOOR = 0.03  # RS_ADAPTIVE_FLOOR


def glass_light_scene(width, height):
    """a small light (radius 0.25, 40 x) right behind a glass sphere as the camera sees it, two diffuse spheres and a
    checker ground under a dim sky: most of the light's paths reach the diffuse surfaces through the glass"""
    from raysnail_amd import scenes as S
    from raysnail_amd.api import (CameraBuilder, Checker, Dielectric, DiffuseLight, Glass, Gradient, HittableList,
                                  Lambertian, Point3, Sphere, World)
    h = HittableList()
    h.add(Sphere((0.0, -100.0, 0.0), 100.0, Lambertian(Checker(S.C32(0.2, 0.3, 0.1), S.C32(0.9, 0.9, 0.9), 3.0))))
    h.add(Sphere((0.0, 1.0, 0.0), 1.0, Dielectric(S.C32(1.0, 1.0, 1.0), 1.5).reflect_curve(Glass())))
    h.add(Sphere((-2.2, 0.7, 1.2), 0.7, Lambertian(S.C32(0.7, 0.3, 0.1))))
    h.add(Sphere((1.8, 0.5, 2.0), 0.5, Lambertian(S.C32(0.2, 0.3, 0.8))))
    light = Sphere((-2.0, 1.6, -2.0), 0.25, DiffuseLight(S.C32(1.0, 0.9, 0.7)).multiplier(40.0))
    h.add(light)
    lights = HittableList()
    lights.add(light)
    cam = CameraBuilder().look_from(Point3(6.0, 2.2, 6.0)).look_at(Point3(0.0, 0.8, 0.0)).fov(35.0) \
        .width(width).height(height).build()
    return cam, World(h, lights, Gradient(S.C32(0.05, 0.06, 0.08), S.C32(0.1, 0.12, 0.15)), (0.0, 0.0))


def inputs(name):
    """{seed: {(K, N): K pass frames}}, the 1024-spp baseline, and the 16-spp feature frames"""
    import features_ref as FR
    from oracle.binding import OracleScene
    from raysnail_amd import scenes
    if name == "rtiow":
        cam, world, _, _ = scenes.rtow_13_1(64, 40, seed=7)
    elif name == "features":
        cam, world = scenes.features_scene(64, 40)
    else:
        cam, world = glass_light_scene(64, 40)
    orc = OracleScene(world)
    ref = orc.render(cam.desc, cam.take_photo().samples(1024).depth(8).seed(2).settings(), threads=8)[0]
    frames = {}
    for seed in SEEDS:
        frames[seed] = {}
        for K, N in CELLS:
            frames[seed][(K, N)] = [
                orc.render(cam.desc, cam.take_photo().samples(N).depth(8).seed(seed).pass_index(k).settings(), threads=8)[0]
                for k in range(K)]
    orc2, rec = FR.oracle_scene(world)
    albedo, normal, _ = FR.expected(cam.desc, cam.take_photo().samples(16).depth(8).seed(1).settings(),
                                    FR.oracle_hits(orc2), FR.Albedo(rec))
    return frames, ref, albedo, normal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import adaptive_ref as AR
    import denoise_var_ref as V
    import robust_ref as R

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def metrics(x, ref):
        a, b = AR.linear(x, 1).astype(np.float64), AR.linear(ref, 1).astype(np.float64)
        e = a - b
        return math.sqrt(float(np.mean(e * e))), AR.rel_error(x, ref, 1, FLOOR), float(a.mean() / b.mean())

    emit("# 64 x 40, depth 8, gamma 1, against 1024 spp (seed 2); per estimator: rmse rel level, alone | after rs_denoise_var")
    emit("# cut = the share of pixels with trimmed >= 1 and the mean of trimmed")
    res = {}
    for name in ("rtiow", "features", "glass_light"):
        frames, ref, albedo, normal = inputs(name)
        for K, N in CELLS:
            for seed in SEEDS:
                for label, trim in ESTIMATORS:
                    fs = frames[seed][(K, N)]
                    if trim == "plain":
                        mean, var = V.pass_moments(fs, 1)
                        trimmed = np.zeros(mean.shape[:2], np.uint8)
                    else:
                        mean, var, trimmed = R.pass_robust(fs, 1, trim)
                    den, _ = V.denoise_var(mean, var, albedo, normal, gamma=1)
                    a, d = metrics(mean, ref), metrics(den, ref)
                    res[(name, (K, N), seed, label)] = (a, d)
                    emit(f"{name:<12} {K:2d}x{N} seed {seed} {label:<6} {a[0]:8.5f} {a[1]:8.5f} {a[2]:6.3f} | "
                         f"{d[0]:8.5f} {d[1]:8.5f} {d[2]:6.3f}   cut {float((trimmed >= 1).mean()):5.3f} "
                         f"{float(trimmed.mean()):5.2f}")
    emit("# after rs_denoise_var, seed-averaged, against the plain mean: rmse ratio, rel ratio (below 1 = the estimator "
         "wins); spread = the plain mean's own |seed 1 - seed 3| / average; a win counts when 1 - ratio > spread")
    wins = {label: [0, 0] for label, _ in ESTIMATORS[1:]}
    n_cells = 0
    for name in ("rtiow", "features", "glass_light"):
        for cell in CELLS:
            n_cells += 1
            plain = [res[(name, cell, s, "mean")][1] for s in SEEDS]
            avg = [sum(p[i] for p in plain) / len(plain) for i in (0, 1)]
            spread = [abs(plain[0][i] - plain[1][i]) / avg[i] for i in (0, 1)]
            row = f"{name:<12} {cell[0]:2d}x{cell[1]} spread {spread[0]:.3f} {spread[1]:.3f} "
            for label, _ in ESTIMATORS[1:]:
                e = [sum(res[(name, cell, s, label)][1][i] for s in SEEDS) / len(SEEDS) for i in (0, 1)]
                ratio = [e[i] / avg[i] for i in (0, 1)]
                for i in (0, 1):
                    wins[label][i] += 1 if 1.0 - ratio[i] > spread[i] else 0
                row += f" {label} {ratio[0]:.3f} {ratio[1]:.3f}"
            emit(row)
    for label, _ in ESTIMATORS[1:]:
        emit(f"# {label}: wins beyond the seed spread in {wins[label][0]} (rmse) and {wins[label][1]} (rel) of {n_cells} cells")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
