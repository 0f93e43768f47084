#!/usr/bin/env python
"""dev: the quality grid behind RS_ADAPTIVE_* (tolerance, floor, radius, min passes), on the CPU (the numpy restatement
tests/adaptive_ref.py on oracle renders; no GPU).

Two scenes (RTIOW, features) at 64 x 40, depth 8, seed 1, both gammas: four cells. Per cell 32 passes of 4 spp; the
reference is 1024 spp at seed 2. Per grid point (tolerance, floor, radius, min passes) and cell: the adaptive loop with
max passes 32 on those pass frames; the total pass-pixels it spent; its mean's error; and the error of the uniform mean
of ceil(total / (W H)) passes, which never has fewer samples. Two metrics: plain RMSE over linear rgb, and the relative
error the criterion targets, the root mean of |x - ref|^2 / max(L_ref, floor)^2. margin = 1 - rel(adaptive) /
rel(uniform). The default is the point with the largest smallest margin over the four cells among the points that stop
before max passes on at least half the pixels of every cell.
usage: python tools/adaptive_quality.py [--out profiles/adaptive/quality.txt]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TOLERANCES = [0.02, 0.05, 0.1, 0.2]
FLOORS = [0.03, 0.15, 0.6]
RADII = [0, 1, 2]
MIN_PASSES = [2, 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import adaptive_ref as R

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    cells = [(name, gamma) for name in R.QUALITY_SCENES for gamma in (0, 1)]
    inputs = {c: R.quality_inputs(*c) for c in cells}
    points = [(t, f, r, m) for t in TOLERANCES for f in FLOORS for r in RADII for m in MIN_PASSES]
    wh = R.QUALITY_W * R.QUALITY_H
    emit(f"# {R.QUALITY_W} x {R.QUALITY_H}, {R.QUALITY_SPP} spp per pass, max passes {R.QUALITY_MAX_PASSES}; per cell: "
         "total pass-pixels / uniform passes / share of pixels stopped early, then adaptive | uniform in rmse and in rel")
    emit("# tol   floor r m  cell            total  uni early   rmse_a   rmse_u    rel_a    rel_u   margin")
    worst, early = {}, {}
    for pt in points:
        t, f, r, m = pt
        worst[pt], early[pt] = (math.inf, None), 1.0
        for c in cells:
            passes, ref = inputs[c]
            q = R.quality_cell(passes, ref, c[1], m, t, f, r)
            margin = 1.0 - q["rel"] / q["rel_uniform"]
            if margin < worst[pt][0]:
                worst[pt] = (margin, f"{c[0]} g{c[1]}")
            early[pt] = min(early[pt], q["early"])
            emit(f"{t:<6g} {f:<5g} {r} {m}  {c[0] + ' g' + str(c[1]):<12} {q['total']:8d} {q['uniform_passes']:4d} "
                 f"{q['early']:5.2f} {q['rmse']:8.5f} {q['rmse_uniform']:8.5f} {q['rel']:8.5f} {q['rel_uniform']:8.5f} "
                 f"{margin:+8.4f}")
    emit("# smallest margin over the four cells (relative metric), its cell, the smallest early share; * = eligible "
         "(early >= 0.5 in every cell)")
    for pt in points:
        ok = early[pt] >= 0.5
        emit(f"tol {pt[0]:g} floor {pt[1]:g} radius {pt[2]} min {pt[3]}: {worst[pt][0]:+.4f}  ({worst[pt][1]})  "
             f"early {early[pt]:.2f} {'*' if ok else ''}")
    elig = [pt for pt in points if early[pt] >= 0.5]
    if elig:
        best = max(elig, key=lambda pt: worst[pt][0])
        emit(f"# largest smallest margin among the eligible points: tol {best[0]:g} floor {best[1]:g} radius {best[2]} "
             f"min {best[3]} ({worst[best][0]:+.4f}); points that win all four cells: "
             f"{sum(1 for pt in elig if worst[pt][0] > 0)} of {len(elig)} eligible")
    else:
        emit("# no eligible point")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
