#!/usr/bin/env python
"""dev: do specular-chain guides (rs_render_features_specular) denoise better than first-hit guides? On the CPU: the
numpy restatements in tests/ on oracle renders; no GPU.

Scenes at 64 x 40, depth 8, both gammas: RTIOW 13.1, the features scene (DESIGN section 13's two) and the book-2 final
scene (all_feature_scene). The noisy input is 16 spp at seed 1 and, for the spread between seeds, again at seed 3:
one 16-spp frame for rs_denoise (denoise_ref, defaults) and the moments of 4 passes of 4 spp for rs_denoise_var
(denoise_var_ref, defaults). The reference is 1024 spp at seed 2. Guide sets at 16 spp, seed 1: first hit
(max_specular 0) and the chain at max_specular 1 / 2 / 4 / 8 (tests/spec_features_ref.py). RMSE over rgb against the
reference over two regions: the whole frame, and the specular-first pixels -- those where at least half the samples
bounce at least once under the max_specular = 8 restatement.
usage: python tools/spec_features_quality.py [--out profiles/spec_features/quality.txt] [--scenes rtiow,features,all]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BUDGETS = [0, 1, 2, 4, 8]
W, H = 64, 40


def rmse(a, b, where):
    import numpy as np
    e = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return math.sqrt(float(np.mean((e * e)[where])))


def scene(name):
    from raysnail_amd import scenes
    if name == "rtiow":
        return scenes.rtow_13_1(W, H, seed=7)[:2]
    if name == "features":
        return scenes.features_scene(W, H)
    return scenes.all_feature_scene(W, H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="rtiow,features,all")
    args = ap.parse_args()
    import numpy as np
    import denoise_ref as D
    import denoise_var_ref as V
    import features_ref as F
    import spec_features_ref as R
    from oracle.binding import OracleScene

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# RMSE over rgb against 1024 spp (seed 2); noisy input 16 spp; guides at 16 spp, seed 1; columns: the input, then")
    emit("# the denoiser's output under first-hit guides (m0) and chain guides at max_specular 1 / 2 / 4 / 8")
    emit("# cell".ljust(44) + "input    " + " ".join(f"m{m}".rjust(8) for m in BUDGETS))
    verdict = []
    for name in args.scenes.split(","):
        cam, world = scene(name)
        orc2, rec = R.oracle_scene(world)
        alb = F.Albedo(rec)
        bouncer = R.Bouncer(alb)
        lo = cam.take_photo().samples(16).depth(8).seed(1)
        chains = {m: R.chains(cam.desc, lo.settings(), F.oracle_hits(orc2), alb, m, bouncer=bouncer) for m in BUDGETS}
        guides = {m: ch.frames() for m, ch in chains.items()}
        spec_first = ((chains[8].bounces >= 1).mean(axis=1) >= 0.5).reshape(H, W)
        emit(f"# {name}: {int(spec_first.sum())} specular-first pixels of {W * H}; mean World::hit calls per sample at "
             + ", ".join(f"m{m} {chains[m].calls.mean():.3f}" for m in (1, 8)))
        orc = OracleScene(world)
        regions = (("whole", np.ones((H, W), bool)), ("specular-first", spec_first))
        for gamma in (0, 1):
            ref = orc.render(cam.desc, cam.take_photo().samples(1024).depth(8).seed(2).gamma(bool(gamma)).settings(),
                             threads=8)[0]
            rows = {}
            for seed in (1, 3):
                one = orc.render(cam.desc, cam.take_photo().samples(16).depth(8).seed(seed).gamma(bool(gamma)).settings(),
                                 threads=8)[0]
                passes = [orc.render(cam.desc, cam.take_photo().samples(4).depth(8).seed(seed).gamma(bool(gamma))
                                     .pass_index(k).settings(), threads=8)[0] for k in range(4)]
                mean, var = V.pass_moments(passes, gamma)
                outs = {"denoise": (one, [D.denoise(one, *guides[m], gamma=gamma) for m in BUDGETS]),
                        "denoise_var": (mean, [V.denoise_var(mean, var, *guides[m], gamma=gamma)[0] for m in BUDGETS])}
                for dn, (inp, res) in outs.items():
                    for rname, where in regions:
                        if not where.any():
                            continue
                        row = [rmse(inp, ref, where)] + [rmse(o, ref, where) for o in res]
                        rows[(dn, rname, seed)] = row
                        emit(f"{name} g{gamma} {dn} {rname} seed {seed}".ljust(44) + " ".join(f"{e:8.5f}" for e in row))
            for dn in ("denoise", "denoise_var"):
                if (dn, "specular-first", 1) not in rows:
                    continue
                a, b = rows[(dn, "specular-first", 1)], rows[(dn, "specular-first", 3)]
                spread = abs(a[1] - b[1])  # first-hit guides, the two seeds of the noisy input
                for k, m in enumerate(BUDGETS[1:], start=2):
                    gain = min(a[1] - a[k], b[1] - b[k])  # the smaller gain of the two seeds (negative: a loss)
                    verdict.append((name, gamma, dn, m, gain, spread))
    emit("# specular-first pixels: gain = rmse(first-hit guides) - rmse(chain guides), the smaller of the two seeds'; spread =")
    emit("# |rmse(seed 1) - rmse(seed 3)| under first-hit guides. `+` the gain exceeds the spread, `-` a loss, `~` inside it")
    for name, gamma, dn, m, gain, spread in verdict:
        mark = "+" if gain > spread else ("-" if gain < 0 else "~")
        emit(f"{name} g{gamma} {dn} m{m}: gain {gain:+.5f} spread {spread:.5f} {mark}")
    for m in BUDGETS[1:]:
        v = [x for x in verdict if x[3] == m]
        emit(f"# max_specular {m}: {sum(1 for x in v if x[4] > x[5])} of {len(v)} cells gain more than the spread, "
             f"{sum(1 for x in v if x[4] < 0)} lose; smallest gain {min(x[4] for x in v):+.5f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
