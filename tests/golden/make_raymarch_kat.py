"""Writes tests/golden/raymarch_kat.json: known answers for RayMarcher (the Mandelbulb object) from the pure-Python
restatement tests/raymarch_ref.py, evaluated with every transcendental rounded once from 256 bits (Exact).

    python tests/golden/make_raymarch_kat.py        (about a minute; needs mpmath)

Ray records: "ray" (o(3) d(3) time), "tmin", "exp" (World::hit of a world holding the marcher alone with material
id 0, in rs_probe_world_hit's layout: hit t1 t2 p(3) n(3) u v outside mat; u = v = 0) and "obj_t1" (t1 of
RayMarcher::hit alone, NaN for a miss: the BVH leaf's bbox test can reject a ray the object itself would accept).
Point records: "p", "contains", "dist" (distance_est). Doubles are hex bit patterns; a NaN equals any NaN.

A ray is kept only if the glibc `math` evaluation of the same restatement (Libm) takes the same hit / miss decision
with t1 within 2^-40 relative (the tolerance of test_per_sample_radiance_vs_oracle) and the normal is finite;
otherwise the next candidate of the seeded stream replaces it, and at most 10 % of a group may be replaced.
"""
import json
import math
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import raymarch_ref as R  # noqa: E402

TMIN = 0.0001
EXACT, LIBM = R.Exact(), R.Libm()
CAM = (13.0 * 0.7, -1.7 * 0.7, 3.0 * 0.7)  # preview_sdl2.rs:338-406 look_from


def evaluate(ray, tmin):
    """-> (record, obj_t1, ok): ok when Libm agrees and the normal is finite"""
    rec, t1 = R.record(EXACT, ray, tmin)
    t1l = R.hit_t(LIBM, ray[0:3], ray[3:6], tmin)
    ok = (t1 is None) == (t1l is None)
    if ok and t1 is not None:
        ok = abs(t1 - t1l) <= 2.0 ** -40 * abs(t1)
    if rec[0] == 1.0:
        ok = ok and all(math.isfinite(c) for c in rec[6:9])
    return rec, t1, ok


def group(name, candidates, count, tmin=TMIN, accept=lambda rec, t1: True, must_keep=0):
    """the first `count` candidates that pass; the first `must_keep` candidates may not be replaced"""
    out, replaced = [], 0
    for k, ray in enumerate(candidates):
        rec, t1, ok = evaluate(ray, tmin)
        if ok and accept(rec, t1):
            out.append({"g": name, "ray": ray, "tmin": tmin, "exp": rec, "obj_t1": R.NAN if t1 is None else t1})
        else:
            assert k >= must_keep, (name, k, "a fixed ray breaks a condition")
            replaced += 1
        if len(out) == count:
            break
    assert len(out) == count, (name, len(out))
    assert replaced * 10 <= count, (name, replaced)
    print(f"group {name}: {count} rays, {sum(1 for r in out if r['exp'][0] == 1.0)} hits, {replaced} replaced")
    return out


def stream(rng, make):
    while True:
        yield make(rng)


def main():
    rng = random.Random(338406)
    u = lambda a, b: rng.uniform(a, b)  # noqa: E731
    box = lambda: (u(-1.3, 1.3), u(-1.3, 1.3), u(-1.3, 1.3))  # noqa: E731

    def toward(o, t):
        return [o[0], o[1], o[2], t[0] - o[0], t[1] - o[1], t[2] - o[2], 0.0]

    rays = []
    A = group("A", stream(rng, lambda _: toward(CAM, box())), 48)
    hits = sum(1 for r in A if r["exp"][0] == 1.0)
    assert 4 * hits >= len(A) and 4 * (len(A) - hits) >= len(A), hits
    rays += A

    def scaled(r, s):
        return r["ray"][0:3] + [c * s for c in r["ray"][3:6]] + [0.0]
    # B: rays of A (hits first, so the scaling has something to change), x0.25 and x3
    pick = [r for r in A if r["exp"][0] == 1.0][:6] + [r for r in A if r["exp"][0] == 0.0][:6]
    B = group("B", (scaled(r, 0.25) for r in pick), 8) + group("B", (scaled(r, 3.0) for r in pick), 8)
    rays += B

    def outside_in_box(_):
        while True:
            o = box()
            if not R.is_inside(EXACT, o) and not R.is_inside(LIBM, o):
                return toward(o, box())
    rays += group("C", stream(rng, outside_in_box), 8)

    def inside_set(_):
        while True:
            o = (u(-0.9, 0.9), u(-0.9, 0.9), u(-0.9, 0.9))
            if R.is_inside(EXACT, o) and R.is_inside(LIBM, o):
                return toward(o, (u(-3.0, 3.0), u(-3.0, 3.0), u(-3.0, 3.0)))

    def d_candidates():
        yield [0.0, 0.0, 0.0, 0.3, -0.4, 1.2, 0.0]
        yield from stream(rng, inside_set)
    rays += group("D", d_candidates(), 4, must_keep=1)

    def far(_):
        while True:
            d = (u(-1.0, 1.0), u(-1.0, 1.0), u(-1.0, 1.0))
            n = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            if n > 0.2:
                o = tuple(-12.0 * c / n for c in d)
                return toward(o, (0.0, 0.0, 0.0))
    E = group("E", stream(rng, far), 4)
    assert all(r["exp"][0] == 0.0 for r in E)
    rays += E

    # F: rays of B at tmin = 2.0: RayMarcher::hit compares the LENGTH with tmin (:141), so the x3 rays (t1 < 2 <
    # length) are hits of the object; World::hit still misses them, because the leaf's bbox test reads t
    b_hits = [r for r in B if r["obj_t1"] == r["obj_t1"]]
    quirk = [r for r in b_hits if r["obj_t1"] < 2.0][:2]
    plain = [r for r in b_hits if r["obj_t1"] > 2.0][:2]
    assert len(quirk) == 2 and len(plain) == 2
    F = group("F", (r["ray"] for r in quirk + plain), 4, tmin=2.0, must_keep=4)
    assert [r["exp"][0] for r in F] == [0.0, 0.0, 1.0, 1.0] and all(r["obj_t1"] == r["obj_t1"] for r in F)
    rays += F

    def grid(_):
        o = tuple(rng.randrange(-3 * 1024, 3 * 1024 + 1) / 1024.0 for _ in range(3))
        return toward(o, box())
    H = group("H", stream(rng, grid), 16)
    assert 2 <= sum(1 for r in H if r["exp"][0] == 1.0) <= 14
    rays += H

    # G: points. A far one (escape in iteration 0: NaN), the z axis (atan2(0, 0)), (-1, 0, 0), negative zeros, the
    # origin, and seeded points in and around the set
    pts = [(5.0, -4.0, 3.0), (0.0, 0.0, 0.5), (0.0, 0.0, -0.75), (0.0, 0.0, 1.25), (-0.0, 0.0, 0.9), (-1.0, 0.0, 0.0),
           (-1.0, -0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, 0.0, 0.0), (0.5, -0.0, 0.25), (-0.0, 0.7, -0.0), (1.0, 0.0, 0.0),
           (0.0, 1.0, 0.0), (0.0, -1.0, -0.0), (2.0, 2.0, 0.1), (1.5, 0.0, 0.0)]
    while len(pts) < 32:
        pts.append(box())
    points = []
    for p in pts:
        inside, dist = R.is_inside(EXACT, p), R.distance_est(EXACT, p)
        assert inside == R.is_inside(LIBM, p), p
        points.append({"g": "G", "p": list(p), "contains": int(inside), "dist": dist})
    assert any(q["dist"] != q["dist"] for q in points) and 4 <= sum(q["contains"] for q in points) <= 28
    print(f"group G: {len(points)} points, {sum(q['contains'] for q in points)} inside")

    def hx(v):
        return [R.to_hex(x) for x in v]
    doc = {"about": "RayMarcher known answers; see tests/golden/make_raymarch_kat.py",
           "rays": [{"g": r["g"], "ray": hx(r["ray"]), "tmin": R.to_hex(r["tmin"]), "exp": hx(r["exp"]),
                     "obj_t1": R.to_hex(r["obj_t1"])} for r in rays],
           "points": [{"g": q["g"], "p": hx(q["p"]), "contains": q["contains"], "dist": R.to_hex(q["dist"])}
                      for q in points]}
    path = os.path.join(HERE, "raymarch_kat.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    assert os.path.getsize(path) < 100 * 1024
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
