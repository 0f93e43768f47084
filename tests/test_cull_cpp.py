"""The f32 cull of the tree walks (raysnail_amd/csrc/rs_cull.h: make_rayf, slab32, make_rayf4, slab4 and the outward
rounding of the node planes) without a GPU: tests/cpp/test_cull.cpp checks on about 10 million seeded cases that
whatever the exact f64 test slab64 accepts, both f32 tests accept on the outward-rounded box and on a strictly larger
one, with an entry that is not NaN, and that slab4 equals slab32 -- over box, origin and direction scales 2^-140 ..
2^140, zero-thickness and thin boxes, rays aimed at corners, edges, faces and interior points, origins on box planes,
direction components that are +-0, 2^-100 .. 2^-136, in (1e-38, 1e-30) or NaN, tmin 0 / 1e-4 / 0.5 and range ends
+inf or on either side of the aimed point. Every family must have at least 10 % exact accepts; the three classes of
misses the test was written for (profiles/cull/README.md) are checked by name."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("wide +-140", "mid +-30", "zero-thick", "thin axis", "on a plane", "d = +-0", "d = +-0 far", "d tiny",
            "d tiny far", "clamp band", "band far", "d = NaN")
HAND = ("A, product overflows, 2^30", "A, product overflows, 2^29", "A, product overflows, 2^28",
        "B, origin beyond FLT_MAX, +", "B, origin beyond FLT_MAX, -", "C, clamp band")


def test_cull_never_rejects_what_the_exact_test_accepts(tmp_path):
    exe = tmp_path / "test_cull"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_cull.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-500:])
    assert "FAILED" not in r.stdout
    total = 0
    for fam in FAMILIES:
        m = re.search(r"^%s +(\d+) cases, +(\d+) exact accepts \( *[\d.]+ %%\), missed by slab32 (\d+), by slab4 (\d+), "
                      r"NaN entries (\d+), slab4 != slab32 (\d+) " % re.escape(fam), r.stdout, flags=re.M)
        assert m, fam
        n, acc, m32, m4, nan, diff = map(int, m.groups())
        assert (m32, m4, nan, diff) == (0, 0, 0, 0), (fam, m.group(0))
        assert acc * 10 >= n, (fam, acc, n)
        total += n
    assert 9_000_000 <= total <= 12_000_000, total
    for name in HAND:
        assert re.search(r"^hand case %s +exact 1 slab32 1 slab4 1$" % re.escape(name), r.stdout, flags=re.M), name
