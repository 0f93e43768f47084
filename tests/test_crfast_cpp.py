"""The scatter math's fast paths (raysnail_amd/csrc/rs_crfast.h) without a GPU: tests/cpp/test_crfast.cpp checks that
sincos_cr_fast returns the bits of rs_crmath.h's sincos_cr on 2^28 arguments 2 pi u (u drawn as Rng::gen draws it), on
the 2,000 doubles around each k pi/2 for k = 0 .. 8, on +-0, denormals, NaN, +-inf and on arguments up to and beyond
2^20 pi/2 (where the fast path must not decide); that over the same run the fast double-double stays within M / 4 of
the full one and at most 2^-12 of the values fail the rounding test; and that sin_sign_fast / sin3_negative_fast equal
sin_sign / sin3_negative on 2^26 triples, arguments on and beside multiples of pi/2 and beyond |k| = 2^20 among them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crfast_equals_crmath(tmp_path):
    exe = tmp_path / "test_crfast"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_crfast.cpp")], check=True)
    r = subprocess.run([str(exe), "28", "26"], capture_output=True, text=True, timeout=1200)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-500:])
    assert "stream n=%d " % (1 << 28) in r.stdout and "triples n=%d " % (1 << 26) in r.stdout
