"""Registers, scratch and occupancy of the spheres unit's streaming kernels, as compiled with the flags
raysnail_amd/csrc/Makefile gives that unit (tools/regs.sh). The frame's schedule is tuned for these occupancies
(the launch bounds in rs_kernels.hip: ext_min_waves, RS_SHADE_WAVES); a change that makes a kernel spill or drop
a wave per SIMD would only show as a slower benchmark otherwise. CPU only: a cross-compile of one unit (about half
a minute)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))

pytestmark = pytest.mark.skipif(not HIPCC, reason="no hipcc")

# gfx950: 512 VGPRs per SIMD lane in units of 8 per wave -> 96 at 5 waves, 128 at 4
VGPRS_AT = {5: 96, 4: 128}
# "a few bytes" of scratch for the lean shading at its 5-wave bound: at most 8 spilled dwords per lane, under a
# quarter of the 136 B with which that bound measured 10 % slower before the unit's flags
LEAN_SCRATCH_MAX = 32


@pytest.fixture(scope="module")
def table():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "regs.sh"), "k_wfs_(extend|shade_all)", "1"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, HIPCC=HIPCC))
    assert r.returncode == 0, r.stderr[-2000:]
    ext, shade = {}, {}
    for line in r.stdout.splitlines():
        v, s, o, name = line.split()
        m = re.search(r"k_wfs_extendILi1ELb([01])ELi(\d)ELb0EE", name)
        if m:
            ext[(int(m.group(2)), int(m.group(1)))] = (int(v), int(s), int(o))
        m = re.search(r"k_wfs_shade_allILi1ELb([01])ELb0ELi(\d)EE", name)
        if m:
            shade[(int(m.group(2)), int(m.group(1)))] = (int(v), int(s), int(o))
    print(r.stdout)
    return ext, shade


def test_extend_parts_at_5_waves(table):
    """k_wfs_extend<kSmSpheres, OVF, PART, false>: the camera part (2, with its in-place shading), the carried part
    (1) and the merged kernel (0), with the LDS-only stack and with the overflow array: <= 96 VGPRs, no scratch."""
    ext, _ = table
    assert sorted(ext) == [(p, o) for p in (0, 1, 2) for o in (0, 1)], sorted(ext)
    for key, (v, s, o) in sorted(ext.items()):
        assert v <= VGPRS_AT[5] and s == 0 and o >= 5, (key, v, s, o)


def test_lean_shading_at_5_waves(table):
    """k_wfs_shade_all<kSmSpheres, false, false, 1>: 5 waves, with at most the few bytes of scratch the bound costs."""
    _, shade = table
    v, s, o = shade[(1, 0)]
    assert v <= VGPRS_AT[5] and s <= LEAN_SCRATCH_MAX and o >= 5, (v, s, o)


def test_heavy_and_unsplit_shading_at_4_waves(table):
    """The heavy launch (PS 2) and the unsplit one (PS 0), with and without the generic switch (G4): <= 128 VGPRs,
    no scratch."""
    _, shade = table
    keys = [(ps, g4) for ps in (0, 2) for g4 in (0, 1)]
    assert all(k in shade for k in keys), sorted(shade)
    for k in keys:
        v, s, o = shade[k]
        assert v <= VGPRS_AT[4] and s == 0 and o >= 4, (k, v, s, o)
