"""Guards of tests/far_worlds.py's fixtures, on the CPU and on the oracle alone: the transformed worlds commit into
the modes of the worlds they come from, the translated sphere worlds give the untranslated rays' hit flags and t1 bit
for bit, far_worlds.keeps_flags() says exactly which combinations keep the hit flags, every family of every
combination still hits something (the shares are printed), and the oracle hits on every named ray -- so that
tests/test_gpu_far_worlds.py cannot go vacuous."""
import numpy as np
import pytest

import edge_rays as E
import far_worlds as F
from raysnail_amd.api import DeviceScene


@pytest.mark.parametrize("name", F.NAMES)
def test_transformed_worlds_keep_their_modes(name):
    mode, arity, ref_order = E.EXPECT_INFO[name]
    for variant in F.VARIANTS:
        inf = DeviceScene(F.world(name, variant), devices=[]).info()
        assert (inf.scene_mode, inf.ref_order) == (mode, ref_order), (name, variant)
        if arity is not None:
            assert inf.tree_arity == arity


def test_rays_are_the_lattice_rays_mapped():
    for name in F.NAMES:
        r0 = E.rays(name)[0][F.base_rows(name)]
        assert 1200 <= len(r0) <= 2000
        for variant, (s, T) in F.VARIANTS.items():
            for dm in F.DIR_MODES:
                r, fam = F.rays(name, variant, dm)
                assert set(np.unique(fam)) == {0, 1, 2}
                assert np.array_equal((r[:, :3] - np.array(T)) / s, r0[:, :3])          # exact both ways
                assert np.array_equal(r[:, 3:6], r0[:, 3:6] * (s if dm == "dirs_scaled" else 1.0))
                assert np.array_equal(r[:, 6], r0[:, 6])


@pytest.mark.parametrize("name", ["spheres", "spheres_moving"])
def test_translated_spheres_hit_exactly_as_untranslated(name):
    """o - c is exact, so the flag and t1 are the untranslated ray's bits on every ray of every family."""
    for variant in F.TRANSLATED:
        for tmin in E.TMINS:
            ref, base = F.reference(name, variant, "dirs_scaled", tmin), F.base_reference(name, tmin)
            assert np.array_equal(E.bits(ref[:, :2]), E.bits(base[:, :2])), (variant, tmin)
            assert int(base[:, 0].sum()) >= 300


@pytest.mark.parametrize("name", F.NAMES)
def test_which_combinations_keep_the_hit_flags(name):
    """keeps_flags(), both halves, and oracle hits in every family of every combination; prints the hit shares."""
    for variant in F.VARIANTS:
        for dm in (F.DIR_MODES if variant in F.SCALED else ("dirs_scaled",)):
            assert (name, variant, dm) not in F.ORACLE_HITS_NOTHING
            fam = F.rays(name, variant, dm)[1]
            keep = np.isin(fam, F.FLAG_FAMILIES)
            for tmin in F.tmins(variant, dm):
                ref, base = F.reference(name, variant, dm, tmin), F.base_reference(name, tmin)
                assert set(np.unique(ref[:, 0])) == {0.0, 1.0}
                same = np.array_equal(ref[keep, 0], base[keep, 0])
                shares = [float(np.mean(ref[fam == f, 0])) for f in range(len(E.FAMILIES))]
                print(f"{name} {variant} {dm} tmin {tmin}: oracle hit share axis / scaled / near "
                      + " / ".join(f"{s:.3f}" for s in shares)
                      + f" (unmapped world {float(np.mean(base[:, 0])):.3f} over all; flags kept: {same})")
                assert same == F.keeps_flags(name, variant, dm), (name, variant, dm, tmin)
                assert min(shares) >= 0.05, (name, variant, dm, tmin, shares)


def test_named_rays_hit_on_the_oracle():
    from oracle.binding import OracleScene
    kinds = set()
    for case, (kind, _, _) in F.NAMED.items():
        w = F.named_world(case)
        inf = DeviceScene(w, devices=[]).info()
        assert (inf.scene_mode, inf.ref_order) == F.NAMED_INFO[kind], case
        assert inf.tree_arity == 4 and len(w.hittables.objects) == 3
        rec = E.oracle_records(OracleScene(w), F.named_ray(case), F.NAMED_TMIN)
        assert rec[0, 0] == 1.0 and np.isfinite(rec[0, 1]) and rec[0, 1] > 1.0, (case, rec[0])
        kinds.add((case[0], kind))
    assert kinds == {("A", "rects"), ("A", "spheres"), ("A", "boxes"), ("B", "spheres"), ("B", "boxes"),
                     ("C", "rects"), ("C", "boxes")}


@pytest.mark.parametrize("name", F.FRAME_NAMES)
def test_frame_camera_sees_the_translated_world(name):
    """The 2^29 frame's camera is well defined and its paths do hit the world (more world.hit calls than samples)."""
    cam = F.frame_camera(name)
    photo = cam.take_photo().samples(4).depth(4).seed(7)
    ref, stats = F.oracle(name, F.FRAME_VARIANT).render(cam.desc, photo.settings(), threads=4)
    assert ref.shape[:2] == (6, 8) and np.isfinite(ref).all()
    assert stats.segments > 8 * 6 * 4 * 1.2, stats.segments
