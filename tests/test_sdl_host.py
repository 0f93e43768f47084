"""C++ host layer (libraysnail_host.so): the SDL front end (src/sdl_parser.rs restated in
raysnail_amd/host/sdl_parser.cpp) and the object export into scene sinks. CPU only.

A recording sink (Python callbacks in the rsh_sink_api table) captures the exact call sequence a
file produces, so the parser's decisions are checked call by call; whole scenes are checked by
rendering them on the CPU oracle next to the hand-built Python scenes of the same files.
"""
import ctypes as C
import os

import numpy as np
import pytest

from raysnail_amd import _abi as A
from raysnail_amd import host_lib, scenes

REF_SDL = "/root/reference/sdl"
GOLDEN_SDL = os.path.join(os.path.dirname(__file__), "golden", "sdl")


class RecordingSink:
    """rsh_sink_api whose entries append (call, args) to self.calls and hand out handles."""

    def __init__(self):
        self.calls = []
        self.mats = []
        self._keep = []
        api = host_lib.rsh_sink_api()
        I, U, D = C.c_int, C.c_uint32, C.c_double
        DP, FP = C.POINTER(C.c_double), C.POINTER(C.c_float)

        def reg(name, restype, argtypes, fn):
            cb = C.CFUNCTYPE(restype, *argtypes)(fn)
            self._keep.append(cb)
            setattr(api, name, C.cast(cb, C.c_void_p).value)

        def handle():
            return len([c for c in self.calls if c[0] in ("sphere", "aarect", "box", "quadric", "intersection",
                                                            "difference", "transformed")]) - 1

        def mat(s, d, out):
            d = d.contents
            self.mats.append((d.kind, tuple(d.texture.even[:3]), tuple(d.texture.odd[:3]), d.texture.kind,
                              d.texture.scale, d.exponent, d.mix_a, d.mix_b, d.mix_p, d.phong_factor,
                              d.phong_exponent))
            self.calls.append(("material", len(self.mats) - 1))
            out[0] = len(self.mats) - 1
            return 0

        def obj(name, nargs):
            def f(s, *a):
                out = a[-1]
                self.calls.append((name,) + tuple(a[:-1]))
                out[0] = handle()
                return 0
            return f

        def sphere(s, c, r, v, m, out):
            self.calls.append(("sphere", tuple(c[:3]), r, m))
            out[0] = handle()
            return 0

        def box(s, p0, p1, m, out):
            self.calls.append(("box", tuple(p0[:3]), tuple(p1[:3]), m))
            out[0] = handle()
            return 0

        def quadric(s, q, m, out):
            self.calls.append(("quadric", tuple(q[:10]), m))
            out[0] = handle()
            return 0

        def transformed(s, o, st, n, out):
            self.calls.append(("transformed", o, tuple((st[i].kind, tuple(st[i].v[:3])) for i in range(n))))
            out[0] = handle()
            return 0

        def csg(name):
            def f(s, a, b, m, out):
                self.calls.append((name, a, b, m))
                out[0] = handle()
                return 0
            return f

        def simple(name):
            def f(s, *a):
                self.calls.append((name,) + tuple(a))
                return 0
            return f

        P = C.c_void_p
        reg("material", I, [P, C.POINTER(A.rs_material_desc), C.POINTER(C.c_int32)], mat)
        reg("sphere", I, [P, DP, D, DP, C.c_int32, C.POINTER(U)], sphere)
        reg("aarect", I, [P, C.c_int32, D, D, D, D, D, C.c_int32, C.POINTER(U)], obj("aarect", 8))
        reg("box", I, [P, DP, DP, C.c_int32, C.POINTER(U)], box)
        reg("quadric", I, [P, DP, C.c_int32, C.POINTER(U)], quadric)
        reg("triangles", I, [P, DP, DP, U, C.c_int32, C.POINTER(U)], obj("triangles", 5))
        reg("intersection", I, [P, U, U, C.c_int32, C.POINTER(U)], csg("intersection"))
        reg("difference", I, [P, U, U, C.c_int32, C.POINTER(U)], csg("difference"))
        reg("transformed", I, [P, U, C.POINTER(A.rs_transform), U, C.POINTER(U)], transformed)
        reg("world_add", I, [P, U], simple("world_add"))
        reg("lights_add", I, [P, U], simple("lights_add"))
        reg("set_background", I, [P, FP, FP], lambda s, lo, hi: self.calls.append(
            ("set_background", tuple(lo[:3]), tuple(hi[:3]))) or 0)
        reg("set_time_range", I, [P, D, D], simple("set_time_range"))
        reg("last_error", C.c_char_p, [], lambda: b"recording sink")
        self.api = api

    def of(self, name):
        return [c for c in self.calls if c[0] == name]


def record_text(tmp_path, text, w=64, h=40):
    p = tmp_path / "scene.sdl"
    p.write_text(text)
    rec = RecordingSink()
    cam = host_lib.sdl_build(str(p), w, h, rec.api, C.c_void_p(1))
    return rec, cam


def build_error(tmp_path, text):
    p = tmp_path / "bad.sdl"
    p.write_text(text)
    with pytest.raises(host_lib.HostError) as e:
        host_lib.sdl_build(str(p), 8, 8, RecordingSink().api, C.c_void_p(1))
    return e.value


CAM = "camera { location <1, 2, 3> look_at <0, 0, 0> angle 40 }\n"


def test_host_library_exports():
    lib = host_lib.load()
    for sym in ("rsh_sdl_build", "rsh_sdl_render", "rsh_last_error"):
        assert hasattr(lib, sym)


def test_camera_light_and_cli_conventions(tmp_path):
    rec, cam = record_text(tmp_path, CAM + "light { <10, 20, 30>, color rgb <1, 0.9, 0.7> }\n", 320, 200)
    assert list(cam.look_from) == [1, 2, 3] and list(cam.look_at) == [0, 0, 0]
    assert (cam.fov, cam.aperture, cam.focus, cam.width, cam.height) == (40.0, 0.01, 10.0, 320, 200)
    # raysnail.rs:351-373: light -> Sphere(loc, 12, DiffuseLight x1.7) in lights and world; gradient sky
    assert rec.of("set_background")[0][1:] == (tuple(np.float32([0.3, 0.4, 0.5])), tuple(np.float32([0.7, 0.89, 1.0])))
    s = rec.of("sphere")
    assert len(s) == 2 and s[0][1:3] == ((10.0, 20.0, 30.0), 12.0)
    assert rec.mats[s[0][3]][0] == A.RS_MAT_DIFFUSE_LIGHT
    assert len(rec.of("world_add")) == 1 and len(rec.of("lights_add")) == 1
    default_fov = record_text(tmp_path, "camera { location <1, 2, 3> }")[1]
    assert default_fov.fov == 60.0 and list(default_fov.look_at) == [0, 0, 0]  # sdl_parser.rs:452-456


def test_expressions_and_declares(tmp_path):
    rec, _ = record_text(tmp_path, CAM + """
        #declare A = 2;
        #declare B = (A + 1) * 3 - 4 / 2;
        sphere { <-A, -(1 + 2) * 2, B / 7 - 1 + 0.5>, 0.5 * A }
    """)
    (_, c, r, m), = rec.of("sphere")
    assert c == (-2.0, -6.0, 7.0 / 7 - 1 + 0.5) and r == 1.0 and m == -1  # no texture -> None (world default)
    # unary minus only on an expression's first term (sdl_parser.rs:1290-1306): "1 - -1" is not a number
    assert "expected an expression" in str(build_error(tmp_path, CAM + "sphere { <0, 0, 1 - -1>, 1 }"))


def test_textures_finishes_and_surfaces(tmp_path):
    rec, _ = record_text(tmp_path, CAM + """
        sphere { <0,0,0>, 1 texture { pigment { color rgb <0.5, 0.25, 0.125> } } }
        sphere { <0,0,0>, 1 texture { pigment { checker color rgb <1,0,0>, color rgb <0,0,1> } } }
        sphere { <0,0,0>, 1 texture { finish { phong 0.5 phong_size 55 } } }
        sphere { <0,0,0>, 1 texture { pigment { color <0.2, 0.2, 0.2> } finish { reflection 0.25 } } }
        sphere { <0,0,0>, 1 texture { surface { metallic } } }
        sphere { <0,0,0>, 1 texture { surface { metallic diffuse 300 } } }
        sphere { <0,0,0>, 1 texture { surface { } } }
    """)
    k = [rec.mats[s[3]] for s in rec.of("sphere")]
    assert k[0][0] == A.RS_MAT_LAMBERTIAN and k[0][1] == (0.5, 0.25, 0.125)
    assert k[1][3] == A.RS_TEX_CHECKER and k[1][4] == 2.0 and k[1][2] == (1, 0, 0) and k[1][1] == (0, 0, 1)
    assert k[2][0] == A.RS_MAT_LAMBERTIAN and k[2][1] == (1, 1, 1) and k[2][9] == 2.0 and k[2][10] == 5
    mixed = k[3]
    assert mixed[0] == A.RS_MAT_MIXED and mixed[8] == 0.25
    assert rec.mats[mixed[6]][0] == A.RS_MAT_METAL and rec.mats[mixed[7]][0] == A.RS_MAT_LAMBERTIAN
    assert k[4][0] == A.RS_MAT_METAL
    assert k[5][0] == A.RS_MAT_DIFFUSE_METAL and k[5][5] == 300.0
    assert k[6][0] == A.RS_MAT_LAMBERTIAN


def test_modifiers_order_and_units(tmp_path):
    rec, _ = record_text(tmp_path, CAM + """
        box { <0,0,0> <1,1,1> rotate <90, 0, 30> scale 2 translate <1, 2, 3> scale <1, 2, 3> }
    """)
    (_, child, st), = rec.of("transformed")
    pi = np.pi
    assert st == ((A.RS_TF_ROTATE_X, (90 * pi / 180, 0, 0)), (A.RS_TF_ROTATE_Z, (30 * pi / 180, 0, 0)),
                  (A.RS_TF_SCALE, (2.0, 2.0, 2.0)), (A.RS_TF_TRANSLATE, (1.0, 2.0, 3.0)),
                  (A.RS_TF_SCALE, (1.0, 2.0, 3.0)))
    (_, p0, p1, _), = rec.of("box")        # corners without a separating comma (expect is silent)
    assert p0 == (0, 0, 0) and p1 == (1, 1, 1)


def test_quadric_coefficient_map(tmp_path):
    rec, _ = record_text(tmp_path, CAM + "quadric { <1, 2, 3>, <4, 5, 6>, <7, 8, 9>, 10 }")
    (_, q, _), = rec.of("quadric")
    # sdl_parser.rs:660: Quadric::new(v1.x, v2.x, v2.y, v3.x, v1.y, v2.z, v3.y, v1.z, v3.z, j)
    assert q == (1, 4, 5, 7, 2, 6, 8, 3, 9, 10)


def test_csg_and_object_instancing(tmp_path):
    rec, _ = record_text(tmp_path, CAM + """
        #declare THING = intersection { sphere { <0,0,0>, 1 } box { <-1,-1,-1>, <1,1,1> } }
        #declare n = 0;
        #while (n < 3)
          object { THING translate <n, 0, 0> }
          #declare n = n + 1;
        #end
        difference { box { <0,0,0>, <1,1,1> } sphere { <1,1,1>, 0.5 } }
    """)
    inter = rec.of("intersection")
    assert len(inter) == 1                       # the declared object is shared (Arc clone)
    tfs = rec.of("transformed")
    assert [t[2][0][1][0] for t in tfs] == [0.0, 1.0, 2.0] and len({t[1] for t in tfs}) == 1
    assert len(rec.of("difference")) == 1
    assert len(rec.of("world_add")) == 4         # 3 instances + the difference (no lights)


def test_while_false_skips_body(tmp_path):
    rec, _ = record_text(tmp_path, CAM + "#while (3 < 2) sphere { <0,0,0>, 1 } #end sphere { <5,5,5>, 2 }")
    (_, c, r, _), = rec.of("sphere")
    assert c == (5, 5, 5) and r == 2


@pytest.mark.parametrize("text", [
    CAM + "cylinder { <0,0,0>, 1 }",                 # unknown statement
    CAM + "sphere { <0,0,0>, 1 texture { surface { metallic diffuse 1 + 2 } } }",  # parse_float, then '+'
    "camera { location <1,2,3> up <0,1,0> }",       # unknown camera item
])
def test_parse_errors(tmp_path, text):
    e = build_error(tmp_path, text)
    assert e.code == A.RS_E_INVALID and "Parse error" in str(e)


@pytest.mark.parametrize("text,msg", [
    (CAM + "sphere { 1, 2 }", "expected a vector"),   # parse_vector(..).unwrap() panics upstream
    (CAM + "object { NOPE }", "undeclared"),
    (CAM + "#end", "#end without #while"),
    ("sphere { <0,0,0>, 1 }", "no camera"),           # scene_data.camera.unwrap() in the CLI
])
def test_reference_panics_become_errors(tmp_path, text, msg):
    assert msg in str(build_error(tmp_path, text))


def test_missing_file():
    with pytest.raises(host_lib.HostError, match="cannot read"):
        host_lib.sdl_build("/nonexistent.sdl", 8, 8, RecordingSink().api, C.c_void_p(1))


def _lam(r, g, b):
    return scenes.Lambertian(scenes.C32(r, g, b))


def _spheres_boxes(width, height):
    """tests/golden/sdl/spheres_boxes.sdl through the Python API, with the CLI's camera and light
    conventions (scenes._cli_camera / _cli_world), the way scenes.example_sdl is built."""
    S, B = scenes.Sphere, scenes.Box
    cam = scenes._cli_camera(scenes.Point3(5.5, 1.75, -3.25), scenes.Point3(0.25, -0.5, 0.5), 48.0, width, height)
    h = scenes.HittableList()
    h.add(S((-0.6, 0.1, 0.4), 0.9, _lam(0.2, 0.65, 0.85)))
    h.add(S((1.4, -0.35, -1.1), 0.55, _lam(0.85, 0.25, 0.35)))
    h.add(S((0.9, 0.9, 1.8), 0.4, _lam(0.9, 0.8, 0.2)))
    h.add(B((-2.75, -0.9, 1.5), (-1.25, 0.35, 2.25), _lam(0.5, 0.2, 0.7)))
    h.add(B((2.0, -0.9, 0.5), (2.5, -0.15, 1.75), _lam(0.15, 0.55, 0.3)))
    h.add(B((-4.5, -1.1, -5.0), (4.5, -0.9, 5.0),
            scenes.Lambertian(scenes.sdl_checker(scenes.C32(0.45, 0.4, 0.35), scenes.C32(0.02, 0.03, 0.04)))))
    h.add(S((0.0, -5001.5, 0.0), 5000.0, _lam(0.1, 0.09, 0.07)))
    return cam, scenes._cli_world(h, [((-220.0, 360.0, -140.0), scenes.C32(0.95, 1.0, 0.85))], cam)


def _clipped_quadrics(width, height):
    """tests/golden/sdl/clipped_quadrics.sdl through the Python API, the way scenes.quadric_sdl is built."""
    cam = scenes._cli_camera(scenes.Point3(8.5, 3.0, -5.0), scenes.Point3(0.5, 0.0, 0.5), 42.0, width, height)
    h = scenes.HittableList()
    specs = [
        (((0.25, 1.0, 0.4375), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), -1.0), ((-2.5, -0.5, -2.0), (2.5, 1.5, 2.0)),
         (0.75, 0.35, 0.3), (-1.5, 0.5, 2.5)),
        (((1.0, 0.0, 1.0), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), 0.0), ((-1.5, -0.25, -1.5), (1.5, 1.5, 1.5)),
         (0.3, 0.6, 0.8), (2.0, -1.0, 0.5)),
        (((1.0, 1.0, 0.0), (0.5, 0.0, 0.0), (0.0, 0.0, 0.0), -0.5), ((-1.5, -1.5, -1.25), (1.5, 1.5, 1.25)),
         (0.55, 0.75, 0.35), (0.0, 0.75, -2.5)),
    ]
    for (v1, v2, v3, j), (b0, b1), col, tr in specs:
        inter = scenes.Intersection(scenes._quad(v1, v2, v3, j), scenes.Box(b0, b1, None), _lam(*col))
        h.add(scenes._translated(inter, tr))
    h.add(scenes.Box((-5.0, -1.25, -6.0), (5.0, -1.0, 6.0),
                     scenes.Lambertian(scenes.sdl_checker(scenes.C32(0.35, 0.35, 0.4), scenes.C32(0.02, 0.02, 0.02)))))
    h.add(scenes.Sphere((0.0, -8001.25, 0.0), 8000.0, _lam(0.06, 0.07, 0.05)))
    return cam, scenes._cli_world(h, [((80.0, 260.0, -150.0), scenes.C32(1.0, 0.95, 0.8))], cam)


@pytest.mark.parametrize("name,build", [
    ("spheres_boxes", lambda: _spheres_boxes(64, 40)),
    ("clipped_quadrics", lambda: _clipped_quadrics(64, 40)),
])
def test_sdl_files_match_python_scenes(oracle_lib, name, build):
    """The C++ front end on a scene file == the same scene built by hand through the Python API with the helpers
    that scenes.example_sdl / quadric_sdl (configs C2 / C4) are built from, bit for bit on the oracle. The files
    are this repository's own, so this runs everywhere; test_reference_sdl_files_match_python_scenes below does
    the same on the reference's sdl/*.sdl, which are scene programs and are not stored here."""
    from oracle.binding import OracleScene
    path = os.path.join(GOLDEN_SDL, name + ".sdl")
    sc = OracleScene(fill=lambda api, h: host_lib.sdl_build(path, 64, 40, api, h))
    cam, world = build()
    photo = cam.take_photo().samples(4).depth(8).seed(3)
    a, sa = sc.render(sc.fill_result, photo.settings(), threads=8)
    b, sb = OracleScene(world).render(cam.desc, photo.settings(), threads=8)
    assert sa.segments == sb.segments and np.array_equal(a, b)
    assert sa.segments > 64 * 40 * 4 and a[..., :3].std() > 0.05   # the frame shows the scene, not one colour


@pytest.mark.skipif(not os.path.isdir(REF_SDL), reason="reference checkout not present")
@pytest.mark.parametrize("name,build", [
    ("example", lambda: scenes.example_sdl(64, 40)),
    ("quadric", lambda: scenes.quadric_sdl(64, 40, cornell_emitter=False)),
])
def test_reference_sdl_files_match_python_scenes(oracle_lib, name, build):
    """The C++ front end on the reference's own scene files == the hand-translated Python scenes
    (used for configs C2 / C4), bit for bit on the oracle."""
    from oracle.binding import OracleScene
    path = os.path.join(REF_SDL, name + ".sdl")
    sc = OracleScene(fill=lambda api, h: host_lib.sdl_build(path, 64, 40, api, h))
    cam, world = build()
    photo = cam.take_photo().samples(4).depth(8).seed(3)
    a, sa = sc.render(sc.fill_result, photo.settings(), threads=8)
    b, sb = OracleScene(world).render(cam.desc, photo.settings(), threads=8)
    assert sa.segments == sb.segments and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["spheres_boxes", "clipped_quadrics", "features", "loops"])
def test_sdl_fixture_files_parse(name):
    rec = RecordingSink()
    cam = host_lib.sdl_build(os.path.join(GOLDEN_SDL, name + ".sdl"), 64, 40, rec.api, C.c_void_p(1))
    assert cam.fov > 0 and len(rec.of("world_add")) > 1 and len(rec.of("lights_add")) >= 1


@pytest.mark.parametrize("name", ["features", "loops"])
def test_fixture_scenes_on_oracle(oracle_lib, name):
    from oracle.binding import OracleScene
    path = os.path.join(GOLDEN_SDL, name + ".sdl")
    sc = OracleScene(fill=lambda api, h: host_lib.sdl_build(path, 48, 30, api, h))
    st = A.rs_render_settings()
    st.samples, st.depth, st.gamma, st.seed, st.row_step = 4, 8, 1, 2, 1
    a, _ = sc.render(sc.fill_result, st, threads=8)
    b, _ = sc.render(sc.fill_result, st, threads=3)
    assert np.isfinite(a).all() and np.array_equal(a, b) and a[..., :3].mean() > 0.05
