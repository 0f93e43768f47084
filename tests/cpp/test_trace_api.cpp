// The ray queries of the C++ host layer (include/raysnail.hpp): World::trace_closest, World::trace_occluded and
// World::object_ids, without a GPU. On a world committed for no device (a host-only build) a valid call reaches the
// library's validation, which answers RS_E_STATE before anything touches a device; a ray table that is not 8 doubles
// per ray, a null output and a misaligned device pointer are RS_E_INVALID before that.
// With arguments `gpu <rays> <file>` (on a GPU): the same world committed to the current device and the rays of <rays>
// (raw doubles, 8 per ray) at tmin = 1e-3: trace_closest's ids, geom and uv, trace_occluded's bytes, the ids of
// trace_closest without geom and uv, then the handles of the ball, the crate and the ground, written to <file> raw.
// Built and run by tests/test_trace_cpp.py (and, on the GPU, by tests/test_gpu_trace.py).
#include <cstdio>
#include <cstring>
#include <memory>

#include "raysnail.hpp"

using namespace raysnail;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);         \
            return 1;                                                  \
        }                                                              \
    } while (0)

template <class F>
static int code_of(F&& f) {
    try {
        f();
    } catch (const Error& e) {
        return e.code();
    }
    return 0;
}

template <class T>
static bool put(std::FILE* out, const std::vector<T>& v) {
    return std::fwrite(v.data(), sizeof(T), v.size(), out) == v.size();
}

int main(int argc, char** argv) {
    static_assert(RS_TRACE_NONE == INT32_MIN, "the header's id of nothing");
    HittableList objects, lights;
    MaterialRef grey = std::make_shared<Lambertian>(Texture::color(Color{0.5f, 0.5f, 0.5f, 1.f}));
    MaterialRef lamp = std::make_shared<DiffuseLight>(Texture::color(Color{1.f, 0.9f, 0.8f, 1.f}));
    HittableRef ball = std::make_shared<Sphere>(Point3{0.0, 0.0, 0.0}, 1.0, grey);
    HittableRef crate = std::make_shared<Box>(Point3{1.5, -1.0, -1.0}, Point3{2.5, 0.5, 1.0}, grey);
    HittableRef ground = AARect::new_xz(AARectMetrics(-1.0, {-8.0, 8.0}, {-8.0, 8.0}), grey);
    HittableRef stranger = std::make_shared<Sphere>(Point3{0.0, 5.0, 0.0}, 1.0, grey);
    auto sun = std::make_shared<Sphere>(Point3{300.0, 400.0, 100.0}, 12.0, lamp);
    objects.add(ball);
    objects.add(crate);
    objects.add(ground);
    objects.add(sun);
    lights.add(sun);
    World world(std::move(objects), std::move(lights));

    if (argc == 4 && std::strcmp(argv[1], "gpu") == 0) {
        std::vector<double> rays;
        {
            std::FILE* in = std::fopen(argv[2], "rb");
            CHECK(in != nullptr);
            double ray[8];
            while (std::fread(ray, sizeof(double), 8, in) == 8) rays.insert(rays.end(), ray, ray + 8);
            std::fclose(in);
        }
        const size_t n = rays.size() / 8;
        CHECK(n > 0);
        World::TraceHits full, lean;
        std::vector<uint8_t> occ;
        std::vector<uint32_t> handles;
        try {
            full = world.trace_closest(rays, 1e-3);
            occ = world.trace_occluded(rays, 1e-3);
            lean = world.trace_closest(rays, 1e-3, false, false);
            for (const HittableRef& o : {ball, crate, ground}) {
                const std::vector<uint32_t> h = world.object_ids(o);
                CHECK(h.size() == 1);
                handles.push_back(h[0]);
            }
            CHECK(world.trace_closest({}, 1e-3).ids.empty() && world.trace_occluded({}, 1e-3).empty());
        } catch (const Error& e) {
            std::printf("FAILED: [%d] %s\n", e.code(), e.what());
            return 1;
        }
        CHECK(full.ids.size() == n * 4 && full.geom.size() == n * 8 && full.uv.size() == n * 2 && occ.size() == n);
        CHECK(lean.ids.size() == n * 4 && lean.geom.empty() && lean.uv.empty());
        std::FILE* out = std::fopen(argv[3], "wb");
        CHECK(out != nullptr);
        CHECK(put(out, full.ids) && put(out, full.geom) && put(out, full.uv) && put(out, occ) && put(out, lean.ids));
        CHECK(put(out, handles));
        std::fclose(out);
        std::printf("ok\n");
        return 0;
    }

    rs_scene* s = world.device_scene(std::vector<int>{});  // host-only build
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.n_devices == 0 && info.n_world == 4);

    // the handles the objects were exported with: dense, in export order; a stranger and a null reference are refused
    CHECK(world.object_ids(ball) == std::vector<uint32_t>{0} && world.object_ids(crate) == std::vector<uint32_t>{1});
    CHECK(world.object_ids(ground) == std::vector<uint32_t>{2} && world.object_ids(sun) == std::vector<uint32_t>{3});
    CHECK(code_of([&] { world.object_ids(stranger); }) == RS_E_INVALID);
    CHECK(code_of([&] { world.object_ids(HittableRef()); }) == RS_E_INVALID);

    const std::vector<double> rays = {5.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 100.0,   //
                                      5.0, 3.0, 0.0, -1.0, 0.0, 0.0, 0.0, 100.0};
    CHECK(code_of([&] { world.trace_closest(rays); }) == RS_E_STATE);
    CHECK(code_of([&] { world.trace_closest(rays, 0.5, false, false); }) == RS_E_STATE);
    CHECK(code_of([&] { world.trace_occluded(rays); }) == RS_E_STATE);
    CHECK(code_of([&] { world.trace_closest({}); }) == RS_E_STATE);
    CHECK(code_of([&] { world.trace_closest(std::vector<double>(15, 0.0)); }) == RS_E_INVALID);
    CHECK(code_of([&] { world.trace_occluded(std::vector<double>(7, 0.0)); }) == RS_E_INVALID);
    // the device-pointer overloads: validation alone (nothing is dereferenced before it)
    alignas(16) static double d_rays[16], d_geom[16], d_uv[4];
    static int32_t d_ids[8];
    static uint8_t d_occ[2];
    CHECK(code_of([&] { world.trace_closest(d_rays, 2, 1e-4, d_ids, d_geom, d_uv); }) == RS_E_STATE);
    CHECK(code_of([&] { world.trace_closest(d_rays, 2, 1e-4, d_ids); }) == RS_E_STATE);
    CHECK(code_of([&] { world.trace_occluded(d_rays, 2, 1e-4, d_occ); }) == RS_E_STATE);
    CHECK(code_of([&] { world.trace_closest(d_rays, 2, 1e-4, nullptr, d_geom, d_uv); }) == RS_E_INVALID);
    CHECK(code_of([&] { world.trace_closest(nullptr, 2, 1e-4, d_ids); }) == RS_E_INVALID);
    CHECK(code_of([&] { world.trace_closest(d_rays + 1, 1, 1e-4, d_ids); }) == RS_E_INVALID);
    CHECK(code_of([&] { world.trace_closest(d_rays, 1, 1e-4, d_ids, d_geom + 1); }) == RS_E_INVALID);
    CHECK(code_of([&] { world.trace_closest(d_rays, 2, 1e-4, d_ids, nullptr, nullptr, nullptr, 1); }) == RS_E_INVALID);
    CHECK(code_of([&] { world.trace_occluded(d_rays, 2, 1e-4, nullptr); }) == RS_E_INVALID);
    CHECK(code_of([&] { world.trace_occluded(d_rays + 1, 1, 1e-4, d_occ); }) == RS_E_INVALID);
    // the C entry points through the same header
    CHECK(rs_trace_closest(s, rays.data(), 2, 1e-4, d_ids, d_geom, d_uv) == RS_E_STATE);
    CHECK(rs_trace_occluded(s, rays.data(), 2, 1e-4, d_occ) == RS_E_STATE);
    CHECK(rs_trace_closest(s, rays.data(), 2, 1e-4, nullptr, d_geom, d_uv) == RS_E_INVALID);
    CHECK(rs_trace_occluded(s, nullptr, 2, 1e-4, d_occ) == RS_E_INVALID);
    std::printf("ok\n");
    return 0;
}
