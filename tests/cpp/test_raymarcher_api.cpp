// raysnail::RayMarcher of the C++ host layer (include/raysnail.hpp), without a GPU: exported into libraysnail_hip's
// sink it becomes an rs_raymarcher object of a host-only committed scene; any other sink table has no marcher.
// Built and run by tests/test_raymarch_cpu.py.
#include <cstdio>
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

int main() {
    rs_scene* s = nullptr;
    CHECK(rs_scene_create(&s) == RS_OK);
    auto grey = std::make_shared<Lambertian>(Texture::color(Color{0.5f, 0.5f, 0.5f, 1.f}));
    auto lamp = std::make_shared<DiffuseLight>(Texture::color(Color{1.f, 0.9f, 0.8f, 1.f}));
    auto bulb = std::make_shared<RayMarcher>(grey);
    auto sun = std::make_shared<Sphere>(Point3{300.0, 400.0, 100.0}, 12.0, lamp);
    {
        SceneSink sink(hip_sink_api(), s);
        const std::vector<uint32_t> hb = sink.object(bulb), hs = sink.object(sun);
        CHECK(hb.size() == 1 && hs.size() == 1 && hb[0] != hs[0]);
        CHECK(sink.object(bulb) == hb);  // exported once
        CHECK(rs_world_add(s, hb[0]) == RS_OK && rs_world_add(s, hs[0]) == RS_OK && rs_lights_add(s, hs[0]) == RS_OK);
    }
    CHECK(rs_scene_commit_devices(s, nullptr, 0) == RS_OK);  // host-only build
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.scene_mode == 0 && info.ref_order == 1 && info.n_world == 2 && info.n_devices == 0);
    rs_scene_destroy(s);

    // a sink table of another backend (here: a copy of the same functions at another address)
    CHECK(rs_scene_create(&s) == RS_OK);
    const rsh_sink_api other = hip_sink_api();
    SceneSink foreign(other, s);
    int code = 0;
    try {
        foreign.object(std::make_shared<RayMarcher>(nullptr));
    } catch (const Error& e) {
        code = e.code();
    }
    CHECK(code == RS_E_UNSUPPORTED);
    rs_scene_destroy(s);
    std::printf("ok\n");
    return 0;
}
