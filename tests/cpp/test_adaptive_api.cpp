// raysnail::AdaptiveSettings and TakePhotoSettings::shot_adaptive of the C++ host layer (include/raysnail.hpp), without
// a GPU: the defaults are the header's; every invalid setting answers RS_E_INVALID before anything touches a device (the
// C entry leaves its buffers alone), and on a world committed for no device shot_adaptive stops at RS_E_STATE; the host
// layer hands both over as a raysnail::Error.
// With arguments `gpu <file>` (on a GPU): the same world committed to the current device, shot_adaptive with 4 samples
// per pass, seed 3, from pass 1, at most 6 passes under the PixelController; the mean and variance frames written to
// <file> as raw f32, then one line `passes <n> <active of each>`.
// Built and run by tests/test_adaptive_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

struct EveryOther : PixelController {
    bool calculate_pixel(size_t x, size_t y) const override { return (x + y) % 2 == 0; }
};

template <class F>
static int code_of(F&& f) {
    try {
        f();
    } catch (const Error& e) {
        return e.code();
    }
    return 0;
}

int main(int argc, char** argv) {
    HittableList objects, lights;
    auto grey = std::make_shared<Lambertian>(Texture::color(Color{0.5f, 0.5f, 0.5f, 1.f}));
    auto lamp = std::make_shared<DiffuseLight>(Texture::color(Color{1.f, 0.9f, 0.8f, 1.f}));
    auto sun = std::make_shared<Sphere>(Point3{300.0, 400.0, 100.0}, 12.0, lamp);
    objects.add(std::make_shared<Sphere>(Point3{0.0, 0.0, 0.0}, 1.0, grey));
    objects.add(sun);
    lights.add(sun);
    Camera cam = CameraBuilder().look_from({13, 2, 3}).look_at({0, 0, 0}).fov(20).width(8).height(6).build();
    World world(std::move(objects), std::move(lights));
    const EveryOther every_other;

    if (argc == 3 && std::strcmp(argv[1], "gpu") == 0) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        AdaptiveSettings as;
        as.max_passes = 6;
        TakePhotoSettings::Adaptive a;
        try {
            a = photo.shot_adaptive(world, as, &every_other);
        } catch (const Error& e) {
            std::printf("FAILED: [%d] %s\n", e.code(), e.what());
            return 1;
        }
        CHECK(a.mean.size() == 8 * 6 && a.var.size() == 8 * 6);
        CHECK(a.passes.size() >= 2 && a.passes.size() <= 6 && a.passes[0].active == 8 * 6 / 2);
        CHECK(photo.last_stats().segments == a.passes.back().stats.segments && photo.last_stats().segments > 0);
        std::FILE* out = std::fopen(argv[2], "wb");
        CHECK(out != nullptr);
        for (const std::vector<Pixel>* f : {&a.mean, &a.var})
            CHECK(std::fwrite(f->data(), sizeof(Pixel), f->size(), out) == f->size());
        std::fclose(out);
        std::printf("passes %zu", a.passes.size());
        for (const rs_adaptive_pass& p : a.passes) std::printf(" %llu", (unsigned long long)p.active);
        std::printf("\nok\n");
        return 0;
    }

    // the defaults are the header's
    const AdaptiveSettings def;
    CHECK(def.min_passes == RS_ADAPTIVE_MIN_PASSES && def.max_passes == RS_ADAPTIVE_MAX_PASSES &&
          def.radius == RS_ADAPTIVE_RADIUS && def.tolerance == RS_ADAPTIVE_TOLERANCE && def.floor == RS_ADAPTIVE_FLOOR);

    rs_scene* s = world.device_scene(std::vector<int>{});  // a host-only build
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.n_devices == 0 && info.n_world == 2);

    // each invalid setting: raysnail::Error(RS_E_INVALID) from shot_adaptive, and RS_E_INVALID from the C entry with
    // its buffers left alone -- the settings are checked before the scene's state
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<AdaptiveSettings> bad(14);
    bad[0].min_passes = 1;
    bad[1].min_passes = 0;
    bad[2].min_passes = 5; bad[2].max_passes = 4;
    bad[3].max_passes = 4097;
    bad[4].tolerance = nan;
    bad[5].tolerance = inf;
    bad[6].tolerance = 1e-7f;
    bad[7].tolerance = 2e4f;
    bad[8].floor = nan;
    bad[9].floor = 0.f;
    bad[10].floor = -1.f;
    bad[11].floor = 2e4f;
    bad[12].radius = 5;
    bad[13].max_passes = 0xFFFFFFFFu;
    const Pixel marker{7.f, 7.f, 7.f, 7.f};
    const rs_render_settings st = cam.take_photo().samples(4).seed(3).settings();
    for (const AdaptiveSettings& b : bad) {
        for (const PixelController* pm : {static_cast<const PixelController*>(nullptr),
                                          static_cast<const PixelController*>(&every_other)}) {
            TakePhotoSettings photo = cam.take_photo().samples(4).seed(3);
            CHECK(code_of([&] { photo.shot_adaptive(world, b, pm); }) == RS_E_INVALID);
        }
        std::vector<Pixel> mean(8 * 6, marker), var(8 * 6, marker);
        rs_adaptive_pass reports[2];
        std::memset(reports, 0x5A, sizeof(reports));
        uint32_t n = 77;
        const rs_adaptive_settings as{b.min_passes, b.max_passes, b.radius, b.tolerance, b.floor};
        CHECK(rs_render_adaptive(s, &cam.desc(), &st, &as, nullptr, reinterpret_cast<float*>(mean.data()),
                                 reinterpret_cast<float*>(var.data()), reports, &n) == RS_E_INVALID);
        for (size_t i = 0; i < mean.size(); ++i) CHECK(mean[i] == marker && var[i] == marker);
        const unsigned char* raw = reinterpret_cast<const unsigned char*>(reports);
        for (size_t i = 0; i < sizeof(reports); ++i) CHECK(raw[i] == 0x5A);
        CHECK(n == 77);
    }
    // the scene-free entries check their arguments before the device too
    float buf[4] = {7.f, 7.f, 7.f, 7.f};
    const float* one[1] = {buf};
    uint8_t byte = 9;
    CHECK(rs_moments_update_device(buf, buf, one, 0, 1, 1, 1, nullptr) == RS_E_INVALID);
    CHECK(rs_moments_update_device(buf, buf, one, 1, 1, 1, 2, nullptr) == RS_E_INVALID);
    CHECK(rs_moments_update_device(buf, buf, one, 1, 0, 1, 1, nullptr) == RS_E_INVALID);
    CHECK(rs_moments_resolve_device(buf, buf, 1, 1, 1, nullptr, nullptr, nullptr) == RS_E_INVALID);
    CHECK(rs_adaptive_mask_device(buf, buf, nullptr, 1, 1, 1, 8, 0.1f, 0.03f, 1, &byte, nullptr, nullptr) == RS_E_INVALID);
    CHECK(rs_adaptive_mask_device(buf, buf, nullptr, 1, 1, 2, 8, 0.1f, 0.03f, 1, nullptr, nullptr, nullptr) == RS_E_INVALID);
    CHECK(buf[0] == 7.f && buf[3] == 7.f && byte == 9);

    // valid settings on the host-only build: RS_E_STATE
    for (const PixelController* pm : {static_cast<const PixelController*>(nullptr),
                                      static_cast<const PixelController*>(&every_other)}) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        CHECK(code_of([&] { photo.shot_adaptive(world, AdaptiveSettings(), pm); }) == RS_E_STATE);
        CHECK(photo.settings().pass == 1);
    }
    std::printf("ok\n");
    return 0;
}
