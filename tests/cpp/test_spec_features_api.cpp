// The specular-chain parameters of the C++ host layer (include/raysnail.hpp): shot_features' max_specular and
// shot_denoised / shot_denoised_passes' guide_specular, without a GPU. On a world committed for no device (a host-only
// build) a valid call reaches the library's validation, which answers RS_E_STATE before anything touches a device; a
// budget above 16 is RS_E_INVALID before that. The defaults are the calls as they were.
// With arguments `gpu <file>` (on a GPU): the same world committed to the current device, 4 samples, seed 3, pass 1
// under the same PixelController; shot_features(world, mask, 2)'s albedo and normal frames, then shot_features(world,
// mask)'s, written to <file> as raw f32.
// Built and run by tests/test_spec_features_cpp.py (and, on the GPU, by tests/test_gpu_spec_features.py).
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
    auto mirror = std::make_shared<Metal>(Texture::color(Color{0.5f, 0.75f, 0.25f, 1.f}));
    auto grey = std::make_shared<Lambertian>(Texture::color(Color{0.5f, 0.5f, 0.5f, 1.f}));
    auto lamp = std::make_shared<DiffuseLight>(Texture::color(Color{1.f, 0.9f, 0.8f, 1.f}));
    auto sun = std::make_shared<Sphere>(Point3{300.0, 400.0, 100.0}, 12.0, lamp);
    objects.add(std::make_shared<Sphere>(Point3{0.0, 0.0, 0.0}, 1.0, mirror));
    objects.add(std::make_shared<Sphere>(Point3{0.0, -101.0, 0.0}, 100.0, grey));
    objects.add(sun);
    lights.add(sun);
    Camera cam = CameraBuilder().look_from({13, 2, 3}).look_at({0, 0, 0}).fov(20).width(8).height(6).build();
    World world(std::move(objects), std::move(lights));
    const EveryOther every_other;

    if (argc == 3 && std::strcmp(argv[1], "gpu") == 0) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        TakePhotoSettings::Features chain, first;
        try {
            chain = photo.shot_features(world, &every_other, 2);
            CHECK(photo.last_stats().samples == 8 * 6 * 4 && photo.last_stats().segments > 8 * 6 * 4 / 2);
            CHECK(photo.last_stats().segments <= 3 * 8 * 6 * 4 / 2);
            first = photo.shot_features(world, &every_other);
            CHECK(photo.last_stats().segments == 8 * 6 * 4 / 2);
        } catch (const Error& e) {
            std::printf("FAILED: [%d] %s\n", e.code(), e.what());
            return 1;
        }
        std::FILE* out = std::fopen(argv[2], "wb");
        CHECK(out != nullptr);
        for (const std::vector<Pixel>* f : {&chain.albedo, &chain.normal, &first.albedo, &first.normal}) {
            CHECK(f->size() == 8 * 6);
            CHECK(std::fwrite(f->data(), sizeof(Pixel), f->size(), out) == f->size());
        }
        std::fclose(out);
        std::printf("ok\n");
        return 0;
    }

    rs_scene* s = world.device_scene(std::vector<int>{});  // host-only build
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.n_devices == 0 && info.n_world == 3);

    for (const PixelController* pm : {static_cast<const PixelController*>(nullptr),
                                      static_cast<const PixelController*>(&every_other)}) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        // the defaults: the calls as they were
        CHECK(code_of([&] { photo.shot_features(world, pm); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_denoised(world, pm); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_denoised_passes(world, 2, pm); }) == RS_E_STATE);
        // the new parameter: validated by the library, the budget before the scene's state
        CHECK(code_of([&] { photo.shot_features(world, pm, 0); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_features(world, pm, 1); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_features(world, pm, 16); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_features(world, pm, 17); }) == RS_E_INVALID);
        CHECK(code_of([&] { photo.shot_denoised(world, pm, DenoiseSettings(), 2); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_denoised_passes(world, 2, pm, DenoiseVarSettings(), 2); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_denoised_passes(world, 1, pm, DenoiseVarSettings(), 2); }) == RS_E_INVALID);
    }
    // the C entry points through the same header
    rs_camera_desc cd = cam.desc();
    rs_render_settings st = cam.take_photo().samples(4).settings();
    float px[8 * 6 * 4];
    CHECK(rs_render_features_specular(s, &cd, &st, nullptr, 17, px, nullptr, nullptr) == RS_E_INVALID);
    CHECK(rs_render_features_specular(s, &cd, &st, nullptr, 3, nullptr, nullptr, nullptr) == RS_E_INVALID);
    CHECK(rs_render_features_specular(s, &cd, &st, nullptr, 3, px, nullptr, nullptr) == RS_E_STATE);
    CHECK(rs_render_features_specular_device(s, &cd, &st, nullptr, 3, px, px, nullptr, nullptr) == RS_E_STATE);
    std::printf("ok\n");
    return 0;
}
