// TakePhotoSettings::shot_features of the C++ host layer (include/raysnail.hpp), without a GPU: on a world committed
// for no device (a host-only build) the call reaches rs_render_features, whose validation answers RS_E_STATE before
// anything touches a device; the host layer hands that over as a raysnail::Error.
// With arguments `gpu <file>` (on a GPU): the same world committed to the current device, shot_features at 4 samples,
// seed 3, pass 1 under the same PixelController, the albedo frame then the normal frame written to <file> as raw f32.
// Built and run by tests/test_features_cpp.py (and, on the GPU, by tests/test_gpu_features.py).
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
        TakePhotoSettings::Features f;
        try {
            f = photo.shot_features(world, &every_other);
        } catch (const Error& e) {
            std::printf("FAILED: [%d] %s\n", e.code(), e.what());
            return 1;
        }
        CHECK(f.albedo.size() == 8 * 6 && f.normal.size() == 8 * 6);
        CHECK(photo.last_stats().samples == 8 * 6 * 4 && photo.last_stats().segments == 8 * 6 * 4 / 2);
        std::FILE* out = std::fopen(argv[2], "wb");
        CHECK(out != nullptr);
        CHECK(std::fwrite(f.albedo.data(), sizeof(Pixel), f.albedo.size(), out) == f.albedo.size());
        CHECK(std::fwrite(f.normal.data(), sizeof(Pixel), f.normal.size(), out) == f.normal.size());
        std::fclose(out);
        std::printf("ok\n");
        return 0;
    }

    rs_scene* s = world.device_scene(std::vector<int>{});  // host-only build
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.n_devices == 0 && info.n_world == 2);
    CHECK(world.device_scene() == s);  // committed once

    int code = 0;
    try {
        world.device_scene(std::vector<int>{});
    } catch (const Error& e) {
        code = e.code();
    }
    CHECK(code == RS_E_STATE);  // already committed

    for (const PixelController* pm : {static_cast<const PixelController*>(nullptr),
                                      static_cast<const PixelController*>(&every_other)}) {
        code = 0;
        try {
            TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
            TakePhotoSettings::Features f = photo.shot_features(world, pm);
            CHECK(f.albedo.empty());  // not reached
        } catch (const Error& e) {
            code = e.code();
        }
        CHECK(code == RS_E_STATE);
    }
    std::printf("ok\n");
    return 0;
}
