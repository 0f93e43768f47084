// raysnail::denoise and TakePhotoSettings::shot_denoised of the C++ host layer (include/raysnail.hpp), without a GPU:
// rs_denoise's validation answers RS_E_INVALID before anything touches a device, and on a world committed for no
// device shot_denoised stops at the beauty render's RS_E_STATE; the host layer hands both over as a raysnail::Error.
// With arguments `gpu <file>` (on a GPU): the same world committed to the current device, shot_denoised at 4 samples,
// seed 3, pass 1 under the PixelController, the denoised frame then the beauty frame written to <file> as raw f32.
// Built and run by tests/test_denoise_cpp.py (and, on the GPU, by tests/test_gpu_denoise.py).
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
        TakePhotoSettings::Denoised d;
        try {
            d = photo.shot_denoised(world, &every_other);
        } catch (const Error& e) {
            std::printf("FAILED: [%d] %s\n", e.code(), e.what());
            return 1;
        }
        CHECK(d.denoised.size() == 8 * 6 && d.beauty.size() == 8 * 6);
        CHECK(photo.last_stats().segments >= 8 * 6 * 4 / 2);  // the beauty frame's: every unmasked sample's first segment
        std::FILE* out = std::fopen(argv[2], "wb");
        CHECK(out != nullptr);
        CHECK(std::fwrite(d.denoised.data(), sizeof(Pixel), d.denoised.size(), out) == d.denoised.size());
        CHECK(std::fwrite(d.beauty.data(), sizeof(Pixel), d.beauty.size(), out) == d.beauty.size());
        std::fclose(out);
        std::printf("ok\n");
        return 0;
    }

    // the defaults are the header's
    const DenoiseSettings def;
    CHECK(def.levels == RS_DENOISE_LEVELS && def.sigma_color == RS_DENOISE_SIGMA_COLOR &&
          def.sigma_normal == RS_DENOISE_SIGMA_NORMAL && def.sigma_depth == RS_DENOISE_SIGMA_DEPTH);

    // invalid arguments: raysnail::Error(RS_E_INVALID), the frame untouched
    const int W = 4, H = 3;
    std::vector<Pixel> px(W * H, Pixel{0.25f, 0.5f, 0.75f, 1.f});
    const std::vector<Pixel> guide(W * H, Pixel{0.f, 0.f, 0.f, 0.f}), small(W * H - 1, Pixel{0.f, 0.f, 0.f, 0.f});
    DenoiseSettings st;
    st.levels = 0;
    CHECK(code_of([&] { denoise(px, nullptr, nullptr, W, H, st); }) == RS_E_INVALID);
    st.levels = 9;
    CHECK(code_of([&] { denoise(px, &guide, &guide, W, H, st); }) == RS_E_INVALID);
    st = DenoiseSettings();
    st.sigma_color = 0.f;
    CHECK(code_of([&] { denoise(px, nullptr, nullptr, W, H, st); }) == RS_E_INVALID);
    st = DenoiseSettings();
    st.sigma_normal = std::numeric_limits<float>::quiet_NaN();
    CHECK(code_of([&] { denoise(px, nullptr, nullptr, W, H, st); }) == RS_E_INVALID);
    st = DenoiseSettings();
    st.sigma_depth = 2e4f;
    CHECK(code_of([&] { denoise(px, nullptr, nullptr, W, H, st); }) == RS_E_INVALID);
    st = DenoiseSettings();
    CHECK(code_of([&] { denoise(px, nullptr, nullptr, W, H + 1, st); }) == RS_E_INVALID);   // size mismatch
    CHECK(code_of([&] { denoise(px, &small, nullptr, W, H, st); }) == RS_E_INVALID);
    CHECK(code_of([&] { denoise(px, nullptr, &small, W, H, st); }) == RS_E_INVALID);
    CHECK(code_of([&] { denoise(px, nullptr, nullptr, -4, -3, st); }) == RS_E_INVALID);
    std::vector<Pixel> empty;
    CHECK(code_of([&] { denoise(empty, nullptr, nullptr, 0, 0, st); }) == RS_E_INVALID);    // W H = 0
    for (const Pixel& p : px) CHECK(p == (Pixel{0.25f, 0.5f, 0.75f, 1.f}));

    // shot_denoised on a host-only build: the beauty render's RS_E_STATE
    rs_scene* s = world.device_scene(std::vector<int>{});
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.n_devices == 0 && info.n_world == 2);
    for (const PixelController* pm : {static_cast<const PixelController*>(nullptr),
                                      static_cast<const PixelController*>(&every_other)}) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        CHECK(code_of([&] { photo.shot_denoised(world, pm); }) == RS_E_STATE);
    }
    std::printf("ok\n");
    return 0;
}
