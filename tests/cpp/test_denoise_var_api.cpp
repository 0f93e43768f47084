// raysnail::pass_moments, raysnail::denoise_var and TakePhotoSettings::shot_denoised_passes of the C++ host layer
// (include/raysnail.hpp), without a GPU: the validation answers RS_E_INVALID before anything touches a device, and on a
// world committed for no device shot_denoised_passes stops at the first pass's RS_E_STATE; the host layer hands both
// over as a raysnail::Error.
// With arguments `gpu <file>` (on a GPU): the same world committed to the current device, shot_denoised_passes with 3
// passes of 4 samples, seed 3, from pass 1 under the PixelController; the denoised, mean and variance frames written
// to <file> as raw f32.
// Built and run by tests/test_denoise_var_cpp.py (and, on the GPU, by tests/test_gpu_denoise_var.py).
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
        TakePhotoSettings::DenoisedPasses d;
        try {
            d = photo.shot_denoised_passes(world, 3, &every_other);
        } catch (const Error& e) {
            std::printf("FAILED: [%d] %s\n", e.code(), e.what());
            return 1;
        }
        CHECK(d.denoised.size() == 8 * 6 && d.mean.size() == 8 * 6 && d.var.size() == 8 * 6);
        CHECK(photo.last_stats().segments >= 8 * 6 * 4 / 2);  // the last pass's: every unmasked sample's first segment
        std::FILE* out = std::fopen(argv[2], "wb");
        CHECK(out != nullptr);
        for (const std::vector<Pixel>* f : {&d.denoised, &d.mean, &d.var})
            CHECK(std::fwrite(f->data(), sizeof(Pixel), f->size(), out) == f->size());
        std::fclose(out);
        std::printf("ok\n");
        return 0;
    }

    // the defaults are the header's
    const DenoiseVarSettings def;
    CHECK(def.levels == RS_DENOISE_VAR_LEVELS && def.k_color == RS_DENOISE_VAR_K_COLOR &&
          def.sigma_normal == RS_DENOISE_SIGMA_NORMAL && def.sigma_depth == RS_DENOISE_SIGMA_DEPTH);

    // denoise_var's invalid arguments: raysnail::Error(RS_E_INVALID), the frames untouched
    const int W = 4, H = 3;
    const Pixel colour{0.25f, 0.5f, 0.75f, 1.f}, variance{0.01f, 0.02f, 0.03f, 4.f}, marker{7.f, 7.f, 7.f, 7.f};
    std::vector<Pixel> px(W * H, colour), out_var(2, marker);
    const std::vector<Pixel> var(W * H, variance);
    const std::vector<Pixel> guide(W * H, Pixel{0.f, 0.f, 0.f, 0.f}), small(W * H - 1, Pixel{0.f, 0.f, 0.f, 0.f});
    DenoiseVarSettings st;
    st.levels = 0;
    CHECK(code_of([&] { denoise_var(px, var, nullptr, nullptr, W, H, st, true, &out_var); }) == RS_E_INVALID);
    st.levels = 9;
    CHECK(code_of([&] { denoise_var(px, var, &guide, &guide, W, H, st); }) == RS_E_INVALID);
    st = DenoiseVarSettings();
    st.k_color = 0.f;
    CHECK(code_of([&] { denoise_var(px, var, nullptr, nullptr, W, H, st, true, &out_var); }) == RS_E_INVALID);
    st.k_color = std::numeric_limits<float>::infinity();
    CHECK(code_of([&] { denoise_var(px, var, nullptr, nullptr, W, H, st); }) == RS_E_INVALID);
    st = DenoiseVarSettings();
    st.sigma_normal = std::numeric_limits<float>::quiet_NaN();
    CHECK(code_of([&] { denoise_var(px, var, nullptr, nullptr, W, H, st); }) == RS_E_INVALID);
    st = DenoiseVarSettings();
    st.sigma_depth = 2e4f;
    CHECK(code_of([&] { denoise_var(px, var, nullptr, nullptr, W, H, st); }) == RS_E_INVALID);
    st = DenoiseVarSettings();
    CHECK(code_of([&] { denoise_var(px, var, nullptr, nullptr, W, H + 1, st); }) == RS_E_INVALID);  // size mismatch
    CHECK(code_of([&] { denoise_var(px, small, nullptr, nullptr, W, H, st, true, &out_var); }) == RS_E_INVALID);
    CHECK(code_of([&] { denoise_var(px, var, &small, nullptr, W, H, st); }) == RS_E_INVALID);
    CHECK(code_of([&] { denoise_var(px, var, nullptr, &small, W, H, st); }) == RS_E_INVALID);
    CHECK(code_of([&] { denoise_var(px, var, nullptr, nullptr, -4, -3, st); }) == RS_E_INVALID);
    std::vector<Pixel> empty;
    CHECK(code_of([&] { denoise_var(empty, empty, nullptr, nullptr, 0, 0, st); }) == RS_E_INVALID);  // W H = 0
    for (const Pixel& p : px) CHECK(p == colour);
    CHECK(out_var.size() == 2 && out_var[0] == marker && out_var[1] == marker);

    // pass_moments' invalid arguments
    const std::vector<std::vector<Pixel>> none, mismatched{px, small}, too_many(65, px), sized_wrong{px, px};
    CHECK(code_of([&] { pass_moments(none, W, H); }) == RS_E_INVALID);          // n_frames = 0
    CHECK(code_of([&] { pass_moments(too_many, W, H); }) == RS_E_INVALID);      // n_frames = 65
    CHECK(code_of([&] { pass_moments(mismatched, W, H); }) == RS_E_INVALID);
    CHECK(code_of([&] { pass_moments(sized_wrong, W, H + 1); }) == RS_E_INVALID);
    CHECK(code_of([&] { pass_moments(sized_wrong, -4, -3); }) == RS_E_INVALID);
    const std::vector<std::vector<Pixel>> empties{empty, empty};
    CHECK(code_of([&] { pass_moments(empties, 0, 0); }) == RS_E_INVALID);       // W H = 0

    // shot_denoised_passes: fewer than 2 passes is RS_E_INVALID; on a host-only build the first pass's RS_E_STATE
    rs_scene* s = world.device_scene(std::vector<int>{});
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.n_devices == 0 && info.n_world == 2);
    for (const PixelController* pm : {static_cast<const PixelController*>(nullptr),
                                      static_cast<const PixelController*>(&every_other)}) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        CHECK(code_of([&] { photo.shot_denoised_passes(world, 1, pm); }) == RS_E_INVALID);
        CHECK(code_of([&] { photo.shot_denoised_passes(world, 0, pm); }) == RS_E_INVALID);
        CHECK(code_of([&] { photo.shot_denoised_passes(world, 4, pm); }) == RS_E_STATE);
        CHECK(photo.settings().pass == 1);  // the photo's own pass index is back
    }
    std::printf("ok\n");
    return 0;
}
