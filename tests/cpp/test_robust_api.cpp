// raysnail::pass_robust and the `robust` argument of TakePhotoSettings::shot_denoised_passes of the C++ host layer
// (include/raysnail.hpp), without a GPU: the constants are the header's, the validation answers RS_E_INVALID before
// anything touches a device or renders, and with robust left at its default shot_denoised_passes goes on to the first
// pass's RS_E_STATE on a world committed for no device, as it always did.
// With arguments `gpu <file>` (on a GPU): the same world committed to the current device, shot_denoised_passes with 4
// passes of 4 samples, seed 3, from pass 1 under the PixelController and robust = ROBUST_AUTO, then pass_robust with
// trim 0.25 over four pass frames of its own; the denoised, mean and variance frames of the first and the mean and
// variance frames of the second written to <file> as raw f32, the second's trim counts after them as bytes.
// Built and run by tests/test_robust_cpp.py.
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
    const int W = 8, H = 6;

    if (argc == 3 && std::strcmp(argv[1], "gpu") == 0) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        TakePhotoSettings::DenoisedPasses d;
        PassRobust r;
        try {
            d = photo.shot_denoised_passes(world, 4, &every_other, DenoiseVarSettings(), 0, ROBUST_AUTO);
            std::vector<std::vector<Pixel>> frames;
            for (uint32_t k = 0; k < 4; ++k)
                frames.push_back(cam.take_photo().samples(4).seed(3).pass_index(1 + k).shot_to_target(
                    nullptr, world, nullptr, nullptr, &every_other));
            r = pass_robust(frames, W, H, true, 0.25f);
        } catch (const Error& e) {
            std::printf("FAILED: [%d] %s\n", e.code(), e.what());
            return 1;
        }
        CHECK(d.denoised.size() == W * H && d.mean.size() == W * H && d.var.size() == W * H);
        CHECK(r.mean.size() == W * H && r.var.size() == W * H && r.trimmed.size() == W * H);
        CHECK(photo.settings().pass == 1);
        std::FILE* out = std::fopen(argv[2], "wb");
        CHECK(out != nullptr);
        for (const std::vector<Pixel>* f : {&d.denoised, &d.mean, &d.var, &r.mean, &r.var})
            CHECK(std::fwrite(f->data(), sizeof(Pixel), f->size(), out) == f->size());
        CHECK(std::fwrite(r.trimmed.data(), 1, r.trimmed.size(), out) == r.trimmed.size());
        std::fclose(out);
        std::printf("ok\n");
        return 0;
    }

    // the constants are the header's; ROBUST_OFF is no valid trim
    CHECK(ROBUST_AUTO == RS_ROBUST_TRIM_AUTO && ROBUST_AUTO == -1.0f);
    CHECK(ROBUST_OFF != ROBUST_AUTO && !(ROBUST_OFF >= 0.0f));

    // pass_robust's invalid arguments: raysnail::Error(RS_E_INVALID)
    const Pixel colour{0.25f, 0.5f, 0.75f, 1.f};
    const std::vector<Pixel> px(W * H, colour), small(W * H - 1, colour), empty;
    const std::vector<std::vector<Pixel>> none, two{px, px}, mismatched{px, small}, too_many(65, px), empties{empty, empty};
    CHECK(code_of([&] { pass_robust(none, W, H); }) == RS_E_INVALID);      // n_frames = 0
    CHECK(code_of([&] { pass_robust(too_many, W, H); }) == RS_E_INVALID);  // n_frames = 65
    CHECK(code_of([&] { pass_robust(mismatched, W, H); }) == RS_E_INVALID);
    CHECK(code_of([&] { pass_robust(two, W, H + 1); }) == RS_E_INVALID);
    CHECK(code_of([&] { pass_robust(two, -8, -6); }) == RS_E_INVALID);
    CHECK(code_of([&] { pass_robust(empties, 0, 0); }) == RS_E_INVALID);  // W H = 0
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (float bad : {nan, inf, -inf, -0.5f, 0.50001f, 1.0f, ROBUST_OFF, -1e-6f})
        CHECK(code_of([&] { pass_robust(two, W, H, true, bad); }) == RS_E_INVALID);

    // shot_denoised_passes: a bad robust is RS_E_INVALID before the first pass (which a host-only build answers with
    // RS_E_STATE); every valid one, and the default, get as far as that pass
    rs_scene* s = world.device_scene(std::vector<int>{});
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.n_devices == 0 && info.n_world == 2);
    TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
    const DenoiseVarSettings st;
    for (float bad : {nan, inf, -0.5f, 0.50001f, -3.0f})
        CHECK(code_of([&] { photo.shot_denoised_passes(world, 4, &every_other, st, 0, bad); }) == RS_E_INVALID);
    CHECK(code_of([&] { photo.shot_denoised_passes(world, 1, nullptr, st, 0, ROBUST_AUTO); }) == RS_E_INVALID);
    for (float good : {ROBUST_OFF, ROBUST_AUTO, 0.0f, 0.1f, 0.5f})
        CHECK(code_of([&] { photo.shot_denoised_passes(world, 4, &every_other, st, 0, good); }) == RS_E_STATE);
    CHECK(code_of([&] { photo.shot_denoised_passes(world, 4); }) == RS_E_STATE);
    CHECK(photo.settings().pass == 1);
    std::printf("ok\n");
    return 0;
}
