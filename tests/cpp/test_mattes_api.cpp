// The material-id mattes of the C++ host layer (include/raysnail.hpp): TakePhotoSettings::shot_mattes, matte_extract
// and World::material_id, without a GPU. On a world committed for no device (a host-only build) a valid call reaches
// the library's validation, which answers RS_E_STATE before anything touches a device; ranks outside 1 .. 8 and a
// budget above 16 are RS_E_INVALID before that. matte_extract's argument checks need no scene at all.
// With arguments `gpu <file>` (on a GPU): the same world committed to the current device, 4 samples, seed 3, pass 1
// under the same PixelController; shot_mattes(world, mask, 4, 2)'s ids, coverages and overflow bytes, then
// shot_mattes(world, mask, 2)'s, then matte_extract of the first layers for {the ground's id, the background id},
// then the ids of the mirror, the ground and the lamp, written to <file> raw.
// Built and run by tests/test_mattes_cpp.py (and, on the GPU, by tests/test_gpu_mattes.py).
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

template <class T>
static bool put(std::FILE* out, const std::vector<T>& v) {
    return std::fwrite(v.data(), sizeof(T), v.size(), out) == v.size();
}

int main(int argc, char** argv) {
    static_assert(RS_MATTE_MAX_RANKS == 8 && RS_MATTE_MAX_DISTINCT == 64, "the header's limits");
    static_assert(RS_MATTE_ID_BACKGROUND == -2 && RS_MATTE_ID_EMPTY == INT32_MIN, "the header's ids");
    HittableList objects, lights;
    MaterialRef mirror = std::make_shared<Metal>(Texture::color(Color{0.5f, 0.75f, 0.25f, 1.f}));
    MaterialRef grey = std::make_shared<Lambertian>(Texture::color(Color{0.5f, 0.5f, 0.5f, 1.f}));
    MaterialRef lamp = std::make_shared<DiffuseLight>(Texture::color(Color{1.f, 0.9f, 0.8f, 1.f}));
    MaterialRef stranger = std::make_shared<Lambertian>(Texture::color(Color{0.1f, 0.1f, 0.1f, 1.f}));
    auto sun = std::make_shared<Sphere>(Point3{300.0, 400.0, 100.0}, 12.0, lamp);
    objects.add(std::make_shared<Sphere>(Point3{0.0, 0.0, 0.0}, 1.0, mirror));
    objects.add(std::make_shared<Sphere>(Point3{0.0, -101.0, 0.0}, 100.0, grey));
    objects.add(sun);
    lights.add(sun);
    Camera cam = CameraBuilder().look_from({13, 2, 3}).look_at({0, 0, 0}).fov(20).width(8).height(6).build();
    World world(std::move(objects), std::move(lights));
    const EveryOther every_other;
    const size_t npx = 8 * 6;

    if (argc == 3 && std::strcmp(argv[1], "gpu") == 0) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        TakePhotoSettings::Mattes chain, first;
        std::vector<float> matte;
        std::vector<int32_t> names;
        try {
            chain = photo.shot_mattes(world, &every_other, 4, 2);
            CHECK(photo.last_stats().kernel_id == RS_KERNEL_MATTES);
            CHECK(photo.last_stats().samples == npx * 4 && photo.last_stats().segments > npx * 4 / 2);
            CHECK(photo.last_stats().segments <= 3 * npx * 4 / 2);
            first = photo.shot_mattes(world, &every_other, 2);
            CHECK(photo.last_stats().segments == npx * 4 / 2);
            names = {world.material_id(mirror), world.material_id(grey), world.material_id(lamp)};
            matte = matte_extract(chain.ids, chain.cov, 8, 6, 4, {names[1], RS_MATTE_ID_BACKGROUND});
        } catch (const Error& e) {
            std::printf("FAILED: [%d] %s\n", e.code(), e.what());
            return 1;
        }
        CHECK(chain.ranks == 4 && chain.ids.size() == npx * 4 && chain.cov.size() == npx * 4 && chain.overflow.size() == npx);
        CHECK(first.ranks == 2 && first.ids.size() == npx * 2 && first.cov.size() == npx * 2 && matte.size() == npx);
        std::FILE* out = std::fopen(argv[2], "wb");
        CHECK(out != nullptr);
        CHECK(put(out, chain.ids) && put(out, chain.cov) && put(out, chain.overflow));
        CHECK(put(out, first.ids) && put(out, first.cov) && put(out, first.overflow));
        CHECK(put(out, matte) && put(out, names));
        std::fclose(out);
        std::printf("ok\n");
        return 0;
    }

    rs_scene* s = world.device_scene(std::vector<int>{});  // host-only build
    rs_scene_info info;
    CHECK(rs_scene_get_info(s, &info) == RS_OK);
    CHECK(info.n_devices == 0 && info.n_world == 3);

    // the handles the materials were exported with: dense, in export order; none for a null reference
    CHECK(world.material_id(mirror) == 0 && world.material_id(grey) == 1 && world.material_id(lamp) == 2);
    CHECK(world.material_id(MaterialRef()) == RS_NO_MATERIAL);
    CHECK(code_of([&] { world.material_id(stranger); }) == RS_E_INVALID);

    for (const PixelController* pm : {static_cast<const PixelController*>(nullptr),
                                      static_cast<const PixelController*>(&every_other)}) {
        TakePhotoSettings photo = cam.take_photo().samples(4).seed(3).pass_index(1);
        CHECK(code_of([&] { photo.shot_mattes(world, pm); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_mattes(world, pm, 1); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_mattes(world, pm, 8, 16); }) == RS_E_STATE);
        CHECK(code_of([&] { photo.shot_mattes(world, pm, 0); }) == RS_E_INVALID);
        CHECK(code_of([&] { photo.shot_mattes(world, pm, 9); }) == RS_E_INVALID);
        CHECK(code_of([&] { photo.shot_mattes(world, pm, 4, 17); }) == RS_E_INVALID);
    }
    // matte_extract: refused before anything touches a device
    const std::vector<int32_t> ids(npx * 2, 1);
    const std::vector<float> cov(npx * 2, 0.5f);
    CHECK(code_of([&] { matte_extract(ids, cov, 8, 6, 2, {}); }) == RS_E_INVALID);
    CHECK(code_of([&] { matte_extract(ids, cov, 8, 6, 2, std::vector<int32_t>(65, 1)); }) == RS_E_INVALID);
    CHECK(code_of([&] { matte_extract(ids, cov, 8, 6, 3, {1}); }) == RS_E_INVALID);
    CHECK(code_of([&] { matte_extract(ids, cov, 8, 5, 2, {1}); }) == RS_E_INVALID);
    CHECK(code_of([&] { matte_extract(ids, cov, -8, -6, 2, {1}); }) == RS_E_INVALID);
    CHECK(code_of([&] { matte_extract({}, {}, 0, 0, 2, {1}); }) == RS_E_INVALID);
    CHECK(code_of([&] { matte_extract({}, {}, 8, 6, 0, {1}); }) == RS_E_INVALID);
    CHECK(code_of([&] { matte_extract(std::vector<int32_t>(npx * 9, 1), std::vector<float>(npx * 9, 0.f), 8, 6, 9, {1}); }) ==
          RS_E_INVALID);
    // the C entry points through the same header
    rs_camera_desc cd = cam.desc();
    rs_render_settings st = cam.take_photo().samples(4).settings();
    int32_t li[8 * 6 * 8];
    float lc[8 * 6 * 8];
    uint8_t lo[8 * 6];
    CHECK(rs_render_mattes(s, &cd, &st, nullptr, 0, 0, li, lc, lo, nullptr) == RS_E_INVALID);
    CHECK(rs_render_mattes(s, &cd, &st, nullptr, 9, 0, li, lc, lo, nullptr) == RS_E_INVALID);
    CHECK(rs_render_mattes(s, &cd, &st, nullptr, 4, 17, li, lc, lo, nullptr) == RS_E_INVALID);
    CHECK(rs_render_mattes(s, &cd, &st, nullptr, 4, 0, nullptr, lc, lo, nullptr) == RS_E_INVALID);
    CHECK(rs_render_mattes(s, &cd, &st, nullptr, 4, 0, li, nullptr, lo, nullptr) == RS_E_INVALID);
    CHECK(rs_render_mattes(s, &cd, &st, nullptr, 8, 16, li, lc, nullptr, nullptr) == RS_E_STATE);
    CHECK(rs_render_mattes_device(s, &cd, &st, nullptr, 8, 16, li, lc, lo, nullptr, nullptr) == RS_E_STATE);
    std::printf("ok\n");
    return 0;
}
