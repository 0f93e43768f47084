// rs_frames.cpp — the C-ABI of the frame operators (include/raysnail_hip.h, raysnail_adaptive.h): the pass combine, the
// noise map, the two denoisers, the pass moments and their robust form, the running moments and the sample mask, the matte of a set of ids. None
// of them touches an rs_scene. Each operator is a checked core (<name>_device: argument checks, then the launches of
// rs_internal.h), its `_device` entry (run around the core) and, where the ABI has one, a host entry that stages the
// caller's arrays in one device allocation, calls the core on the null stream and copies the results back. Argument
// checks come before anything touches a device.
#include <cstring>
#include <string>

#include "rs_host_util.h"
#include "rs_internal.h"

using namespace rs;

namespace {

// Device memory that work on `stream` uses: the stream is drained before the memory is freed, on every path.
struct StreamMem {
    hipStream_t stream;
    DeviceMem mem;
    StreamMem(size_t bytes, hipStream_t st) : stream(st), mem(device_alloc(bytes)) {}
    ~StreamMem() { (void)hipStreamSynchronize(stream); }
};

// A host entry's one allocation (null stream), carved front to back: RGBA f32 frames first, then byte planes.
struct Staging : StreamMem {
    size_t n_pix, frame_bytes;
    char* next;
    Staging(uint32_t width, uint32_t height, size_t frames, size_t planes)  // (+ 16: never an empty allocation)
        : StreamMem((size_t)width * height * (4 * sizeof(float) * frames + planes) + 16, nullptr),
          n_pix((size_t)width * height), frame_bytes(n_pix * 4 * sizeof(float)), next(static_cast<char*>(mem.get())) {}
    float* frame(size_t count = 1) { float* d = reinterpret_cast<float*>(next); next += count * frame_bytes; return d; }
    uint8_t* plane() { uint8_t* d = reinterpret_cast<uint8_t*>(next); next += n_pix; return d; }
    // a frame holding the caller's; null for a null one
    float* upload(const float* host) {
        if (!host) return nullptr;
        float* d = frame();
        HIP_OK(hipMemcpy(d, host, frame_bytes, hipMemcpyHostToDevice));
        return d;
    }
    // back into an output the caller asked for (a frame, or a byte plane)
    void download(void* host, const void* d, size_t bytes) {
        if (host) HIP_OK(hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost));
    }
    void download(float* host, const float* d) { download(host, d, frame_bytes); }
    void download(uint8_t* host, const uint8_t* d) { download(host, d, n_pix); }
    void sync() { HIP_OK(hipStreamSynchronize(stream)); }
};

}  // namespace

// ---- argument checks ----
void rs::validate_frame_size(uint32_t width, uint32_t height, const char* what) {
    const uint64_t n = (uint64_t)width * height;
    if (n == 0) throw Error(RS_E_INVALID, std::string(what) + ": empty frame");
    if (n > 0x7FFFFFFFull) throw Error(RS_E_INVALID, std::string(what) + ": frame too large");
}

void rs::validate_adaptive(uint32_t min_n, uint32_t max_n, float tolerance, float floor, uint32_t radius) {
    if (min_n < 2) throw Error(RS_E_INVALID, "adaptive: min passes below 2");
    if (max_n < min_n || max_n > 4096) throw Error(RS_E_INVALID, "adaptive: max passes below min passes or above 4096");
    for (float v : {tolerance, floor})
        if (!(v >= 1e-6f && v <= 1e4f)) throw Error(RS_E_INVALID, "adaptive: tolerance or floor not finite or outside [1e-6, 1e4]");
    if (radius > 4) throw Error(RS_E_INVALID, "adaptive: radius above 4");
}

namespace {

// both denoisers' (everything but the buffers; sigma_color is rs_denoise_var's k_color)
void validate_denoise(uint32_t width, uint32_t height, uint32_t levels, float sigma_color, float sigma_normal,
                      float sigma_depth, int32_t gamma) {
    if (levels < 1 || levels > 8) throw Error(RS_E_INVALID, "denoise: levels outside 1 .. 8");
    for (float sg : {sigma_color, sigma_normal, sigma_depth})
        if (!(sg >= 1e-4f && sg <= 1e4f)) throw Error(RS_E_INVALID, "denoise: sigma not finite or outside [1e-4, 1e4]");
    if (gamma != 0 && gamma != 1) throw Error(RS_E_INVALID, "denoise: gamma is not 0 or 1");
    validate_frame_size(width, height, "denoise");
}

// An operator `op` over a list of frames. trim_ok: pass_robust's own check, which fires before the frame's size;
// other_null: a null among the operator's other required pointers; no_output: every output is null.
void validate_frame_list(const char* op, const float* const* frames, uint32_t n_frames, uint32_t width, uint32_t height,
                         int32_t gamma, bool trim_ok, bool other_null, bool no_output) {
    const std::string what(op);
    static_assert(kMaxFrames == 64, "the message below");
    if (n_frames < 1 || n_frames > (uint32_t)kMaxFrames) throw Error(RS_E_INVALID, what + ": n_frames outside 1 .. 64");
    if (gamma != 0 && gamma != 1) throw Error(RS_E_INVALID, what + ": gamma is not 0 or 1");
    if (!trim_ok) throw Error(RS_E_INVALID, what + ": trim is neither RS_ROBUST_TRIM_AUTO nor in [0, 0.5]");
    validate_frame_size(width, height, op);
    if (!frames || other_null) throw Error(RS_E_INVALID, what + ": null argument");
    for (uint32_t k = 0; k < n_frames; ++k)
        if (!frames[k]) throw Error(RS_E_INVALID, what + ": null frame pointer");
    if (no_output) throw Error(RS_E_INVALID, what + ": null argument (both outputs)");
}
// (a NaN fails both)
bool trim_ok(float trim) { return trim == RS_ROBUST_TRIM_AUTO || (trim >= 0.0f && trim <= 0.5f); }

// ---- the checked cores ----
void noise_map_device(const float* d_rgba, uint32_t width, uint32_t height, float threshold, uint8_t* d_redo,
                      hipStream_t st, rs_noise_stats* stats) {
    if (!d_rgba) throw Error(RS_E_INVALID, "null argument");
    if ((uint64_t)width * height > 0x7FFFFFFFull) throw Error(RS_E_INVALID, "frame too large");
    // [0] min bits, [1] max bits (non-negative floats order like their bit patterns), [2..3] count
    StreamMem cnt(4 * sizeof(unsigned int), st);
    unsigned int* d = static_cast<unsigned int*>(cnt.mem.get());
    const float lim[2] = {3.0f, 1.0f};  // raysnail.rs:396-397
    unsigned int init[4] = {0, 0, 0, 0};
    std::memcpy(init, lim, sizeof(lim));
    HIP_OK(hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, st));
    unsigned long long* d_count = reinterpret_cast<unsigned long long*>(d + 2);
    HIP_OK(launch_noise(d_rgba, (int)width, (int)height, threshold, d_redo, d, d_count, st));
    unsigned int out[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(out, d, sizeof(out), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (stats) {
        std::memcpy(&stats->min, &out[0], 4);
        std::memcpy(&stats->max, &out[1], 4);
        uint64_t c;
        std::memcpy(&c, &out[2], 8);
        stats->count = c;
    }
}

void denoise_device(const float* d_beauty, const float* d_albedo, const float* d_normal, uint32_t width, uint32_t height,
                    uint32_t levels, float sigma_color, float sigma_normal, float sigma_depth, int32_t gamma, float* d_out,
                    float* d_work, hipStream_t st) {
    validate_denoise(width, height, levels, sigma_color, sigma_normal, sigma_depth, gamma);
    if (!d_beauty || !d_out || !d_work) throw Error(RS_E_INVALID, "denoise: null argument");
    // the contract's constants, in f32 (the colour sigma halves per level: an exact scaling)
    float ic[8];
    float sc = sigma_color;
    for (uint32_t i = 0; i < levels; ++i, sc = sc * 0.5f) ic[i] = 1.0f / (sc * sc);
    const float inv_n = 1.0f / (sigma_normal * sigma_normal), inv_d = 1.0f / (sigma_depth * sigma_depth);
    HIP_OK(launch_denoise(d_beauty, d_albedo, d_normal, width, height, levels, ic, inv_n, inv_d, gamma, d_out, d_work,
                          st));
}

void denoise_var_device(const float* d_beauty, const float* d_var, const float* d_albedo, const float* d_normal,
                        uint32_t width, uint32_t height, uint32_t levels, float k_color, float sigma_normal,
                        float sigma_depth, int32_t gamma, float* d_out, float* d_out_var, float* d_work, hipStream_t st) {
    validate_denoise(width, height, levels, k_color, sigma_normal, sigma_depth, gamma);
    if (!d_beauty || !d_var || !d_out || !d_work) throw Error(RS_E_INVALID, "denoise: null argument");
    const float inv_n = 1.0f / (sigma_normal * sigma_normal), inv_d = 1.0f / (sigma_depth * sigma_depth);
    HIP_OK(launch_denoise_var(d_beauty, d_var, d_albedo, d_normal, width, height, levels, k_color, inv_n, inv_d, gamma,
                              d_out, d_out_var, d_work, st));
}

void pass_moments_device(const float* const* d_frames, uint32_t n_frames, uint32_t width, uint32_t height, int32_t gamma,
                         float* d_mean, float* d_var, hipStream_t st) {
    validate_frame_list("pass_moments", d_frames, n_frames, width, height, gamma, true, false, !d_mean && !d_var);
    HIP_OK(launch_pass_moments(d_frames, n_frames, width * height, gamma, d_mean, d_var, st));
}

void pass_robust_device(const float* const* d_frames, uint32_t n_frames, uint32_t width, uint32_t height, int32_t gamma,
                        float trim, float* d_mean, float* d_var, uint8_t* d_trimmed, hipStream_t st) {
    validate_frame_list("pass_robust", d_frames, n_frames, width, height, gamma, trim_ok(trim), false, !d_mean && !d_var);
    HIP_OK(launch_pass_robust(d_frames, n_frames, width * height, gamma, trim, d_mean, d_var, d_trimmed, st));
}

// (wanted is a host array in both entries: the checks may read it)
void validate_matte_extract(const int32_t* ids, const float* cov, uint32_t width, uint32_t height, uint32_t ranks,
                            const int32_t* wanted, uint32_t n_wanted, const float* out) {
    if (ranks < 1 || ranks > RS_MATTE_MAX_RANKS) throw Error(RS_E_INVALID, "matte_extract: ranks outside 1 .. 8");
    static_assert(RS_MATTE_MAX_RANKS == 8 && kMaxWanted == 64, "the messages here");
    if (n_wanted < 1 || n_wanted > (uint32_t)kMaxWanted) throw Error(RS_E_INVALID, "matte_extract: n_wanted outside 1 .. 64");
    validate_frame_size(width, height, "matte_extract");
    if (!ids || !cov || !wanted || !out) throw Error(RS_E_INVALID, "matte_extract: null argument");
}
void matte_extract_device(const int32_t* d_ids, const float* d_cov, uint32_t width, uint32_t height, uint32_t ranks,
                          const int32_t* wanted, uint32_t n_wanted, float* d_out, hipStream_t st) {
    validate_matte_extract(d_ids, d_cov, width, height, ranks, wanted, n_wanted, d_out);
    HIP_OK(launch_matte_extract(d_ids, d_cov, width * height, ranks, wanted, n_wanted, d_out, st));
}

}  // namespace

void rs::adaptive_mask_stats(const float* d_acc, const float* d_m2, const uint8_t* d_base, uint32_t width, uint32_t height,
                             uint32_t min_n, uint32_t max_n, float tol2, float floor, uint32_t radius, uint8_t* d_mask,
                             unsigned int* d_counters, hipStream_t st, rs_adaptive_stats* stats, uint32_t row_begin,
                             uint32_t row_end, uint32_t row_step) {
    HIP_OK(hipMemsetAsync(d_counters, 0, 4 * sizeof(unsigned int), st));
    HIP_OK(launch_adaptive_mask(d_acc, d_m2, d_base, width, height, min_n, max_n, tol2, floor, radius, d_mask, d_counters, st,
                                row_begin, row_end, row_step));
    unsigned int out[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(out, d_counters, sizeof(out), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemsetAsync(d_counters, 0, 4 * sizeof(unsigned int), st));  // (left as an all-zero pixel: see the loop)
    HIP_OK(hipStreamSynchronize(st));
    stats->active = out[0];
    stats->hot = out[1];
    stats->nonfinite = out[2];
    std::memcpy(&stats->max_err2, &out[3], 4);
}

// ---- the C-ABI ----
extern "C" {

int rs_combine_pixels_device(float* d_acc, const float* d_new, uint64_t n_pixels, float pass, void* stream) {
    return run([&] {
        if (!d_acc || !d_new) throw Error(RS_E_INVALID, "null argument");
        HIP_OK(launch_combine(d_acc, d_new, n_pixels, pass, (hipStream_t)stream));
    });
}

int rs_noise_map_device(const float* d_rgba, uint32_t width, uint32_t height, float threshold, uint8_t* d_redo,
                        void* stream, rs_noise_stats* stats) {
    return run([&] { noise_map_device(d_rgba, width, height, threshold, d_redo, (hipStream_t)stream, stats); });
}

int rs_noise_map(const float* rgba, uint32_t width, uint32_t height, float threshold, uint8_t* redo,
                 rs_noise_stats* stats) {
    return run([&] {
        if (!rgba) throw Error(RS_E_INVALID, "null argument");
        Staging s(width, height, 1, 1);
        const float* d_px = s.upload(rgba);
        uint8_t* d_redo = s.plane();  // (the kernel always writes it)
        noise_map_device(d_px, width, height, threshold, d_redo, s.stream, stats);
        s.download(redo, d_redo);
    });
}

int rs_denoise_device(const float* d_beauty, const float* d_albedo, const float* d_normal, uint32_t width, uint32_t height,
                      uint32_t levels, float sigma_color, float sigma_normal, float sigma_depth, int32_t gamma,
                      float* d_out, float* d_work, void* stream) {
    return run([&] {
        denoise_device(d_beauty, d_albedo, d_normal, width, height, levels, sigma_color, sigma_normal, sigma_depth, gamma,
                       d_out, d_work, (hipStream_t)stream);
    });
}

int rs_denoise(const float* beauty, const float* albedo, const float* normal, uint32_t width, uint32_t height,
               uint32_t levels, float sigma_color, float sigma_normal, float sigma_depth, int32_t gamma, float* out) {
    return run([&] {
        validate_denoise(width, height, levels, sigma_color, sigma_normal, sigma_depth, gamma);
        if (!beauty || !out) throw Error(RS_E_INVALID, "denoise: null argument");
        Staging s(width, height, 5, 0);  // beauty (the output, in place), albedo, normal, the two work planes
        float* d_beauty = s.upload(beauty);
        const float* d_albedo = s.upload(albedo);
        const float* d_normal = s.upload(normal);
        denoise_device(d_beauty, d_albedo, d_normal, width, height, levels, sigma_color, sigma_normal, sigma_depth, gamma,
                       d_beauty, s.frame(2), s.stream);
        s.sync();
        s.download(out, d_beauty);
    });
}

int rs_pass_moments_device(const float* const* d_frames, uint32_t n_frames, uint32_t width, uint32_t height, int32_t gamma,
                           float* d_mean, float* d_var, void* stream) {
    return run([&] { pass_moments_device(d_frames, n_frames, width, height, gamma, d_mean, d_var, (hipStream_t)stream); });
}

int rs_pass_moments(const float* const* frames, uint32_t n_frames, uint32_t width, uint32_t height, int32_t gamma,
                    float* mean, float* var) {
    return run([&] {
        validate_frame_list("pass_moments", frames, n_frames, width, height, gamma, true, false, !mean && !var);
        Staging s(width, height, (size_t)n_frames + 2, 0);  // the frames, then the mean and the variance
        const float* d_frames[kMaxFrames];
        for (uint32_t k = 0; k < n_frames; ++k) d_frames[k] = s.upload(frames[k]);
        float* d_mean = mean ? s.frame() : nullptr;
        float* d_var = var ? s.frame() : nullptr;
        pass_moments_device(d_frames, n_frames, width, height, gamma, d_mean, d_var, s.stream);
        s.sync();
        s.download(mean, d_mean);
        s.download(var, d_var);
    });
}

int rs_pass_robust_device(const float* const* d_frames, uint32_t n_frames, uint32_t width, uint32_t height, int32_t gamma,
                          float trim, float* d_mean, float* d_var, uint8_t* d_trimmed, void* stream) {
    return run([&] {
        pass_robust_device(d_frames, n_frames, width, height, gamma, trim, d_mean, d_var, d_trimmed, (hipStream_t)stream);
    });
}

int rs_pass_robust(const float* const* frames, uint32_t n_frames, uint32_t width, uint32_t height, int32_t gamma,
                   float trim, float* mean, float* var, uint8_t* trimmed) {
    return run([&] {
        validate_frame_list("pass_robust", frames, n_frames, width, height, gamma, trim_ok(trim), false, !mean && !var);
        Staging s(width, height, (size_t)n_frames + 2, 1);  // the frames, the mean, the variance; the trim counts
        const float* d_frames[kMaxFrames];
        for (uint32_t k = 0; k < n_frames; ++k) d_frames[k] = s.upload(frames[k]);
        float* d_mean = mean ? s.frame() : nullptr;
        float* d_var = var ? s.frame() : nullptr;
        uint8_t* d_trimmed = trimmed ? s.plane() : nullptr;
        pass_robust_device(d_frames, n_frames, width, height, gamma, trim, d_mean, d_var, d_trimmed, s.stream);
        s.sync();
        s.download(mean, d_mean);
        s.download(var, d_var);
        s.download(trimmed, d_trimmed);
    });
}

int rs_denoise_var_device(const float* d_beauty, const float* d_var, const float* d_albedo, const float* d_normal,
                          uint32_t width, uint32_t height, uint32_t levels, float k_color, float sigma_normal,
                          float sigma_depth, int32_t gamma, float* d_out, float* d_out_var, float* d_work, void* stream) {
    return run([&] {
        denoise_var_device(d_beauty, d_var, d_albedo, d_normal, width, height, levels, k_color, sigma_normal, sigma_depth,
                           gamma, d_out, d_out_var, d_work, (hipStream_t)stream);
    });
}

int rs_denoise_var(const float* beauty, const float* var, const float* albedo, const float* normal, uint32_t width,
                   uint32_t height, uint32_t levels, float k_color, float sigma_normal, float sigma_depth, int32_t gamma,
                   float* out, float* out_var) {
    return run([&] {
        validate_denoise(width, height, levels, k_color, sigma_normal, sigma_depth, gamma);
        if (!beauty || !var || !out) throw Error(RS_E_INVALID, "denoise: null argument");
        Staging s(width, height, 8, 0);  // beauty and var (the outputs, in place), albedo, normal, the four work planes
        float* d_beauty = s.upload(beauty);
        float* d_var = s.upload(var);
        const float* d_albedo = s.upload(albedo);
        const float* d_normal = s.upload(normal);
        denoise_var_device(d_beauty, d_var, d_albedo, d_normal, width, height, levels, k_color, sigma_normal, sigma_depth,
                           gamma, d_beauty, out_var ? d_var : nullptr, s.frame(4), s.stream);
        s.sync();
        s.download(out, d_beauty);
        s.download(out_var, d_var);
    });
}

int rs_matte_extract_device(const int32_t* d_ids, const float* d_cov, uint32_t width, uint32_t height, uint32_t ranks,
                            const int32_t* wanted, uint32_t n_wanted, float* d_out, void* stream) {
    return run([&] { matte_extract_device(d_ids, d_cov, width, height, ranks, wanted, n_wanted, d_out, (hipStream_t)stream); });
}

int rs_matte_extract(const int32_t* ids, const float* cov, uint32_t width, uint32_t height, uint32_t ranks,
                     const int32_t* wanted, uint32_t n_wanted, float* out) {
    return run([&] {
        validate_matte_extract(ids, cov, width, height, ranks, wanted, n_wanted, out);
        const size_t n_pix = (size_t)width * height, layer = n_pix * ranks * 4;  // the ids, the coverages, the matte
        StreamMem m(2 * layer + n_pix * sizeof(float), nullptr);
        char* const base = static_cast<char*>(m.mem.get());
        int32_t* const d_ids = reinterpret_cast<int32_t*>(base);
        float* const d_cov = reinterpret_cast<float*>(base + layer);
        float* const d_out = reinterpret_cast<float*>(base + 2 * layer);
        HIP_OK(hipMemcpy(d_ids, ids, layer, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_cov, cov, layer, hipMemcpyHostToDevice));
        matte_extract_device(d_ids, d_cov, width, height, ranks, wanted, n_wanted, d_out, m.stream);
        HIP_OK(hipStreamSynchronize(m.stream));
        HIP_OK(hipMemcpy(out, d_out, n_pix * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int rs_moments_update_device(float* d_acc, float* d_m2, const float* const* d_frames, uint32_t n_frames, uint32_t width,
                             uint32_t height, int32_t gamma, void* stream) {
    return run([&] {
        validate_frame_list("moments_update", d_frames, n_frames, width, height, gamma, true, !d_acc || !d_m2, false);
        HIP_OK(launch_moments_update(d_acc, d_m2, d_frames, n_frames, width * height, gamma, (hipStream_t)stream));
    });
}

int rs_moments_resolve_device(const float* d_acc, const float* d_m2, uint32_t width, uint32_t height, int32_t gamma,
                              float* d_mean, float* d_var, void* stream) {
    return run([&] {
        if (gamma != 0 && gamma != 1) throw Error(RS_E_INVALID, "moments_resolve: gamma is not 0 or 1");
        validate_frame_size(width, height, "moments_resolve");
        if (!d_acc || !d_m2) throw Error(RS_E_INVALID, "moments_resolve: null argument");
        if (!d_mean && !d_var) throw Error(RS_E_INVALID, "moments_resolve: null argument (both outputs)");
        HIP_OK(launch_moments_resolve(d_acc, d_m2, width * height, gamma, d_mean, d_var, (hipStream_t)stream));
    });
}

int rs_adaptive_mask_device(const float* d_acc, const float* d_m2, const uint8_t* d_base, uint32_t width, uint32_t height,
                            uint32_t min_n, uint32_t max_n, float tolerance, float floor, uint32_t radius, uint8_t* d_mask,
                            void* stream, rs_adaptive_stats* stats) {
    return run([&] {
        validate_adaptive(min_n, max_n, tolerance, floor, radius);
        validate_frame_size(width, height, "adaptive_mask");
        if (!d_acc || !d_m2 || !d_mask) throw Error(RS_E_INVALID, "adaptive_mask: null argument");
        const float tol2 = tolerance * tolerance;
        const hipStream_t st = (hipStream_t)stream;
        if (!stats) {
            HIP_OK(launch_adaptive_mask(d_acc, d_m2, d_base, width, height, min_n, max_n, tol2, floor, radius, d_mask,
                                        nullptr, st, 0, height, 1));
            return;
        }
        StreamMem cnt(4 * sizeof(unsigned int), st);
        adaptive_mask_stats(d_acc, d_m2, d_base, width, height, min_n, max_n, tol2, floor, radius, d_mask,
                            static_cast<unsigned int*>(cnt.mem.get()), st, stats, 0, height, 1);
    });
}

}  // extern "C"
