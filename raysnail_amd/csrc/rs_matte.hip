// rs_matte.hip — the matte of a set of material ids from rs_render_mattes' ranked (id, coverage) layers
// (rs_matte_extract_device); the contract is in include/raysnail_hip.h. f32, every addition rounded once. Scene-free:
// no rs_device.h.
//
// One thread per pixel: it reads its `ranks` (id, coverage) pairs (a wave reads 64 ranks consecutive dwords of each
// array), tests each id against the wanted ids, which ride in the argument block and are read with scalar loads (k is
// wave-uniform), and writes one float. The kernel is bound by the 8 ranks + 4 bytes per pixel it moves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_frame_dev.h"
#include "../../include/raysnail_hip.h"

namespace rs {
namespace {

struct Wanted {
    int32_t id[kMaxWanted];
};

__global__ __launch_bounds__(kBlock) void k_matte_extract(const int32_t* __restrict__ ids, const float* __restrict__ cov,
                                                          const uint32_t n_pix, const uint32_t ranks, const Wanted w,
                                                          const uint32_t n_wanted, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= n_pix) return;
    const uint64_t base = (uint64_t)p * ranks;
    float a = 0.f;
    for (uint32_t r = 0; r < ranks; ++r) {
        const int32_t id = ids[base + r];
        const float c = cov[base + r];
        bool in = false;
        for (uint32_t k = 0; k < n_wanted; ++k) in = in || w.id[k] == id;
        a = in && id != RS_MATTE_ID_EMPTY ? a + c : a;
    }
    out[p] = a;
}

}  // namespace

hipError_t launch_matte_extract(const int32_t* ids, const float* cov, uint32_t n_pix, uint32_t ranks, const int32_t* wanted,
                                uint32_t n_wanted, float* out, hipStream_t st) {
    Wanted w;
    for (uint32_t k = 0; k < (uint32_t)kMaxWanted; ++k) w.id[k] = wanted[k < n_wanted ? k : 0];  // (the rest: never read)
    k_matte_extract<<<dim3((n_pix + kBlock - 1) / kBlock), dim3(kBlock), 0, st>>>(ids, cov, n_pix, ranks, w, n_wanted, out);
    return hipGetLastError();
}

}  // namespace rs
