// rs_host_util.h — what the host units of libraysnail_hip.so share (rs_host.cpp: scenes and rendering; rs_frames.cpp:
// the scene-free frame operators): how an entry point reports an error, and the owners of what a call creates for
// itself. Host only; not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../include/raysnail_hip.h"

namespace rs {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIP_OK(x)                                                                                               \
    do {                                                                                                        \
        hipError_t e_ = (x);                                                                                    \
        if (e_ != hipSuccess) throw ::rs::Error(RS_E_HIP, std::string(#x " failed: ") + hipGetErrorString(e_)); \
    } while (0)

// An entry point's body: RS_OK, or the code of what it threw, whose message becomes the calling thread's
// rs_last_error() (rs_host.cpp: the one definition of that string).
int run(const std::function<void()>& f);

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        HIP_OK(hipGetDevice(&prev));
        if (prev != dev) HIP_OK(hipSetDevice(dev));
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// Owners of what a call creates for itself (move-only). An entry point drains what it enqueued before these go out
// of scope on an error: that work may still use them.
template <class T, hipError_t (*Free)(T*)>
struct HipFree { void operator()(T* p) const { (void)Free(p); } };
using Event = std::unique_ptr<ihipEvent_t, HipFree<ihipEvent_t, hipEventDestroy>>;
using DeviceMem = std::unique_ptr<void, HipFree<void, hipFree>>;
using PinnedMem = std::unique_ptr<void, HipFree<void, hipHostFree>>;
inline DeviceMem device_alloc(size_t bytes) {
    void* d = nullptr;
    HIP_OK(hipMalloc(&d, bytes));
    return DeviceMem(d);
}

// rs_frames.cpp, for rs_render_adaptive[_device] (which need a scene and stay in rs_host.cpp)
void validate_frame_size(uint32_t width, uint32_t height, const char* what);
void validate_adaptive(uint32_t min_n, uint32_t max_n, float tolerance, float floor, uint32_t radius);
// The mask launch with its statistics read back through `d_counters`: 16 bytes of device memory (one pixel of a frame)
// that the stream may overwrite at this point. The rows that count as base: rs_internal.h launch_adaptive_mask.
// Synchronises the stream.
void adaptive_mask_stats(const float* d_acc, const float* d_m2, const uint8_t* d_base, uint32_t width, uint32_t height,
                         uint32_t min_n, uint32_t max_n, float tol2, float floor, uint32_t radius, uint8_t* d_mask,
                         unsigned int* d_counters, hipStream_t st, rs_adaptive_stats* stats, uint32_t row_begin,
                         uint32_t row_end, uint32_t row_step);

}  // namespace rs
