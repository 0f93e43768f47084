/*
 * raysnail_adaptive.h -- adaptive sampling for the progressive pass loop: part of libraysnail_hip.so's C-ABI
 * (additive extensions of ABI 6; rs_abi_version() stays 6). include/raysnail_hip.h includes this header, and this
 * header includes that one: either include gives the whole boundary. Conventions (status codes, rs_last_error, frame
 * layout, streams) are raysnail_hip.h's.
 */
#ifndef RAYSNAIL_ADAPTIVE_H
#define RAYSNAIL_ADAPTIVE_H

#include "raysnail_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- adaptive sampling: running per-pixel moments and a variance-driven sample mask for the progressive pass loop
 * (no reference counterpart: upstream's redo map is never applied, src/bin/raysnail.rs:404-427) ----
 * Scene-free kernels (rs_moments_update, rs_moments_resolve, rs_adaptive_mask) and the loop over rs_render_device's
 * pixel mask that they drive (rs_render_adaptive[_device]). Frames are W*H RGBA f32. Arithmetic: all f32, every
 * operation rounded once (IEEE division and square root, denormals kept, no contraction), no transcendental function;
 * a + b + c without brackets is never written. Every function: W H = 0 or > 0x7FFFFFFF is RS_E_INVALID, as every
 * invalid argument is before anything touches the device. Additive extensions of ABI 6.
 *
 * State: two frames owned by the caller. acc[p] = [mu_r, mu_g, mu_b, n]: the mean in linear radiance and the sample
 * (pass) count as a float; m2[p] = [M2_r, M2_g, M2_b, 0]: the sums of squared deviations. A zero-filled pair is the
 * empty state.
 *
 * rs_moments_update_device: Welford's update of the state with n_frames frames. d_frames is a HOST array of 1 .. 64
 * device pointers; they travel in the kernel's argument block. One launch on `stream` (hipStream_t, NULL = default) of
 * the current device; never synchronises, allocates nothing. Per pixel, for frame k = 0 .. n_frames-1 in that order,
 * with F_k = frame k's pixel:
 *   frame k contributes when F_k.a != 0 and F_k.rgb are finite (rs_pass_moments' convention: a masked pixel and a NaN
 *   pixel add nothing)
 *   x = F_k.rgb; gamma == 1: x = x x per channel (moments of linear radiance)
 *   n1 = n + 1;  d = x - mu;  mu' = mu + d / n1;  e = x - mu';  M2' = M2 + (d e) (the product rounded, then the
 *   addition);  n = n1                                                       -- per channel
 * m2.w is written as +0.0. A pixel that no frame contributes to keeps its state bit for bit (it is not written). The
 * frames must not overlap the state. RS_E_INVALID: NULL state; frames NULL or a NULL frame pointer; n_frames outside
 * 1 .. 64; gamma not 0 or 1.
 *
 * rs_moments_resolve_device: the state as rs_pass_moments' two frames, which rs_denoise_var consumes unchanged:
 *   mean[p] = [mu (gamma == 1: sqrt(mu) per channel), 1.0] for n >= 1, [0,0,0,0] otherwise
 *   var[p]  = [M2 / (n (n - 1)) per channel, n] for n >= 2 (the product rounded once: exact for n <= 4096),
 *             [0,0,0,n] otherwise: the variance of the mean, linear radiance, never gamma
 * Either output may be NULL, not both. d_mean and d_var may alias neither state frame nor each other. One launch, never
 * synchronises, allocates nothing.
 *
 * rs_adaptive_mask_device: where the next pass samples. tol2 = tolerance tolerance, on the host in f32. Per pixel q,
 * with n = acc[q].w (compared as a float with min_n and max_n, which convert exactly) and base(q) = d_base[q] (NULL:
 * all ones):
 *   fin(q)  = the three mu and the three M2 are finite
 *   t = (M2_r + M2_g) + M2_b;  v = t / (n (n - 1));  L = (mu_r + mu_g) + mu_b;  Dn = max(L, floor);
 *   err2(q) = v / (Dn Dn)                                   -- read for n >= 2 and fin(q) only
 *   (the squared standard error of the mean's channel sum, relative to the pixel's own level; `floor` keeps dark
 *   pixels from asking for samples without end)
 *   hot(q)  = base(q) != 0 and n < max_n and (n < min_n or (fin(q) and err2(q) > tol2))
 *   A pixel whose state is not finite is never hot once it has min_n samples.
 *   mask[p] = 1 when base(p) != 0 and n_p < max_n and some q with |dx|, |dy| <= radius inside the frame has hot(q),
 *             0 otherwise (a variance estimated from a few samples is itself noisy: a converged-looking pixel next to
 *             an unconverged one keeps sampling)
 * stats (may be NULL): active = the mask bytes that are 1; hot = the hot pixels; nonfinite = the pixels with
 * base != 0 whose state is not finite; max_err2 = the maximum of err2 over the pixels with base != 0, n >= 2 and fin,
 * +0.0 if there are none (values that do not compare > 0 -- a NaN from inf / inf, a negative M2 -- take no part).
 * Counts are integer atomics and the maximum an integer atomic max on the float's bits: exact, order-independent.
 * With stats != NULL the call allocates its counters and synchronises the stream to return them, as
 * rs_noise_map_device does; with stats == NULL it is one launch and neither allocates nor synchronises.
 * RS_E_INVALID: min_n < 2; max_n < min_n or max_n > 4096; tolerance or floor not finite or outside [1e-6, 1e4];
 * radius > 4; NULL state or NULL mask.
 *
 * rs_render_adaptive_device: the loop. For p = 0, 1, ...:
 *   1. rs_adaptive_mask_device on the state into d_work_mask, with min_n = min_passes, max_n = max_passes, base =
 *      d_base_mask (its statistics are read back: one stream synchronisation per pass)
 *   2. stop when active == 0 or p == max_passes
 *   3. render pass st->pass + p under that mask into d_work_frame, exactly as rs_render_device does (so a sampled pixel
 *      is bit for bit the maskless pass frame's pixel, and a masked one traces nothing)
 *   4. rs_moments_update_device with that one frame and st->gamma
 * The caller zero-fills d_acc and d_m2 for a fresh image; a non-empty state continues an earlier run (the caller then
 * advances st->pass past the passes already spent, and a pixel's n never passes max_passes). d_work_frame = W H 4
 * floats, d_work_mask = W H bytes, caller memory; nothing is allocated beyond what rs_render_device allocates (the
 * mask's counters live in d_work_frame between the passes). passes_out (max_passes entries, or NULL) receives one
 * report per rendered pass: the mask's active and hot counts and max_err2 before the pass, and the pass's render
 * statistics (with passes_out == NULL the renders take no statistics). n_passes_out (may be NULL) = the passes
 * rendered. Pointers, stream and devices as rs_render_device: with several devices the state, the work buffers and the
 * stream belong to the first listed one. The row lattice of st (row_begin, row_end, row_step) is part of the base mask:
 * rs_render_device leaves rows off it untouched, so their pixels are never hot, never sampled, counted in no
 * statistic, and keep their state bit for bit. d_work_frame is zeroed on entry and holds [0,0,0,0] wherever the last
 * pass did not sample (and in its first pixel) on return. Afterwards rs_moments_resolve_device gives the image.
 * RS_E_INVALID as rs_adaptive_mask_device's settings and rs_render_device's arguments; RS_E_STATE as rs_render_device.
 * Checking the mask only every c passes (to save the per-pass synchronisation) is deliberately left out.
 *
 * rs_render_adaptive: host buffers, a fresh state. base_mask = W H bytes or NULL; mean and var = rs_moments_resolve's
 * frames (either may be NULL, not both). Owns its device memory (on the first listed device).
 *
 * Defaults (RS_ADAPTIVE_*): the point of tools/adaptive_quality.py's grid with the largest smallest margin over its
 * four cells (profiles/adaptive/quality.txt); max passes 32 is the grid's own bound. */
#define RS_ADAPTIVE_MIN_PASSES ((uint32_t)2)
#define RS_ADAPTIVE_MAX_PASSES ((uint32_t)32)
#define RS_ADAPTIVE_RADIUS     ((uint32_t)1)
#define RS_ADAPTIVE_TOLERANCE  ((float)0.1)
#define RS_ADAPTIVE_FLOOR      ((float)0.03)
typedef struct rs_adaptive_stats {
    uint64_t active, hot, nonfinite;
    float    max_err2;
} rs_adaptive_stats;
typedef struct rs_adaptive_settings {
    uint32_t min_passes, max_passes, radius;
    float    tolerance, floor;
} rs_adaptive_settings;
typedef struct rs_adaptive_pass {
    uint64_t active, hot;     /* the mask the pass rendered under */
    float    max_err2;
    rs_render_stats stats;    /* the pass's render */
} rs_adaptive_pass;
int rs_moments_update_device(float* d_acc, float* d_m2, const float* const* d_frames, uint32_t n_frames,
                             uint32_t width, uint32_t height, int32_t gamma, void* stream);
int rs_moments_resolve_device(const float* d_acc, const float* d_m2, uint32_t width, uint32_t height, int32_t gamma,
                              float* d_mean, float* d_var, void* stream);
int rs_adaptive_mask_device(const float* d_acc, const float* d_m2, const uint8_t* d_base, uint32_t width,
                            uint32_t height, uint32_t min_n, uint32_t max_n, float tolerance, float floor,
                            uint32_t radius, uint8_t* d_mask, void* stream, rs_adaptive_stats* stats);
int rs_render_adaptive_device(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st,
                              const rs_adaptive_settings* as, const uint8_t* d_base_mask, float* d_acc, float* d_m2,
                              float* d_work_frame, uint8_t* d_work_mask, void* stream, rs_adaptive_pass* passes_out,
                              uint32_t* n_passes_out);
int rs_render_adaptive(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st,
                       const rs_adaptive_settings* as, const uint8_t* base_mask, float* mean, float* var,
                       rs_adaptive_pass* passes_out, uint32_t* n_passes_out);

#ifdef __cplusplus
}
#endif
#endif /* RAYSNAIL_ADAPTIVE_H */
