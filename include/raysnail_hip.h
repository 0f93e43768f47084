/*
 * raysnail_hip.h — C-ABI of libraysnail_hip.so, the MI355X (gfx950) render path.
 *
 * This is the drop-in boundary for raysnail's per-pixel render path
 *   Painter::draw sample loop -> Camera::ray -> Hittable::hit (BVH) -> Material::scatter/emitted
 * (reference: src/camera.rs:261-287 TakePhotoSettings::shot_to_target, src/painter.rs:307-336
 * Painter::draw). The GPU cannot call a Rust closure, so the boundary sits at shot_to_target
 * level: the caller flattens World + Camera + settings into plain-old-data through the calls
 * below, then asks for a frame. Every entry point is extern "C", takes plain pointers and sizes,
 * returns an int status (0 = ok, <0 = error) and never throws or aborts across the ABI;
 * rs_last_error() returns a thread-local message for the last failure on the calling thread.
 *
 * Reference interfaces replaced (file:line in Varkalandar/raysnail @ 2024-10-08):
 *   rs_scene_create/destroy  World::new                      src/hittable/collection/world.rs:40-53
 *   rs_material              Lambertian/Metal/DiffuseMetal/Dielectric/DiffuseLight/MixedMaterial
 *                            constructors                      src/material/{lambertian.rs:29-35,
 *                            metal.rs:43-49 (DiffuseMetal), metal.rs:95-100 (Metal), dielectric.rs:38-53,
 *                            light.rs:17-28, mixed_material.rs:32-38, isotropic.rs:15-22,
 *                            blinn_phong.rs:19-28}; textures Color / Checker / Perlin / Image
 *                            src/prelude/color.rs:61-65, src/texture/checker.rs:16-18,
 *                            src/texture/noise.rs, src/texture/image.rs;
 *                            CommonMaterialSettings src/material/mod.rs:41-54
 *   rs_sphere                Sphere::new / with_speed         src/hittable/geometry/sphere.rs:35-48
 *   rs_aarect                AARect::new_xy/new_xz/new_yz     src/hittable/geometry/rect.rs:58-79
 *   rs_box                   Box::new                         src/hittable/geometry/box.rs:40-45
 *   rs_quadric               Quadric::new                     src/hittable/geometry/quadric.rs:46-61
 *   rs_triangles             Triangle::new + set_normals      src/hittable/geometry/triangle_mesh.rs:42-71
 *   rs_raymarcher            RayMarcher::new (Mandelbulb)     src/hittable/geometry/raymarching.rs:33-38
 *   rs_intersection          Intersection::new                src/hittable/csg/intersection.rs:33-39
 *   rs_difference            Difference::new                  src/hittable/csg/difference.rs:32-38
 *   rs_transformed           TfFacade::new + TransformStack   src/hittable/transform/tf_facade.rs:30-37,
 *                                                             transform.rs:16-127
 *   rs_constant_medium       ConstantMedium::new (+ Isotropic) src/hittable/medium/constant.rs:29-39,
 *                                                             src/material/isotropic.rs:15-22
 *   rs_perlin                Perlin::new/scale/smooth/turbulence/marble  src/texture/noise.rs:44-103
 *   rs_image                 Image::new (decoded pixels)      src/texture/image.rs:24-31
 *   rs_world_add             HittableList::add (world list)   src/hittable/collection/list.rs:29-33
 *   rs_lights_add            HittableList::add (lights list)  src/hittable/collection/list.rs:29-33
 *   rs_set_background        World background closure         examples/rtow_13_1.rs:38-41,
 *                                                             src/bin/raysnail.rs:364-367
 *   rs_render                TakePhotoSettings::shot_to_target src/camera.rs:261-287 (CameraBuilder
 *                            src/camera.rs:300-413; Painter src/painter.rs:69-336)
 *   rs_render_device         same, with the frame left in device memory (no PCIe in the timed region)
 *   rs_render_device_passes  the CLI pass loop's renders (no redo map)  src/bin/raysnail.rs:379-427, as one call
 *
 * Output layout is the reference's Vec<[f32;4]>: W*H RGBA float32, row-major, row 0 = top,
 * sqrt-gamma applied when gamma != 0, unclamped, alpha 1.0 for rendered pixels, [0,0,0,0] for
 * pixels whose mask byte is 0 (PixelController::calculate_pixel == false, src/painter.rs:204-210).
 * Rows outside [row_begin, row_end) or not on the row_step lattice are left untouched.
 *
 * Determinism contract (the reference has none: every FastRng is seeded from thread_rng,
 * src/prelude/random.rs:116-121). Sample s of pixel p (linear index y*W+x) draws from its own
 * XorShift128 stream, seeded with rand_core-0.6 seed_from_u64(rs_stream_key(seed, pass, p, s)).
 * Within a sample, draws follow the reference order exactly: render_pixel jitter x then y
 * (painter.rs:167-170), Camera::ray disk rejection + shutter time (camera.rs:77-85), then per
 * bounce of ray_color (camera.rs:156-255). thread_rng draws on the path are taken from the same
 * stream at the same point: Dielectric's Random::normal (dielectric.rs:72) as one gen(),
 * MixedMaterial's next_u32 (mixed_material.rs:44) as one next_u32(). ConstantMedium::hit's
 * Random::normal() (medium/constant.rs:63) is called inside world.hit, where the number of calls
 * depends on the traversal; it is therefore NOT taken from the stream but from a counter-free hash
 * of the stream's state at the start of the segment and the medium's handle (rs_medium_uniform),
 * so every test of one medium within one world.hit sees the same draw, on every backend.
 */
#ifndef RAYSNAIL_HIP_H
#define RAYSNAIL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ABI_VERSION 6

/* ---- status codes ---- */
#define RS_OK             0
#define RS_E_INVALID     -1  /* bad argument / handle */
#define RS_E_NO_LIGHTS   -2  /* a pdf material exists but the lights list is empty (ref: % 0 panic, list.rs:51) */
#define RS_E_HIP         -3  /* HIP runtime error */
#define RS_E_STATE       -4  /* call not allowed in this state (e.g. render before commit) */
#define RS_E_UNSUPPORTED -5  /* construct outside what the GPU path implements */
#define RS_E_NOMEM       -6

/* ---- textures (src/prelude/color.rs:61-65, src/texture/{checker.rs:21-30, noise.rs, image.rs}) ---- */
#define RS_TEX_SOLID   0
#define RS_TEX_CHECKER 1
#define RS_TEX_PERLIN  2  /* data = rs_perlin id; Color(1,1,1,1) * noise (noise.rs:187-211) */
#define RS_TEX_IMAGE   3  /* data = rs_image id; pixel at (u W, (1 - v) H) / 255 (image.rs:34-50) */
typedef struct rs_texture_desc {
    int32_t kind;     /* RS_TEX_SOLID: color = even; RS_TEX_CHECKER: sin(sx)sin(sy)sin(sz) < 0 ? odd : even */
    int32_t data;     /* RS_TEX_PERLIN / RS_TEX_IMAGE: the id returned by rs_perlin / rs_image */
    float   even[4];  /* rgba */
    float   odd[4];   /* rgba */
    double  scale;    /* checker frequency */
} rs_texture_desc;

/* ---- materials (src/material/ *.rs) ---- */
#define RS_MAT_LAMBERTIAN    0
#define RS_MAT_METAL         1
#define RS_MAT_DIFFUSE_METAL 2
#define RS_MAT_DIELECTRIC    3
#define RS_MAT_DIFFUSE_LIGHT 4
#define RS_MAT_MIXED         5
#define RS_MAT_ISOTROPIC     6  /* Isotropic(color = texture.even): SpherePdf (isotropic.rs:25-33) */
#define RS_MAT_BLINN_PHONG   7  /* BlinnPhong(k_specular, exponent, texture): BlinnPhongPdf (blinn_phong.rs:32-42) */
#define RS_NO_MATERIAL      (-1)  /* Option<Arc<dyn Material>> = None */

typedef struct rs_material_desc {
    int32_t kind;
    int32_t glass;            /* Dielectric: 1 = .reflect_curve(Glass{}) (Schlick), 0 = none */
    rs_texture_desc texture;  /* albedo / light texture; Dielectric tint = texture.even */
    double  refractive;       /* Dielectric refractive index */
    double  exponent;         /* DiffuseMetal phong-lobe exponent; BlinnPhong exponent */
    double  multiplier;       /* DiffuseLight multiplier */
    int32_t mix_a, mix_b;     /* MixedMaterial: material ids (already created) */
    double  mix_p;            /* MixedMaterial probability of mix_a */
    double  phong_factor;     /* CommonMaterialSettings.phong_factor (0 = off) */
    int32_t phong_exponent;   /* CommonMaterialSettings.phong_exponent */
    int32_t _pad;
    double  k_specular;       /* BlinnPhong k_specular */
} rs_material_desc;

/* ---- Perlin noise texture data (src/texture/noise.rs) ----
 * The reference builds the tables from a FastRng seeded by the OS (noise.rs:44-66 via
 * FastRng::new()); here the caller passes the tables (include/raysnail.hpp builds them from a
 * seeded FastRng with rand 0.8's shuffle). */
#define RS_PERLIN_NORMAL     0  /* TextureType::Normal: noise(scale p), (n + 1) / 2 for vector values */
#define RS_PERLIN_TURBULENCE 1  /* TextureType::Turbulence(depth) */
#define RS_PERLIN_MARBLE     2  /* TextureType::Marble(depth): (sin(scale z + 10 turb) + 1) / 2 */
#define RS_SMOOTH_NONE       0
#define RS_SMOOTH_LINEAR     1
#define RS_SMOOTH_HERMITE    2
typedef struct rs_perlin_desc {
    uint32_t        point_count;  /* power of two (indices are masked with point_count - 1) */
    int32_t         vector;       /* 1: RandomValueType::Vector (values = 3 doubles each), 0: Float */
    int32_t         smooth;       /* RS_SMOOTH_* */
    int32_t         type;         /* RS_PERLIN_* */
    uint32_t        depth;        /* turbulence / marble depth */
    int32_t         _pad;
    double          scale;
    const double*   values;       /* point_count * (vector ? 3 : 1) */
    const uint32_t* perm_x;       /* point_count each, entries < point_count */
    const uint32_t* perm_y;
    const uint32_t* perm_z;
} rs_perlin_desc;

/* ---- geometry ---- */
#define RS_PLANE_XY 0   /* AARect::new_xy: axes (0,1), fixed 2 */
#define RS_PLANE_XZ 1   /* AARect::new_xz: axes (0,2), fixed 1 */
#define RS_PLANE_YZ 2   /* AARect::new_yz: axes (1,2), fixed 0 */

#define RS_TF_TRANSLATE 0 /* v = offset */
#define RS_TF_ROTATE_X  1 /* v[0] = angle in radians (Transform::rotate_by_x_axis) */
#define RS_TF_ROTATE_Y  2
#define RS_TF_ROTATE_Z  3
#define RS_TF_SCALE     4 /* v = factors */
typedef struct rs_transform {
    int32_t kind;
    int32_t _pad;
    double  v[3];
} rs_transform;

/* ---- camera (CameraBuilder, src/camera.rs:300-413) ---- */
typedef struct rs_camera_desc {
    double   look_from[3];
    double   look_at[3];
    double   vup[3];
    double   fov;        /* vertical field of view, degrees */
    double   aperture;
    double   focus;      /* focus distance */
    double   shutter;    /* shutter speed (ray time = shutter * gen()) */
    uint32_t width, height;
} rs_camera_desc;

/* ---- render settings (TakePhotoSettings src/camera.rs:104-154 + Painter src/painter.rs:69-130) ---- */
#define RS_MODE_AUTO      0
#define RS_MODE_MEGAKERNEL 1  /* one thread per path, all bounces in one launch */
#define RS_MODE_WAVEFRONT  2  /* extend / shade kernels over SoA path queues */
typedef struct rs_render_settings {
    uint32_t samples;    /* requested spp; N = floor(sqrt(samples))^2 is rendered (painter.rs:110-118) */
    uint32_t depth;      /* ray_color recursion depth (default 8, camera.rs:118) */
    int32_t  gamma;      /* 1 = sqrt gamma (into_color, vec3.rs:227-240) */
    int32_t  mode;       /* RS_MODE_* */
    uint64_t seed;       /* frame seed of the determinism contract */
    uint32_t pass;       /* progressive pass index (mixes into the stream key) */
    uint32_t row_begin;  /* rows [row_begin, row_end) with stride row_step are rendered */
    uint32_t row_end;    /* 0 = height */
    uint32_t row_step;   /* 0 or 1 = every row */
} rs_render_settings;

#define RS_KERNEL_NONE       0
#define RS_KERNEL_PATH_MEGA  1  /* k_path_mega: whole path per thread */
#define RS_KERNEL_WF_EXTEND  2  /* k_wf_extend: wavefront traversal (generic scenes) */
#define RS_KERNEL_WFS_EXTEND 3  /* k_wfs_extend: wavefront traversal + material classification */
#define RS_KERNEL_FEATURES   4  /* k_features: first-hit feature buffers (rs_render_features) */
#define RS_KERNEL_MATTES     5  /* k_mattes: ranked material-id mattes (rs_render_mattes) */
typedef struct rs_render_stats {
    uint64_t samples;    /* camera samples traced */
    uint64_t segments;   /* world.hit calls (path segments): the reference's count, so a frame that reports it traces
                          * every path as the reference does. A frame rendered without statistics may trace fewer
                          * segments (a streaming frame ends the paths whose throughput is exactly zero where the
                          * scene allows it, csrc/rs_dead_gate.h); its pixels are the same bit for bit. */
    double   ms;         /* wall time inside the call (device work + sync) */
    double   path_ms;    /* device time of all path-tracing launches (HIP events on the call's stream) */
    uint32_t launches;   /* number of path-tracing launches in the call */
    uint32_t kernel_launches; /* launches of the dominant kernel (megakernel or wavefront extend) */
    double   kernel_ms;  /* device time of those launches (HIP events bracketing each launch) */
    uint64_t kernel_bytes;    /* algorithmic HBM bytes those launches move */
    int32_t  kernel_id;       /* RS_KERNEL_* */
    int32_t  tree_arity;      /* BVH the traversal used: 4 = 4-wide, 2 = binary, 0 = empty world */
} rs_render_stats;

/* What rs_scene_commit built (diagnostic; no reference counterpart: BVH::new_internal,
 * bvh.rs:58-113, builds its own binary tree). */
typedef struct rs_scene_info {
    int32_t  tree_arity;      /* 4: 4-wide tree, near-first traversal; 2: binary tree; 0: empty world */
    int32_t  ref_order;       /* 1: the binary tree is walked in BVH::hit's recursion order (bvh.rs:173-192) */
    int32_t  scene_mode;      /* kernel specialisation: 0 generic, 1 spheres, 2 flat, 3 nest-0, 4 nest-2 */
    int32_t  tree_depth;      /* levels of the tree in use */
    int32_t  stack_need;      /* exact worst-case traversal stack entries of that tree */
    int32_t  stack_lds;       /* entries held in LDS; deeper ones spill to an HBM overflow array */
    uint64_t n_nodes;         /* nodes of the tree in use */
    uint64_t n_objects;       /* object handles (world objects, nested children, lights) */
    uint64_t n_world;         /* objects in the world list (BVH leaves) */
    int32_t  n_devices;       /* devices the scene is committed to */
    uint32_t class_mask;      /* wavefront shading classes some world object's hits fall into (bit k: 0 Lambertian,
                                 1 Metal, 2 DiffuseMetal, 3 Dielectric, 4 generic) */
} rs_scene_info;

typedef struct rs_scene rs_scene;

/* ---- library ---- */
int         rs_abi_version(void);
const char* rs_last_error(void);
int         rs_device_count(int* count);
uint64_t    rs_stream_key(uint64_t seed, uint32_t pass, uint64_t pixel, uint32_t sample);
/* ConstantMedium's Random::normal(): a uniform in [0, 1] from the XorShift128 state (x, y, z, w)
 * at the start of the segment and the medium's handle (see the determinism contract above) */
double      rs_medium_uniform(const uint32_t state[4], uint32_t handle);

/* ---- scene construction ---- */
int rs_scene_create(rs_scene** out);
int rs_scene_destroy(rs_scene* s);
/* texture data referenced by rs_texture_desc.data */
int rs_perlin(rs_scene* s, const rs_perlin_desc* desc, int32_t* id_out);
/* decoded 8-bit RGB pixels, row 0 = top (what DynamicImage::get_pixel indexes, image.rs:34-50) */
int rs_image(rs_scene* s, const uint8_t* rgb, uint32_t width, uint32_t height, int32_t* id_out);
int rs_material(rs_scene* s, const rs_material_desc* desc, int32_t* id_out);
int rs_sphere(rs_scene* s, const double center[3], double radius, const double speed[3] /* NULL = 0 */,
              int32_t material, uint32_t* handle_out);
int rs_aarect(rs_scene* s, int32_t plane, double k, double a0, double a1, double b0, double b1,
              int32_t material, uint32_t* handle_out);
int rs_box(rs_scene* s, const double p0[3], const double p1[3], int32_t material, uint32_t* handle_out);
int rs_quadric(rs_scene* s, const double q[10] /* qa qb qc qd qe qf qg qh qi qj */, int32_t material,
               uint32_t* handle_out);
/* RayMarcher::new(material): the Mandelbulb distance-estimator object about the origin (bbox +-1.3, 100 iterations,
   power 8: raymarching.rs has no parameters). Its hit() ignores the range end, so a world holding one is walked in
   the reference's BVH order; the object exists in the generic scene mode (rs_scene_info::scene_mode 0) only.
   An additive extension of ABI 6: no struct and no existing call changes, RS_ABI_VERSION stays 6. */
int rs_raymarcher(rs_scene* s, int32_t material, uint32_t* handle_out);
/* n triangles; pos = n*9 doubles (p0 p1 p2); nrm = n*9 doubles (n0 n1 n2) or NULL (zero normals,
 * Triangle::new default); handles are first_out .. first_out+n-1 */
int rs_triangles(rs_scene* s, const double* pos, const double* nrm, uint32_t n, int32_t material,
                 uint32_t* first_out);
int rs_intersection(rs_scene* s, uint32_t a, uint32_t b, int32_t material, uint32_t* handle_out);
int rs_difference(rs_scene* s, uint32_t plus, uint32_t minus, int32_t material, uint32_t* handle_out);
int rs_transformed(rs_scene* s, uint32_t object, const rs_transform* stack, uint32_t n, uint32_t* handle_out);
/* ConstantMedium::new(boundary, color, density): the medium's material is Isotropic(color) */
int rs_constant_medium(rs_scene* s, uint32_t boundary, const float color[4], double density, uint32_t* handle_out);
int rs_world_add(rs_scene* s, uint32_t handle);
int rs_lights_add(rs_scene* s, uint32_t handle);
int rs_set_background(rs_scene* s, const float lo[3], const float hi[3]);
/* World::new time_limit (world.rs:40-53): bounding boxes of moving spheres span [t0, t1];
 * the reference passes 0..camera.shutter_speed. Default [0, 0]. */
int rs_set_time_range(rs_scene* s, double t0, double t1);
/* freeze the scene: build the BVH and upload it to the current HIP device */
int rs_scene_commit(rs_scene* s);
/* freeze the scene for several devices (Painter::draw's thread fan-out, painter.rs:256-302 and the
 * thread count of :318-325, moved to GPUs): the scene is built once and replicated to each listed
 * HIP device ordinal. A device may be listed more than once (virtual devices with their own streams
 * and buffers). Every rs_render / rs_render_device call then splits its row lattice over the
 * devices the way render_rows interleaves rows over threads (device k of n takes lattice rows
 * k, k+n, ..., painter.rs:248) and runs them concurrently; because every sample owns its RNG
 * stream, the frame is bitwise independent of n. n = 0 is a host-only build: rs_scene_get_info
 * works, rendering returns RS_E_STATE. */
int rs_scene_commit_devices(rs_scene* s, const int* devices, int n);
int rs_scene_get_info(const rs_scene* s, rs_scene_info* out);
/* wavefront lanes for the scene's later renders (1 .. 4; 0 = the defaults): concurrent streams within
 * one frame. The bounce-synchronous wavefront (flat / mesh and rich scenes) deals the chunks of a
 * batch to them round robin (default 2); the streaming wavefront (spheres / box / CSG scenes) deals
 * whole sample batches to lanes, each with its own pool of paths (default 1). No reference
 * counterpart (a scheduling knob like Painter::threads, painter.rs:318-325); frames are bitwise the
 * same. */
int rs_scene_set_lanes(rs_scene* s, uint32_t lanes);
/* frames in flight per device (1 .. 4; default 3): consecutive asynchronous frames are dealt to this
 * many frame slots, each with its own streams and buffers, and a frame waits only for the previous
 * frame of its slot -- the next frame's first paths are traced while the previous frame's last paths
 * drain. Output and stream semantics are unchanged: a frame's result is written on the call's stream,
 * in call order; a frame with a mask (or statistics) also waits for the work queued on its stream
 * before the call. No reference counterpart (painter.rs renders one frame at a time). */
int rs_scene_set_frames_in_flight(rs_scene* s, uint32_t frames);
/* workspace sizes (0 = keep): camera samples per radiance batch buffer (default 32 Mi, whole sample
 * planes are used) and paths per path set (default 256 Mi: the bound of the streaming wavefront's pool
 * -- camera samples injected per iteration times the iterations a path can span; capped per device so
 * that the pools of its frame slots and lanes take at most two thirds of its memory, and, when a frame
 * slot allocates its pool, by the memory then free on the device (other allocations of the process
 * shrink the pool instead of failing the render; RS_E_NOMEM only when not even the floor fits: the
 * frame's pool or 64 Ki x max(depth, 1) paths, whichever is smaller, for the streaming wavefront, a
 * chunk of the frame's size or 1 Mi paths, whichever is smaller, for the bounce-synchronous one)
 * -- and the chunk of the bounce-synchronous wavefront). pool_paths is a soft bound: an iteration injects at least 256
 * samples (one block), so a pool below 256 x depth paths is raised to that for the frame.
 * Scheduling only: frames are bitwise the same for any value. */
int rs_scene_set_workspace(rs_scene* s, uint64_t max_batch_items, uint64_t pool_paths);

/* ---- render ---- */
/* host output: out_rgba = W*H*4 floats; mask = W*H bytes or NULL (all pixels) */
int rs_render(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st,
              const uint8_t* mask, float* out_rgba, rs_render_stats* stats);
/* host output with progressive row delivery -- Painter::draw's PainterTarget::register_pixels
 * (painter.rs:214) and its end-of-pass sentinel (painter.rs:332). The call's row lattice is rendered
 * in `bands` bands (0 = 16) of consecutive lattice rows, several in flight at once
 * (rs_scene_set_frames_in_flight per device, bands dealt to the devices round robin); as soon as a
 * band is complete, cb(user, y, row, W) is called for each of its rows y (row = out_rgba's row y,
 * already written), from the calling thread, in band order, while the later bands are traced; then
 * cb(user, H, NULL, 0). Rows off the lattice are neither written nor reported. The frame is bitwise
 * the rs_render frame. Stats carry the counts (samples, segments, kernel_bytes, tree_arity) and the call's
 * wall time `ms`; the bands stay in flight together, so no per-kernel device times are taken (0). */
typedef void (*rs_row_callback)(void* user, uint32_t y, const float* row_rgba, uint32_t width);
int rs_render_rows(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st, const uint8_t* mask,
                   float* out_rgba, uint32_t bands, rs_row_callback cb, void* user, rs_render_stats* stats);
/* device output: d_out_rgba device pointer (W*H*4 floats), d_mask device pointer or NULL,
 * stream = hipStream_t or NULL (default stream). With stats != NULL the call returns after the
 * work is enqueued AND complete (it synchronises its stream) so that stats are final, and times
 * the dominant kernel's launches; with stats == NULL it returns once the frame is enqueued
 * (asynchronous, no timing events): the frame is complete when `stream` reaches this point, and
 * the next call may be made at once (a call on another stream waits for this frame's buffers).
 * With several devices
 * (rs_scene_commit_devices) d_out_rgba, d_mask and stream belong to the FIRST listed device, which
 * renders its rows in place; the other devices render on their own streams and copy their rows
 * into d_out_rgba at frame end (peer access where the devices allow it). Stats are summed over
 * the devices (kernel_ms / path_ms are device time, ms is the call's wall time). */
int rs_render_device(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st,
                     const uint8_t* d_mask, float* d_out_rgba, void* stream, rs_render_stats* stats);
/* n_passes progressive passes of one frame into device frames: pass st->pass + k into d_outs[k] (k < n_passes;
 * the pointers may repeat: later passes overwrite), each frame bitwise the one rs_render_device renders for that
 * pass (no mask: the CLI's pass loop with its never-applied redo map, src/bin/raysnail.rs:379-427). On one device,
 * in the streaming scene modes (spheres, box / CSG: rs_scene_info.scene_mode 1, 3, 4), passes of at most 1 Mi
 * samples -- or 8 Mi at depth >= 16 -- run as sample streams, one per frame slot over a contiguous group of the
 * passes: pass k + 1's camera samples enter the path pool while pass k's paths drain, so the small late launches of
 * a pass carry the next one's work. A stream's path pool bounds the paths its passes can leave in flight: up to
 * depth x one pass's samples per slot, within the caps of rs_scene_set_workspace. Everything else renders the
 * passes one rs_render_device call after the other (larger passes fill the device alone; the stream measured 2-3 %
 * slower there). Stream and stats semantics as rs_render_device (stats summed over the passes). No reference
 * counterpart as one call: the reference renders its passes one after the other (raysnail.rs:379). */
int rs_render_device_passes(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st, uint32_t n_passes,
                            float* const* d_outs_rgba, void* stream, rs_render_stats* stats);

/* ---- first-hit feature buffers (guides for a denoiser, a compositor, edge-aware noise maps; no reference
 * counterpart) ----
 * Two RGBA f32 frames in the beauty frame's layout: out_albedo = [r, g, b, coverage], out_normal = [nx, ny, nz,
 * depth]. Either may be NULL (not written); both NULL is RS_E_INVALID. Sample s of pixel (x, y), pix = y W + x, with
 * sqrt_spp = floor(sqrt(samples)), N = sqrt_spp^2, si = s % sqrt_spp, sj = s / sqrt_spp:
 *   camera sample   the stratum centre, painter.rs:133-139 / :167-170 with both jitter draws 0.5, in f64:
 *                   xo = x + (si + 0.5) / sqrt_spp, yo = y + (sj + 0.5) / sqrt_spp, u = xo / W, v = (H - 1 - yo) / H
 *   ray             Camera::ray(u, v, rng) from the start of the stream seed_from_u64(rs_stream_key(seed, pass, pix,
 *                   s)): the lens disk and shutter time of the beauty frame's camera (depth of field and motion blur
 *                   stay; a pinhole camera's guides are noise-free)
 *   first hit       World::hit(ray, 0.0001, +inf) with medium key 0 (rs_probe_world_hit's convention): a
 *                   ConstantMedium stops a feature ray at the fixed key-0 distance
 *   on a hit        normal = HitRecord.normal, depth = t1 (ray directions are unit vectors), coverage = 1, albedo =
 *                   the f32 colour of the hit's material (the world's white Lambertian where the object has none),
 *                   widened to f64: Lambertian / Metal / DiffuseMetal / BlinnPhong texture.color(u, v, point);
 *                   Dielectric / Isotropic texture.even; DiffuseLight its texture's colour without the multiplier;
 *                   MixedMaterial its material_1's (as settings() chooses, mixed_material.rs:56-58; no RNG draw)
 *   on a miss       0 in all 8 channels (the background is not composited: coverage lets the caller do it)
 * Each channel of a pixel is the f64 sum over s = 0 .. N-1 in that order, starting from +0.0, divided by (double)N,
 * cast to f32: channels are premultiplied by coverage; no gamma. Masked pixels are [0,0,0,0] in both frames; rows
 * off the row lattice are not written. st->depth, gamma and mode are ignored (mode must still be a valid RS_MODE_*).
 * Validation as rs_render (RS_E_STATE before commit or on a host-only scene), before anything touches the device.
 * Several devices: the row lattice is split and gathered as rs_render's; frames are bitwise independent of it.
 * stats: samples, segments (world.hit calls: one per sample of an unmasked pixel), the kernel's launches and device
 * time, kernel_id RS_KERNEL_FEATURES. Additive extension of ABI 6. */
int rs_render_features(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st, const uint8_t* mask,
                       float* out_albedo, float* out_normal, rs_render_stats* stats);
/* the same into device frames; pointers, stream and stats semantics as rs_render_device (asynchronous when
 * stats == NULL) */
int rs_render_features_device(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st,
                              const uint8_t* d_mask, float* d_out_albedo, float* d_out_normal, void* stream,
                              rs_render_stats* stats);

/* ---- feature buffers through mirrors and glass: the end of each sample's specular chain ----
 * rs_render_features with one difference: what a sample contributes. Camera sample, ray, mask, row lattice, the f64
 * sum in sample order from +0.0 divided by (double)N and cast to f32, zero masked pixels, unwritten rows off the
 * lattice, the gathering of several devices, NULL outputs and validation are rs_render_features'. max_specular > 16 is
 * RS_E_INVALID (checked with the other arguments, before anything touches the device). A sample's chain, with
 * T = (1, 1, 1) in f64, depth unset, k = 0 and ray = the camera ray:
 *   loop            h = World::hit(ray, 0.0001, +inf) with medium key 0
 *   miss, k == 0    0 in all 8 channels (as rs_render_features)
 *   miss, k > 0     the chain escapes: albedo = T, coverage = 1, normal = the previous hit's, depth = the sum so far
 *   hit             depth = (k == 0) ? t1 : depth + t1 (directions are unit vectors: the path length). The hit's
 *                   material is resolved as rs_render_features' albedo resolves it (the world's default material
 *                   where the object has none; MixedMaterial -> material_1 up to 16 times, no RNG draw)
 *   specular hit    the resolved kind is RS_MAT_METAL or RS_MAT_DIELECTRIC and k < max_specular:
 *     Metal         c = the f32 texture.color(u, v, point); rf = d - n * (2.0 * dot(d, n)) (metal.rs:104-118). If
 *                   !(dot(rf, n) > 0.0) the hit is terminal (below). Else T = T * (double)c per channel and
 *                   ray = (p, rf, time)
 *     Dielectric    dielectric.rs:55-79 with reflect_prob taken as 0 (no draw; `glass` is ignored):
 *                   cos_theta = dot(-d, n); sin_theta = sqrt(1.0 - cos_theta * cos_theta); refr = outside ?
 *                   enter_refractive : outer_refractive. If refr * sin_theta > 1.0: nd = d - n * (2.0 * dot(d, n))
 *                   (total internal reflection). Else rp = (d + cos_theta * n) * refr; rq = (-sqrt(1.0 - dot(rp, rp)))
 *                   * n; nd = rp + rq. No fused multiply-add in any of it (the beauty path's arithmetic and order).
 *                   T = T * (double)texture.even per channel; ray = (p, nd, time). A NaN direction goes on into the
 *                   next World::hit as it does in the beauty path
 *                   then ++k and loop
 *   terminal hit    any other hit, a specular kind at k == max_specular included: albedo = T * (double)(the f32 albedo
 *                   rs_render_features gives this hit) per channel, coverage = 1, normal = this hit's, depth
 * At most max_specular + 1 World::hit calls per sample; stats->segments counts them. max_specular == 0 gives
 * rs_render_features' frames bit for bit (1.0 * x is exact) through the same kernel. kernel_id stays
 * RS_KERNEL_FEATURES. No Fresnel split: a dielectric's guide is what is seen through it. Additive extension of ABI 6. */
int rs_render_features_specular(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st,
                                const uint8_t* mask, uint32_t max_specular, float* out_albedo, float* out_normal,
                                rs_render_stats* stats);
/* the same into device frames; pointers, stream and stats semantics as rs_render_features_device */
int rs_render_features_specular_device(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st,
                                       const uint8_t* d_mask, uint32_t max_specular, float* d_out_albedo,
                                       float* d_out_normal, void* stream, rs_render_stats* stats);

/* ---- material-id mattes: per pixel the `ranks` most covering material ids and their coverage (the model of
 * Cryptomatte: Friedman, Jones 2015; no reference counterpart) ----
 * out_ids (int32) and out_cov (f32) are W*H*ranks elements each, rank-minor: pixel p = y W + x, rank r at p*ranks + r;
 * both must be non-NULL. out_overflow is W*H bytes and may be NULL (not written). Camera sample, ray, stream key,
 * mask, row lattice, N = floor(sqrt(samples))^2, validation (RS_E_STATE before commit or on a host-only scene) and the
 * split and gathering of several devices are rs_render_features' unchanged. RS_E_INVALID, checked with the other
 * arguments before anything touches the device: ranks outside 1 .. RS_MATTE_MAX_RANKS, max_specular > 16, a NULL
 * out_ids or out_cov.
 *   a sample's id   the chain of rs_render_features_specular with the same max_specular (0: the first hit), the same
 *                   rays and the same World::hit calls. A terminal hit gives its HitRecord's material as
 *                   rs_probe_world_hit reports it in field 12: the handle the object was created with, RS_NO_MATERIAL
 *                   where it has none. A MixedMaterial's own handle is the id (it is resolved only to decide whether
 *                   the hit is specular, as the chain does). A camera ray that misses and a chain that escapes after
 *                   a bounce both give RS_MATTE_ID_BACKGROUND. Every sample has exactly one id.
 *   counting        c(id) = the number of the pixel's N samples with that id. A pixel with more than
 *                   RS_MATTE_MAX_DISTINCT distinct ids keeps the RS_MATTE_MAX_DISTINCT smallest ids (signed compare),
 *                   each with its full count, and has overflow[p] = 1; otherwise overflow[p] = 0. Nothing depends on
 *                   the order of the samples.
 *   ranking         the kept ids sorted by c descending, on equal c by id ascending (signed). Rank r < ranks that
 *                   exists: ids = id, cov = (float)((double)c / (double)N). Ranks beyond the kept ids:
 *                   (RS_MATTE_ID_EMPTY, +0.0f).
 * Masked pixels and N == 0: every rank (RS_MATTE_ID_EMPTY, +0.0f), overflow 0. Rows off the row lattice are not written.
 * st->depth, gamma and mode are ignored (mode must still be a valid RS_MODE_*). stats: samples, segments (the
 * World::hit calls, as rs_render_features_specular counts them), the kernel's launches and device time, kernel_id
 * RS_KERNEL_MATTES. Additive extension of ABI 6. */
#define RS_MATTE_MAX_RANKS     8
#define RS_MATTE_MAX_DISTINCT  64
#define RS_MATTE_ID_BACKGROUND ((int32_t)-2)
#define RS_MATTE_ID_EMPTY      ((int32_t)0x80000000)
int rs_render_mattes(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st, const uint8_t* mask,
                     uint32_t ranks, uint32_t max_specular, int32_t* out_ids, float* out_cov, uint8_t* out_overflow,
                     rs_render_stats* stats);
/* the same into device arrays; pointers, stream and stats semantics as rs_render_features_device */
int rs_render_mattes_device(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st, const uint8_t* d_mask,
                            uint32_t ranks, uint32_t max_specular, int32_t* d_out_ids, float* d_out_cov,
                            uint8_t* d_out_overflow, void* stream, rs_render_stats* stats);

/* The matte of a set of ids from rs_render_mattes' layers. Scene-free, like rs_denoise. out is W*H f32:
 *   out[p] = the f32 sum, from +0.0f, in rank order r = 0 .. ranks-1, of cov[p*ranks + r] over the ranks whose id is
 *   one of wanted[0 .. n_wanted) and is not RS_MATTE_ID_EMPTY; each addition rounded once.
 * RS_E_INVALID before anything touches the device: a NULL pointer, ranks outside 1 .. RS_MATTE_MAX_RANKS, n_wanted
 * outside 1 .. 64, W H = 0 or > 0x7FFFFFFF. wanted is a HOST array in both forms (it travels in the kernel's argument
 * block, like rs_pass_moments_device's frame pointers).
 * rs_matte_extract_device: one launch on `stream` of the current device, never synchronises, allocates nothing; d_out
 * may not overlap the inputs. rs_matte_extract: host buffers; uploads, runs the device variant on the default stream,
 * synchronises, downloads. Additive extension of ABI 6. */
int rs_matte_extract_device(const int32_t* d_ids, const float* d_cov, uint32_t width, uint32_t height, uint32_t ranks,
                            const int32_t* wanted, uint32_t n_wanted, float* d_out, void* stream);
int rs_matte_extract(const int32_t* ids, const float* cov, uint32_t width, uint32_t height, uint32_t ranks,
                     const int32_t* wanted, uint32_t n_wanted, float* out);

/* ---- progressive passes (the CLI's pass loop, src/bin/raysnail.rs:311-427) ----
 * Device-resident frames (RGBA f32, W*H*4), all work on the caller's stream (NULL = default). */
typedef struct rs_noise_stats {
    float    min;        /* min over pixels of calc_noise, starting from 3.0 (raysnail.rs:396) */
    float    max;        /* max, starting from 1.0 (raysnail.rs:397) */
    uint64_t count;      /* pixels with noise >= threshold: the redo map's ones (raysnail.rs:411-422) */
} rs_noise_stats;

/* combine_pixels (raysnail.rs:176-208): acc[i] = new[i] == [0,0,0,0] ? acc[i]
 * : (acc[i] * pass + new[i]) / (pass + 1), per channel in f32. */
int rs_combine_pixels_device(float* d_acc_rgba, const float* d_new_rgba, uint64_t n_pixels, float pass, void* stream);

/* calc_noise (raysnail.rs:150-173) for every pixel -- including upstream's `let x = y` (the 5x5
 * window is centred on column y, the reference colour is pixel (x, y)) -- and the redo map
 * noise >= threshold (raysnail.rs:404-422; the CLI uses 0.01). d_redo may be NULL. Synchronises
 * the stream to return the stats. */
int rs_noise_map_device(const float* d_rgba, uint32_t width, uint32_t height, float threshold, uint8_t* d_redo,
                        void* stream, rs_noise_stats* stats);
/* the same on host buffers (uploaded, computed on the GPU, redo map copied back; redo may be NULL) */
int rs_noise_map(const float* rgba, uint32_t width, uint32_t height, float threshold, uint8_t* redo,
                 rs_noise_stats* stats);

/* ---- denoiser: a guided, edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010; no reference
 * counterpart) over a beauty frame and, optionally, the first-hit feature frames of rs_render_features ----
 * Scene-free, like rs_noise_map: frames are W*H RGBA f32. beauty = an rs_render frame (alpha 1, masked pixels
 * [0,0,0,0]); albedo = [r, g, b, coverage] or NULL (no demodulation); normal = [nx, ny, nz, depth] or NULL (no normal
 * and depth weights). Defaults (RS_DENOISE_*): levels 5, sigma_color 0.3, sigma_normal 0.25, sigma_depth 0.1.
 * RS_E_INVALID before anything touches the device: beauty, out (or d_work) NULL; levels outside 1 .. 8; a sigma that
 * is not finite or outside [1e-4, 1e4]; gamma not 0 or 1; W H = 0 or > 0x7FFFFFFF.
 *
 * Arithmetic: all f32, every operation below rounded once (IEEE division and square root, denormals kept, no
 * contraction), no transcendental function; a + b + c without brackets is never written. On the host, in f32:
 *   ic_i = 1 / ((sigma_color 2^-i) (sigma_color 2^-i))   for level i (the colour sigma halves per level)
 *   inv_n = 1 / (sigma_normal sigma_normal), inv_d = 1 / (sigma_depth sigma_depth)
 * Prepare, per pixel p (B = beauty[p], Al = albedo[p], g_p = normal[p] exactly as the frame holds it: premultiplied by
 * coverage, not renormalised):
 *   c = B.rgb; gamma == 1: c = c c per channel (undoes into_color's sqrt)
 *   albedo given: u = 1 - Al.w; a' = Al.rgb + u (the un-covered share counts as albedo 1: a sky pixel demodulates by
 *                 1); m = max(a', 1e-3) per channel; c = c / m
 *   usable(p) = B.a != 0 and B.rgb finite and (albedo given: Al's four channels finite) and (normal given: g_p's four
 *               channels finite) and c's three channels finite
 * Level i = 0 .. levels-1, step s = 2^i, from level i's colours c to level i+1's, for a usable p:
 *   taps q = p + s (dx, dy), dy = -2 .. 2 the outer loop, dx = -2 .. 2 the inner; a tap outside the frame or on a pixel
 *   that is not usable is skipped (it adds nothing, not even a zero); k = {1, 4, 6, 4, 1} / 16, h = k[dx] k[dy] (exact)
 *   the tap q = p has weight w = h(0, 0) exactly; every other tap, with D_ = the tap's value minus p's:
 *     dc2 = (D_r D_r + D_g D_g) + D_b D_b                  on level i's colours
 *     A = 1 + dc2 ic_i
 *     normal given:  dn2 = (D_x D_x + D_y D_y) + D_z D_z   on g.xyz;   dd = g_q.w - g_p.w
 *                    M = max(max(|g_p.w|, |g_q.w|), 1e-6); M2 = M M    (depth is compared relatively: feature depths
 *                    B = 1 + dn2 inv_n;  D = M2 + (dd dd) inv_d         are world distances)
 *                    w = h (M2 / ((A B) D))
 *     normal NULL:   w = h (1 / A)
 *   (rational -- Cauchy -- edge-stopping kernels on squared differences: one division per tap)
 *   S_c (three channels) and S_w start from +0.0 and add w c_q and w in tap order; the new colour is S_c / S_w
 *   a pixel that is not usable keeps its value through the levels
 * Finish: a usable p gets c m per channel (albedo given: the same m), then sqrt per channel if gamma == 1, and alpha
 * B.a; a pixel that is not usable gets the four channels of B bit for bit (a NaN pixel stays that NaN pixel and
 * reaches no neighbour; a masked pixel stays [0,0,0,0]).
 * Ranges: a usable pixel's |depth| must stay below 2^63 (M2 overflows beyond) and colours below about 1e18, or
 * infinities and NaNs appear in the sums as IEEE arithmetic gives them.
 *
 * rs_denoise_device: device pointers; enqueues one prepare launch and `levels` a-trous launches on `stream`
 * (hipStream_t, NULL = default) of the current device, never synchronises and allocates nothing. d_work is caller
 * memory of exactly 2 W H 4 floats (two colour planes; the guide is read in place). d_out may equal d_beauty (the
 * last level reads d_work and the guides, and B only at its own pixel); it must not overlap d_work or the guides.
 * rs_denoise: host buffers; uploads, runs the device variant on the default stream, synchronises, downloads (out may
 * equal beauty). Additive extension of ABI 6. */
#define RS_DENOISE_LEVELS       5
#define RS_DENOISE_SIGMA_COLOR  (0.3f)
#define RS_DENOISE_SIGMA_NORMAL (0.25f)
#define RS_DENOISE_SIGMA_DEPTH  (0.1f)
int rs_denoise_device(const float* d_beauty, const float* d_albedo, const float* d_normal,
                      uint32_t width, uint32_t height, uint32_t levels,
                      float sigma_color, float sigma_normal, float sigma_depth, int32_t gamma,
                      float* d_out, float* d_work, void* stream);
int rs_denoise(const float* beauty, const float* albedo, const float* normal,
               uint32_t width, uint32_t height, uint32_t levels,
               float sigma_color, float sigma_normal, float sigma_depth, int32_t gamma, float* out);

/* ---- pass moments: per-pixel mean, and variance of that mean, over K pass frames (no reference counterpart) ----
 * Scene-free. The K frames are independent renders of the same pixels (rs_render_device_passes' frames: W*H RGBA f32,
 * alpha 1, masked pixels [0,0,0,0]); their spread estimates the noise of their mean, which rs_denoise_var consumes.
 * RS_E_INVALID before anything touches the device: frames NULL or a NULL frame pointer; n_frames outside 1 .. 64;
 * gamma not 0 or 1; W H = 0 or > 0x7FFFFFFF; mean and var both NULL (either alone may be NULL: not written).
 *
 * Arithmetic: all f32, every operation rounded once (IEEE division and square root, denormals kept, no contraction),
 * no transcendental function. Per pixel p, with F_k = frame k's pixel p, k = 0 .. n_frames-1 in that order:
 *   frame k contributes when F_k.a != 0 and F_k.rgb are finite (rs_denoise's masked and NaN conventions)
 *   x_k = F_k.rgb; gamma == 1: x_k = x_k x_k per channel (undoes into_color's sqrt: moments of linear radiance)
 *   n = the number of contributing frames
 *   S = the sum of x_k over the contributing k in frame order, from +0.0;   mu = S / (float)n
 *   Q = the sum of (x_k - mu)(x_k - mu) over the contributing k in the same order, from +0.0 (the difference rounded,
 *       then its square, then the addition)
 *   v = Q / ((float)n (float)(n - 1)) for n >= 2 (the product of the two is exact), else +0.0
 *   mean[p] = [mu (gamma == 1: sqrt(mu) per channel), 1.0] for n >= 1, [0,0,0,0] for n = 0: a frame in rs_render's
 *             convention
 *   var[p]  = [v_r, v_g, v_b, (float)n]: linear radiance, the variance of the mean (not of one pass), never gamma
 * A contributing x_k x_k that overflows gives the infinities and NaNs IEEE arithmetic gives.
 *
 * rs_pass_moments_device: d_frames is a HOST array of n_frames device pointers; they travel in the kernel's argument
 * block (no device-side table, no copy). One launch on `stream` (hipStream_t, NULL = default) of the current device,
 * never synchronises, allocates nothing. A thread reads its pixel of every frame, twice, before it writes that pixel:
 * d_mean may alias any input frame. d_var must not overlap the frames or d_mean.
 * rs_pass_moments: host buffers; uploads, runs the device variant on the default stream, synchronises, downloads
 * (mean may be one of the frames). Additive extension of ABI 6. */
int rs_pass_moments_device(const float* const* d_frames, uint32_t n_frames, uint32_t width, uint32_t height,
                           int32_t gamma, float* d_mean, float* d_var, void* stream);
int rs_pass_moments(const float* const* frames, uint32_t n_frames, uint32_t width, uint32_t height,
                    int32_t gamma, float* mean, float* var);

/* ---- robust pass combine: per-pixel rank-trimmed mean of K pass frames, and the Winsorised variance of that mean
 * (median of means, Jung et al. 2015; the trim from the Gini coefficient, Buisine et al. 2021; the variance of a
 * trimmed mean, Tukey & McLaughlin 1963; no reference counterpart) ----
 * rs_pass_moments with the t lowest and the t highest frames of each pixel cut: a firefly (one pass frame that caught
 * a caustic path into a small light) no longer reaches the mean, nor blows up the variance rs_denoise_var divides by.
 * Frames, outputs and conventions are rs_pass_moments'; the two output frames are consumed by rs_denoise_var unchanged.
 * RS_E_INVALID before anything touches the device: everything rs_pass_moments refuses (mean and var both NULL too;
 * trimmed may be NULL: not written); a trim that is neither RS_ROBUST_TRIM_AUTO nor finite in [0, 0.5].
 *
 * Arithmetic: rs_pass_moments' rules (all f32, every operation rounded once, IEEE division and square root, no
 * contraction, no transcendental function). Per pixel p, with F_k = frame k's pixel p, k = 0 .. n_frames-1:
 *   x_k = F_k.rgb; gamma == 1: x_k = x_k x_k per channel.   Key: s_k = (x_k.r + x_k.g) + x_k.b
 *   frame k contributes when F_k.a != 0, F_k.rgb are finite and s_k is finite (a square that overflows drops the
 *   frame: the one difference from rs_pass_moments);   n = the number of contributing frames
 *   order: frame j is before frame k when s_j < s_k, or s_j == s_k and j < k (a total order; -0.0 == +0.0);
 *   r_k = the number of contributing j before k
 *   t_max = (n - 2) / 2 (integer division) for n >= 2, else 0: two frames always survive, the variance stays defined
 *   trim given:  t = min(t_max, (uint32)floorf(trim (float)n))
 *   trim == RS_ROBUST_TRIM_AUTO: the Gini coefficient of the keys decides.
 *     S_s = the sum of s_k over the contributing k in frame order, from +0.0
 *     N_g = the sum of (float)(2 r_k - (n - 1)) s_k in the same order, from +0.0 (the integer is exact; the product
 *           rounded, then the addition)
 *     G = S_s > 0 ? N_g / ((float)n S_s) : 0, then fminf(fmaxf(G, 0), 1) (a NaN becomes 0)
 *     t = min(t_max, (uint32)floorf((G (float)n) 0.5f))
 *   h = n - 2 t; frame k is kept when t <= r_k <= n - 1 - t; lo, hi = the frames of rank t and n - 1 - t
 *   S = the sum of x_k over the kept k in frame order, per channel, from +0.0;   mu = S / (float)h
 *   w_k = x_lo for r_k < t, x_hi for r_k > n - 1 - t (the whole rgb triple of that frame: the colour stays one some
 *         pass rendered), else x_k
 *   mw = (the sum of w_k over the contributing k in frame order, from +0.0) / (float)n
 *   Q = the sum of (w_k - mw)(w_k - mw) in frame order, from +0.0 (the difference rounded, then its square, then the
 *       addition);   v = Q / ((float)h (float)(h - 1)) for n >= 2, else +0.0
 *   mean[p] = rs_pass_moments' mean[p] with this mu;   var[p] = [v_r, v_g, v_b, (float)n];
 *   trimmed[p] = (uint8)t (0 for n = 0)
 * At t = 0 every operation is rs_pass_moments', in its order: trim = 0 gives rs_pass_moments' two frames bit for bit
 * on every pixel none of whose squares overflow.
 *
 * rs_pass_robust_device: rs_pass_moments_device's rules (d_frames a HOST array of device pointers that travel in the
 * argument block; one launch on `stream`, never synchronises, allocates nothing). Every load of a thread comes before
 * its stores: d_mean may alias a frame. d_var and d_trimmed (W H bytes) overlap nothing.
 * rs_pass_robust: host buffers; uploads, runs the device variant on the default stream, synchronises, downloads (mean
 * may be one of the frames). Additive extension of ABI 6. */
#define RS_ROBUST_TRIM_AUTO ((float)-1.0)
int rs_pass_robust_device(const float* const* d_frames, uint32_t n_frames, uint32_t width, uint32_t height,
                          int32_t gamma, float trim, float* d_mean, float* d_var, uint8_t* d_trimmed, void* stream);
int rs_pass_robust(const float* const* frames, uint32_t n_frames, uint32_t width, uint32_t height,
                   int32_t gamma, float trim, float* mean, float* var, uint8_t* trimmed);

/* ---- variance-guided denoiser: rs_denoise's a-trous filter with the colour edge-stopping weight normalised by a
 * per-pixel variance that is itself filtered level by level (Schied et al. 2017, SVGF's spatial filter without its
 * temporal half; no reference counterpart) ----
 * Frames as rs_denoise's, plus var = rs_pass_moments' variance frame [var_r, var_g, var_b, n] of the beauty frame
 * (linear radiance). Everything not restated here is rs_denoise's contract unchanged: the arithmetic rules, the tap
 * order (dy outer, dx inner), k and h, dn2, dd, M, M2, B, D, skipped taps, the finish of the colour, the pass-through
 * of pixels that are not usable, the ranges. k_color (RS_DENOISE_VAR_K_COLOR) replaces sigma_color and takes a sigma's
 * range. Defaults (RS_DENOISE_VAR_*): levels 5, k_color 2.5; sigma_normal and sigma_depth default to RS_DENOISE_SIGMA_*.
 * RS_E_INVALID before anything touches the device: beauty, var, out (or d_work) NULL; levels outside 1 .. 8; k_color
 * or a sigma not finite or outside [1e-4, 1e4]; gamma not 0 or 1; W H = 0 or > 0x7FFFFFFF.
 *
 * On the host, in f32: inv_n, inv_d as rs_denoise's. The colour constant does not halve per level: the variance shrinks.
 * Prepare, per pixel p (V = var[p]): c, m as rs_denoise's, and
 *   mm = m m per channel (albedo given; rounded once); v = V.rgb / mm (albedo given), v = V.rgb (albedo NULL)
 *   usable(p) = rs_denoise's usable(p) and V.rgb finite and >= 0 (-0.0 passes) and v's three channels finite
 *   (V.w is not read before the finish)
 * Level i = 0 .. levels-1, step s = 2^i, from level i's (c, v) to level i+1's, for a usable p:
 *   t_q = (v_q.r + v_q.g) + v_q.b of level i's variances
 *   vs_p: the 3 x 3 Gaussian-weighted mean of t around p at pixel spacing 1 (at every level): taps q = p + (dx, dy),
 *         dy = -1 .. 1 the outer loop, dx = -1 .. 1 the inner, the centre in its place in that order; g = {1, 2, 1} / 4,
 *         weight g[dx] g[dy] (exact); a tap outside the frame or on a pixel that is not usable is skipped;
 *         N = the sum of (g[dx] g[dy]) t_q and G = the sum of g[dx] g[dy], both from +0.0 (product, then addition);
 *         vs_p = N / G
 *   iv = 1 / (k_color vs_p + RS_DENOISE_VAR_EPS)   (one division per pixel and level; EPS = 1e-6f keeps a
 *        variance-free neighbourhood finite: there the filter degenerates to rs_denoise's with sigma_color 1e-3)
 *   the 5 x 5 taps q = p + s (dx, dy) as rs_denoise's, with A = 1 + dc2 iv for every tap but the centre; B, D, M2, w as
 *   there (normal NULL: w = h (1 / A)); the centre has w = h(0, 0)
 *   S_c, S_w as rs_denoise's; S_v (three channels, from +0.0) adds ww v_q per channel in tap order, ww = w w
 *   rounded once (the centre adds (h(0,0) h(0,0)) v_p)
 *   new colour S_c / S_w; SS = S_w S_w (rounded once); new variance S_v / SS per channel
 *   a pixel that is not usable takes no part and its plane values are never read
 * Finish (with the last level): the colour as rs_denoise's. out_var[p], when given, = [v mm per channel (albedo
 * given; the same mm) or v (albedo NULL), V.w] for a usable p, and V's four channels bit for bit otherwise.
 *
 * rs_denoise_var_device: device pointers; one prepare launch and `levels` a-trous launches on `stream` of the current
 * device, never synchronises, allocates nothing. d_work is caller memory of exactly 4 W H 4 floats (two colour and two
 * variance planes that ping-pong; the guide is read in place). d_out may equal d_beauty and d_out_var may equal d_var
 * (the last level reads B and V only at its own pixel); neither may overlap d_work, the guides, or the other's input.
 * d_out_var may be NULL.
 * rs_denoise_var: host buffers (out may equal beauty, out_var may equal var or be NULL); uploads, runs the device
 * variant on the default stream, synchronises, downloads. Additive extension of ABI 6. */
#define RS_DENOISE_VAR_LEVELS   ((uint32_t)5)
#define RS_DENOISE_VAR_K_COLOR  ((float)2.5)
#define RS_DENOISE_VAR_EPS      ((float)1e-6)
int rs_denoise_var_device(const float* d_beauty, const float* d_var, const float* d_albedo, const float* d_normal,
                          uint32_t width, uint32_t height, uint32_t levels,
                          float k_color, float sigma_normal, float sigma_depth, int32_t gamma,
                          float* d_out, float* d_out_var, float* d_work, void* stream);
int rs_denoise_var(const float* beauty, const float* var, const float* albedo, const float* normal,
                   uint32_t width, uint32_t height, uint32_t levels,
                   float k_color, float sigma_normal, float sigma_depth, int32_t gamma,
                   float* out, float* out_var);

/* ---- ray queries: World::hit for the caller's own rays, as the closest hit's record or as an occlusion byte ----
 * rays: n * 8 doubles, 64 bytes per ray = [origin.xyz, direction.xyz, time, tmax]. Ray i's results go to index i of
 * every output: nothing is reordered or compacted. Directions need not be unit vectors (t is in units of the
 * direction's length). The medium key of every ray is 0 (rs_probe_world_hit's convention). tmin is one value per call.
 *
 * Each ray computes World::hit(ray, tmin..tmax) (world.rs:63-65 -> BVH::hit, bvh.rs:173-192) with its own tmax as the
 * INITIAL end of the range: the walk starts from it and every box and object test sees it, so an object whose nearest
 * root lies beyond tmax can still answer with another one inside the range (a sphere seen from inside, a Box, a
 * Quadric, a CSG operand). It is not a filter on the result of a walk to +inf. Which end of the range is open is each
 * object's own rule in the reference: spheres, rects, boxes and quadrics take tmin <= t < tmax, a triangle closes its
 * range at tmax. No value gets a special case: a NaN tmax, a negative one and tmax < tmin do what the reference's
 * range tests do with them (the box tests' min / max ignore a NaN end; each object's own comparisons then decide).
 *
 * Closest hit. d_ids (required): n * 4 int32 = [hit (0 / 1), outside (0 / 1), material id as rs_probe_world_hit
 * reports it in field 12 (RS_NO_MATERIAL: none), object]. d_geom (may be NULL): n * 8 doubles = [t1, t2, p.xyz, n.xyz].
 * d_uv (may be NULL): n * 2 doubles = (u, v), computed only in scenes that read them (an Image texture) and +0.0 in all
 * others, as rs_probe_world_hit's fields 9 and 10. A miss writes ids = [0, 0, RS_TRACE_NONE, RS_TRACE_NONE], geom =
 * [+inf, +0.0 x 7], uv = [+0.0, +0.0].
 *   object   the handle of the world object whose record this is: the value rs_sphere .. rs_transformed returned for
 *            the object given to rs_world_add, and first + i for triangle i of an rs_triangles call. A nested object (a
 *            CSG operand, the child of a transform or of a medium) is never reported: its parent is. The same in every
 *            scene mode (the numbering of rs_probe_tree's lprim and pbox).
 *   ties     where several objects are hit at the same t1: in scenes whose tree is walked in the reference's order
 *            (rs_scene_info / rs_probe_tree ref_order = 1) the reference's winner; otherwise one of the tied objects
 *            (near-first walk), hit flag and t1 being the reference's in either case.
 * Occlusion. d_occluded: n bytes, 1 iff that World::hit is Some, else 0: the closest form's hit flag, for every ray.
 * The walk of an occlusion ray ends at its first accepted object. (Some object is accepted under its turn's range iff
 * one is accepted under the full range -- until the first acceptance the turn's range is the full one -- so the flag
 * does not depend on the visiting order.)
 *
 * Errors, all before anything touches the device. RS_E_INVALID: a NULL d_ids / d_occluded; a NULL d_rays with n > 0;
 * d_rays or d_geom not 16-byte aligned; replica neither 0 nor below the number of committed devices. Then RS_E_STATE:
 * before commit, or on a host-only commit (no device). n == 0 is RS_OK and launches nothing. Outputs must not overlap
 * the rays or each other.
 *
 * The _device forms take device pointers on the device of entry `replica` of the committed device list (the caller
 * picks one: a batch is not split), enqueue ONE launch on `stream` (hipStream_t, NULL = default) and return without
 * synchronising. They allocate nothing per call, the traversal stack's overflow array aside, which is sized once per
 * replica for the frame launches' grid (scenes whose tree fits the on-chip stack have none). The launch is a
 * grid-stride loop of min(ceil(n / 256), 8 * the device's compute units) blocks of 256 threads, one ray per thread per
 * trip: what a call needs beyond its arguments is bounded by the device, not by n. A ray is read with four 16-byte
 * loads, a geom row written with four 16-byte stores and an ids row with one.
 * rs_trace_closest / rs_trace_occluded: host arrays (no alignment asked); stage through one device allocation on
 * replica 0, run the device form on the default stream, synchronise, copy back.
 * No reference counterpart as an entry (the oracle's is orc_world_hit). Additive extension of ABI 6. */
#define RS_TRACE_NONE ((int32_t)0x80000000)   /* INT32_MIN: material / object of a ray that hit nothing */
int rs_trace_closest_device(rs_scene* s, uint32_t replica, const double* d_rays, uint32_t n, double tmin,
                            int32_t* d_ids, double* d_geom, double* d_uv, void* stream);
int rs_trace_occluded_device(rs_scene* s, uint32_t replica, const double* d_rays, uint32_t n, double tmin,
                             uint8_t* d_occluded, void* stream);
int rs_trace_closest(rs_scene* s, const double* rays, uint32_t n, double tmin, int32_t* ids, double* geom, double* uv);
int rs_trace_occluded(rs_scene* s, const double* rays, uint32_t n, double tmin, uint8_t* occluded);

/* ---- diagnostics (parity probes used by tests/) ---- */
/* World::hit (world.rs:63-65) for n rays on the device. rays: n*7 doubles (origin, direction,
 * time); out: n*13 doubles = [hit, t1, t2, p.xyz, n.xyz, u, v, outside, material id] (u, v are
 * computed only in scenes with an Image texture, the only reader: 0 otherwise). The medium key of
 * the probe rays is 0. tmax must be +inf or the hit is dropped when t1 >= tmax. */
int rs_probe_world_hit(rs_scene* s, const double* rays, uint32_t n, double tmin, double tmax, double* out);

/* Radiance of samples s0 .. s0+n-1 of pixel (x, y) -- one ray_color (camera.rs:156-255) each, the
 * camera sample and RNG stream exactly as rs_render draws them (st: samples, depth, seed, pass).
 * out: n*4 doubles = [r, g, b, world.hit count], before the /N and gamma of into_color. Diagnostic
 * (per-sample parity against the oracle); no reference counterpart. */
int rs_probe_samples(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st, uint32_t x, uint32_t y,
                     uint32_t s0, uint32_t n, double* out);

/* One level of ray_color (camera.rs:156-255) after world.hit, on n synthetic hit records, through the scene
 * mode's own shading code. rows: n*18 doubles = [ray o.xyz, d.xyz, time, hit p.xyz, n.xyz, t1, outside, u, v,
 * material id as rs_probe_world_hit reports it (-1: the world's default material)]. Row i draws from the stream
 * seed_from_u64(rs_stream_key(seed, 0, i, 0)) and starts from throughput T = (1, 1, 1), radiance L = 0.
 * out: n*18 doubles = [continues, L.xyz (the level's emission), T.xyz (the level's factor; (1, 1, 1) when the
 * path ends), the next ray's o.xyz, d.xyz, time (the row's own ray when the path ends), the four RNG state words
 * after the level]. The scene needs a lights list (RS_E_NO_LIGHTS); an id outside the scene's materials is
 * RS_E_INVALID. Diagnostic (shading parity against the oracle on exact inputs); additive extension of ABI 6. */
int rs_probe_shade(rs_scene* s, const double* rows, uint32_t n, uint64_t seed, double* out);

/* The camera sample alone (painter.rs:133-139, :167-170 and camera.rs:37-85), through the scene mode's own compile
 * of the code every render kernel calls. xys: n triples of uint32 = [pixel x, pixel y, sample index below
 * floor(sqrt(st->samples))^2]; st gives samples, seed and pass. centres == 0: the jittered sample rs_render draws;
 * otherwise the stratum centre rs_render_features[_specular] uses (no jitter draw: the ray is drawn from the start
 * of the sample's stream). out: n*11 doubles = [origin.xyz, direction.xyz, time, the four RNG state words after the
 * sample]. Any camera rs_render accepts is accepted; a pixel outside the frame or a sample index beyond the
 * stratum grid is RS_E_INVALID. Diagnostic (camera parity against the oracle on degenerate cameras); additive
 * extension of ABI 6. */
int rs_probe_camera(rs_scene* s, const rs_camera_desc* cam, const rs_render_settings* st, const uint32_t* xys, uint32_t n,
                    int32_t centres, double* out);

/* The tree rs_scene_commit staged for upload, copied out of the staged arrays themselves (what every replica
 * receives; nothing is rebuilt), on host-only commits too. head: 8 int32 = [arity of the tree the walks use (4: the
 * 4-wide nodes, 2: the binary nodes, 0: an empty world), its root code (a node index; ~leaf for a single object; the
 * binary tree's root when the arity is 2), ref_order, ltop (spheres mode: the first ltop nodes are the breadth-first
 * top the extend holds in LDS), n_nodes, n_lprim (leaf entries; 0: a leaf code ~h names prim handle h itself),
 * n_pbox (prim handles, nested children included), stack_need]. Each of the other arrays may be null (skipped):
 * planes: n_nodes * arity * 6 floats = per node and child slot [lo.xyz, hi.xyz] (an empty slot: +inf, -inf);
 * child: n_nodes * arity child codes (>= 0 a node, < 0 a leaf code ~e, INT32_MIN an empty slot); lprim: n_lprim prim
 * handles (leaf entry -> handle); pbox: n_pbox * 6 doubles = per prim handle the exact [lo.xyz, hi.xyz] the leaf
 * test applies. Call it once with the arrays null for the sizes. Diagnostic (the tree's invariants checked on the
 * CPU: tests/test_tree_invariants.py); additive extension of ABI 6. */
int rs_probe_tree(const rs_scene* s, int32_t* head, float* planes, int32_t* child, int32_t* lprim, double* pbox);

#ifdef __cplusplus
}
#endif

/* adaptive sampling (rs_moments_update_device, rs_moments_resolve_device, rs_adaptive_mask_device,
 * rs_render_adaptive[_device]): additive extensions of ABI 6, declared in a header of their own */
#include "raysnail_adaptive.h"

#endif /* RAYSNAIL_HIP_H */
