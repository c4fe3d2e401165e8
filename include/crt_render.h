/*
 * crt_render.h — C ABI of the MI355X (gfx950) render path.
 *
 * This is the drop-in boundary for the reference's hot path
 *   Camera::render(const Scene&)            include/base/camera.h:301-303
 *   template<T> Camera::render(const T&)    include/base/camera.h:264-297
 *   BVH(world, 32, 12) build + BVH::hit_by  include/acceleration/bvh.h:183-550, 585-715
 * (paths relative to the reference repository DeltaPavonis/cpp_raytracer).
 *
 * Plain C types only: pointers, sizes, POD structs. No HIP or torch types in any signature;
 * streams are passed as `void*` (a hipStream_t, or NULL for the default stream).
 * Every function returns 0 on success and a negative CRT_E* code on failure; the message of the
 * last failure on the calling thread is available from crt_last_error().
 *
 * The C++ reference-compatible API (cpp_raytracer_amd/include/base/camera.h etc.) is built on
 * top of these entry points; INTEGRATION.md shows the bindings.
 */
#ifndef CRT_RENDER_H
#define CRT_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI versions:
 *   1  rounds 1-4.
 *   2  round 5: crt_scene_image added; crt_bvh_params.build_device = d + 1 now also sets the scene
 *      up on GPU d (its copy there lives as long as the scene; other devices peer-copy it, guard
 *      words zeroed) and leaves the host-side staging image empty. */
#define CRT_ABI_VERSION 2

/* ---- status codes ---------------------------------------------------------------------- */
#define CRT_OK 0
#define CRT_E_INVALID (-1)     /* bad argument / unsupported object                         */
#define CRT_E_HIP (-2)         /* a HIP runtime call failed (message names it)              */
#define CRT_E_NODEVICE (-3)    /* no gfx950 device visible, or device index out of range    */
#define CRT_E_NOT_UPLOADED (-4)/* scene not resident on the requested device               */
#define CRT_E_ALLOC (-5)       /* host or device allocation failed                          */

/* ---- scene description ----------------------------------------------------------------- */
/* Material kinds: base/material.h:58 (Lambertian), :105 (Metal), :164 (Dielectric),
 * :231 (DiffuseLight). */
enum {
    CRT_LAMBERTIAN = 1,    /* color = intrinsic colour                                       */
    CRT_METAL = 2,         /* color, param = fuzz AFTER the ctor's fmin(fuzz, 1) clamp (:150) */
    CRT_DIELECTRIC = 3,    /* param = refractive index                                       */
    CRT_DIFFUSE_LIGHT = 4  /* color, param = intensity                                       */
};

/* Object kinds: shapes/sphere.h:12, shapes/parallelogram.h:133, shapes/box.h:432. */
enum {
    CRT_SPHERE = 1,        /* v[0..2] centre, v[3] radius                                    */
    CRT_PARALLELOGRAM = 2, /* v[0..2] vertex, v[3..5] side1, v[6..8] side2                  */
    CRT_BOX = 3            /* v[0..2] vertex, v[3..5] opposite vertex (6 faces, box.h:53-84) */
};

typedef struct crt_material {
    uint32_t kind;
    uint32_t reserved;
    double color[3];
    double param;
} crt_material; /* 40 bytes */

typedef struct crt_object {
    uint32_t kind;
    uint32_t material; /* index into the material array */
    double v[9];
} crt_object; /* 80 bytes */

/* BVH build knobs, BVH(world, num_buckets = 32, max_primitives_in_node = 12) bvh.h:754-756.
 * linear != 0 builds a single always-entered leaf in object order: the semantics of rendering a
 * non-BVH Hittable (Scene::hit_by scene.h:59-75 / Box::hit_by box.h:24-28). */
typedef struct crt_bvh_params {
    uint32_t num_buckets;
    uint32_t max_prims_in_node;
    uint32_t linear;
    uint32_t build_device;  /* 0: build on the host; d + 1: build on GPU d (the same tree), and
                             * set the scene up on GPU d: its copy there is in place after
                             * crt_scene_create (the same bytes the host staging uploads) */
} crt_bvh_params;

/* ---- camera ---------------------------------------------------------------------------- */
/* The Camera's user-set state (camera.h:16-82 members, set by the setters at :308-406).
 * Angles are RADIANS, exactly as the Camera stores them after its degree conversions. */
typedef struct crt_camera_settings {
    uint32_t image_w, image_h;
    uint32_t samples_per_pixel, max_depth;
    double center[3];
    double direction[3];
    double lookat[3];
    double up[3];
    double focus_dist;
    double fov;            /* vertical if fov_is_vertical, else horizontal; radians          */
    double defocus_angle;  /* radians                                                        */
    double background[3];
    uint32_t has_lookat;
    uint32_t has_focus_dist;
    uint32_t fov_is_vertical;
    uint32_t reserved;
} crt_camera_settings;

/* The camera after Camera::init() (camera.h:87-157): what the per-sample loop reads. */
typedef struct crt_camera {
    uint32_t image_w, image_h;
    uint32_t samples_per_pixel, max_depth;
    double origin[3];
    double pixel00[3];
    double pixel_delta_x[3];
    double pixel_delta_y[3];
    double defocus_disk_x[3];
    double defocus_disk_y[3];
    double defocus_angle;
    double background[3];
    double t_min;          /* Interval::with_min(0.00001), camera.h:217                      */
    uint32_t base_seed;    /* per-render seed of the per-sample RNG stream (crt_sample_seed)  */
    uint32_t reserved;
} crt_camera;

/* Rows owned by one device/rank: row r is rendered iff (r / row_block) % tile_count == tile_index.
 * {1,1,0,0} (or NULL) = the whole frame. flags: CRT_TILING_PACKED = the output buffer holds only
 * the owned rows, packed in order (owned row k at offset k * image_w * 3): a rank or device then
 * allocates its share of the frame, not the whole frame.
 * ABI change (round 4): this word was `reserved` before CRT_TILING_PACKED existed; any other bit
 * set is rejected with CRT_E_INVALID, so a caller that left it uninitialised must now zero it. */
#define CRT_TILING_PACKED 1u
typedef struct crt_tiling {
    uint32_t row_block;
    uint32_t tile_count;
    uint32_t tile_index;
    uint32_t flags;
} crt_tiling;

typedef struct crt_scene crt_scene; /* opaque: flattened primitives + BVH + device copies */

typedef struct crt_scene_info {
    uint64_t num_objects, num_materials, num_primitives, num_spheres, num_parallelograms;
    uint64_t num_nodes;
    uint32_t depth;          /* levels in the BVH (root = 1)                                 */
    uint32_t max_leaf_size;
    uint64_t device_bytes;   /* bytes of one device copy                                     */
    double build_ms;         /* host BVH build time                                          */
} crt_scene_info;

/* A LinearBVHNode (bvh.h:117-161) as exported for parity checks. */
typedef struct crt_bvh_node {
    double bounds[6];        /* x.min x.max y.min y.max z.min z.max                          */
    uint32_t index;          /* first primitive (leaf) / second child (interior)             */
    uint32_t count;          /* primitives in leaf, 0 for interior                           */
    uint32_t axis;           /* split axis of an interior node                               */
    uint32_t flags;          /* bit0: always entered (linear leaf)                           */
} crt_bvh_node;

/* Closest hit of one ray (the hit_info of hittable.h:20-72 that BVH::hit_by returns). */
typedef struct crt_hit {
    double t;
    double point[3];
    double normal[3];        /* faces the ray (front-face flip applied)                      */
    int32_t prim;            /* flattened primitive index (Scene::get_primitive_components), -1 = miss */
    int32_t front_face;      /* hit_from_outside                                             */
    uint32_t material;
    uint32_t reserved;
} crt_hit;

/* Work counters of one render (instrumented pass): the algorithmic-byte basis of bench.py. */
typedef struct crt_render_stats {
    uint64_t samples;
    uint64_t rays;           /* ray segments traced (primary + scattered)                    */
    uint64_t nodes_visited;  /* BVH nodes whose AABB was tested                              */
    uint64_t sphere_tests;
    uint64_t parallelogram_tests;
    double kernel_ms;
    /* wave-time breakdown of the instrumented pass (sum over waves, 100 MHz ticks): interior
     * BVH walk, leaf primitive tests, shading + path regeneration, whole wave lifetime */
    uint64_t ticks_walk, ticks_leaf, ticks_shade, ticks_total;
    /* wave iterations of each phase: lane utilization = lane work / (iterations * 64) with lane
     * work = nodes_visited, sphere+parallelogram tests, rays respectively */
    uint64_t wave_iters_walk, wave_iters_leaf, wave_iters_shade;
    uint64_t ticks_tail;  /* summed per wave: ticks from its first idle lane to its end */
    /* node tests the f32 walk could not decide (decided in f64), and the wave iterations that
     * ran such a test */
    uint64_t slow_node_tests, wave_iters_slow;
    /* two-pass sphere leaves: exact tests of the filter's candidates, and the wave iterations
     * of that pass (sphere_tests counts the filter's tests) */
    uint64_t candidate_tests, wave_iters_candidates;
} crt_render_stats;

/* ---- entry points ---------------------------------------------------------------------- */
int crt_abi_version(void);
const char* crt_last_error(void);
/* The library's compile-time configuration ("arch=gfx950 CRT_BLOCK=256 ..."): the kernel build
 * switches documented in INTEGRATION.md. */
const char* crt_build_info(void);
int crt_device_count(int* count);
void crt_free(void* p);

/* Per-sample RNG seed: state X0 of the reference's LCG (rand_util.h:85-117) for one (pixel,
 * sample); the kernel then draws X1, X2, ... exactly as rand_double does. */
uint32_t crt_sample_seed(uint32_t base_seed, uint32_t pixel, uint32_t sample);

/* One reference-LCG draw: advances *state and returns min + (max-min)*X*(1/(2^32-2)). */
double crt_rand_double(uint32_t* state, double min, double max);

/* Scenes of the reference's src/main.cpp, built with the reference's RNG semantics
 * (SeedSeqGenerator + LCG, evaluation order of a g++ build). has_seed = 0 keeps the scene
 * function's own seeding (rtow_final_image never seeds; such a call is rejected).
 * Arrays are malloc'd; release with crt_free. cam receives the scene's camera settings. */
int crt_scene_build_named(const char* name, uint32_t seed, int has_seed,
                          crt_material** materials, size_t* num_materials,
                          crt_object** objects, size_t* num_objects,
                          crt_camera_settings* cam);

/* Flatten (Scene::get_primitive_components, scene.h:85-106) and build the BVH (bvh.h:183-550)
 * on the host, or with params->build_device on that GPU, where the whole scene is then set up.
 * params may be NULL (= {32, 12, 0, 0}). */
int crt_scene_create(const crt_material* materials, size_t num_materials,
                     const crt_object* objects, size_t num_objects,
                     const crt_bvh_params* params, crt_scene** out);
int crt_scene_info_get(const crt_scene* scene, crt_scene_info* info);
/* nodes: num_nodes entries; prim_order: num_primitives entries (slot -> primitive index). */
int crt_scene_export_bvh(const crt_scene* scene, crt_bvh_node* nodes, uint32_t* prim_order);
/* Copy the scene into HBM of `device` (synchronous). Idempotent. */
int crt_scene_upload(crt_scene* scene, int device);
/* The scene's copy in HBM of `device` (uploaded first if needed) copied to host memory: bytes =
 * crt_scene_info.device_bytes. The layout is internal (tests and tooling compare copies). */
int crt_scene_image(crt_scene* scene, int device, void* host, size_t bytes);
void crt_scene_destroy(crt_scene* scene);

/* Camera::init() (camera.h:87-157). */
int crt_camera_resolve(const crt_camera_settings* settings, crt_camera* out);

/* Render the owned rows of the frame into d_rgb (DEVICE pointer on the scene's device,
 * image_h*image_w*3 doubles, row-major, the layout of Image::operator[] image.h:32-33; with
 * CRT_TILING_PACKED only owned_rows*image_w*3 doubles, the owned rows in order).
 * Enqueued on `stream`; returns without waiting. Rows not owned are left untouched.
 * Output is the per-pixel mean over samples_per_pixel samples (camera.h:285-292). */
int crt_render_async(const crt_scene* scene, int device, const crt_camera* cam,
                     const crt_tiling* tiling, double* d_rgb, void* stream);

/* ---- progressive rendering ---------------------------------------------------------------
 * A render's samples are grouped into chunks of crt_sample_chunk_len(samples_per_pixel) samples
 * (the last chunk of a pixel may be shorter); a pixel's value is the chunk sums added in chunk
 * order, times 1 / samples_per_pixel. A render cut into passes at chunk boundaries and
 * accumulated in chunk order makes the same additions, so its final frame equals the one-shot
 * frame of crt_render_async bit for bit. */

/* Samples per chunk of a render with this many samples per pixel: max(4, ceil(spp / 192)).
 * Pass boundaries are multiples of it. */
uint32_t crt_sample_chunk_len(uint32_t samples_per_pixel);

/* One pass: samples [first_sample, first_sample + num_samples) of every owned pixel, of a job of
 * cam->samples_per_pixel samples in all (that total fixes the chunking and the seeds).
 *   d_sum    DEVICE, the layout of crt_render_async's d_rgb (whole frame, or the owned rows packed
 *            under CRT_TILING_PACKED): the pixels' running sums. first_sample == 0 overwrites it
 *            (and d_noise); any other pass adds to it.
 *   d_noise  DEVICE or NULL, 2 doubles per pixel at the same pixel addresses: t = sum of y and
 *            q = sum of y * y over the full-length chunks so far, y = (r + g) + b of a chunk's sum
 *            (the state crt_noise_estimate reads). A ragged last chunk is left out.
 *   d_rgb    DEVICE or NULL, as crt_render_async's: the frame so far, sum * (1 / (double)(first_sample
 *            + num_samples)); after the last pass, the one-shot frame.
 * CRT_E_INVALID (the message names the rule) unless first_sample is a multiple of the chunk
 * length, num_samples > 0, first_sample + num_samples <= samples_per_pixel, the end is a multiple
 * of the chunk length or equals samples_per_pixel, and d_sum is not NULL.
 * Scratch of pass renders (this call, crt_render_pass_masked_async, crt_noise_estimate,
 * crt_adaptive_update and the blocking drivers over them) comes from a stream-ordered memory pool
 * the library creates per device and never trims: it holds the largest scratch a pass needed (the
 * pass's partial sums, at most 4 GiB or CRT_PARTIAL_MB) until the process ends. The process's
 * default pool is not used or changed by them. CRT_E_HIP if the pool cannot be created.
 * The call keeps no state: issuing each pass once, in increasing order, on one stream (or
 * otherwise ordered) is the caller's job. In order, the final frame is bit-identical to the
 * one-shot frame; passes after the first issued out of order still give a correct mean, equal
 * within rounding (floating-point addition is not associative). Enqueued on `stream`. */
int crt_render_pass_async(const crt_scene* scene, int device, const crt_camera* cam,
                          const crt_tiling* tiling, uint32_t first_sample, uint32_t num_samples,
                          double* d_sum, double* d_noise, double* d_rgb, void* stream);

/* Noise of `pixels` d_noise records (device memory on `device`) after samples_done samples of a
 * samples_per_pixel job. With L = the chunk length and K = samples_done / L full chunks, a pixel
 * has m = t / (K L), the mean of r + g + b, and se = sqrt(max(0, q / L^2 - K m^2) / (K (K - 1))),
 * the standard error of m. *sum_se and *sum_mean (HOST) receive the sums of se and of m over the
 * pixels; sum_se / sum_mean is the frame's relative noise. Both are NaN while K < 2. The sums are
 * taken in a fixed order: repeated calls give the same bits. Synchronous on `stream`. */
int crt_noise_estimate(int device, const double* d_noise, size_t pixels, uint32_t samples_per_pixel,
                       uint32_t samples_done, double* sum_se, double* sum_mean, void* stream);

/* Progress callback of crt_render_progressive, called on the calling thread after every pass:
 * noise is sum_se / sum_mean over the frame with CRT_PROGRESS_NOISE (NaN without it, or before two
 * chunks are done); h_rgb is the caller's frame buffer holding the frame so far with
 * CRT_PROGRESS_PREVIEW, else NULL. A non-zero return stops the render. */
typedef int (*crt_progress_fn)(void* user, uint32_t samples_done, uint32_t samples_total,
                               double noise, const double* h_rgb);
#define CRT_PROGRESS_NOISE 1u
#define CRT_PROGRESS_PREVIEW 2u

/* Blocking whole-frame render over devices [0, num_devices) as crt_render's, in passes of
 * samples_per_pass samples (rounded up to whole chunks; 0 = a tenth of the job, at least one
 * chunk). fn may be NULL. h_rgb (HOST, image_w*image_h*3 doubles) is written after every pass with
 * CRT_PROGRESS_PREVIEW, else once when the render ends. When it ends after all samples h_rgb is
 * crt_render's frame bit for bit; when fn stops it, the mean of the *samples_done (may be NULL)
 * samples rendered so far. */
int crt_render_progressive(crt_scene* scene, const crt_camera* cam, int num_devices,
                           uint32_t samples_per_pass, uint32_t flags, crt_progress_fn fn, void* user,
                           double* h_rgb, uint32_t* samples_done);

/* ---- adaptive sampling --------------------------------------------------------------------
 * A block is the render kernel's tile: CRT_BLOCK_W columns x CRT_BLOCK_H owned rows. Block
 * (bx, by) covers columns [16 bx, 16 bx + 16) and owned rows [4 by, 4 by + 4) (edge blocks are
 * smaller) and has the number by * ceil(image_w / 16) + bx. Block state, d_blocks, is one uint32_t
 * per block in device memory: the samples accumulated in each of the block's pixels, plus the bit
 * CRT_BLOCK_STOPPED. Between passes crt_adaptive_update stops the blocks whose noise is below a
 * threshold; a masked pass renders the others. A block that stops after n samples holds, bit for
 * bit, what crt_render_pass_async's passes hold after n samples.
 * The adaptive calls take a tiling only with tile_count == 1 or row_block % 4 == 0 (else
 * CRT_E_INVALID): a rank's blocks are then blocks of the frame, whatever the number of ranks. */
#define CRT_BLOCK_W 16
#define CRT_BLOCK_H 4
#define CRT_BLOCK_STOPPED 0x80000000u

/* Blocks of owned_rows rows of an image_w wide frame: ceil(image_w / 16) * ceil(owned_rows / 4). */
size_t crt_block_count(uint32_t image_w, uint32_t owned_rows);

/* crt_render_pass_async (its rules, checked before any device work) for the blocks with
 * d_blocks[b] == first_sample only; a stopped block never matches. A rendered block gets exactly
 * crt_render_pass_async's additions, in its order, into d_sum and d_noise, and its word becomes
 * first_sample + num_samples. A skipped block: with first_sample > 0, d_sum and d_noise are left
 * alone and d_rgb (if given) gets sum * (1 / (double)n), n = the block's own count (0 when n = 0);
 * with first_sample == 0 its pixels' d_sum, d_noise and d_rgb are written 0, so a caller may
 * pre-set CRT_BLOCK_STOPPED on blocks to render a region only. The caller zeroes d_blocks
 * (crt_block_count words, DEVICE) before the first pass.
 * active_hint: the number of blocks the caller expects to be rendered (0 = unknown: all of them).
 * It sizes the grid and the work items only: any value gives the same bits. */
int crt_render_pass_masked_async(const crt_scene* scene, int device, const crt_camera* cam,
                                 const crt_tiling* tiling, uint32_t first_sample, uint32_t num_samples,
                                 double* d_sum, double* d_noise, double* d_rgb, uint32_t* d_blocks,
                                 uint32_t active_hint, void* stream);

/* The stopping rule, for every block with d_blocks[b] == samples_done. With L = the chunk length
 * and K = samples_done / L, sum_se and sum_m are the sums over the block's pixels of
 * crt_noise_estimate's se and m (in a fixed order that depends on the block's shape only). The
 * block gets CRT_BLOCK_STOPPED iff K >= 2, samples_done >= min_samples and
 * sum_se <= threshold * sum_m: no division, so an all-black block (0 <= 0) stops, and a NaN
 * (compares false) never does. min_samples >= samples_per_pixel: never stop. threshold must be
 * finite and >= 0; samples_done a multiple of the chunk length, or samples_per_pixel.
 * *active_blocks (HOST) receives the number of blocks still at samples_done and
 * not stopped. Synchronous on `stream`. */
int crt_adaptive_update(int device, const crt_camera* cam, const crt_tiling* tiling, const double* d_noise,
                        uint32_t* d_blocks, uint32_t samples_done, double threshold, uint32_t min_samples,
                        uint32_t* active_blocks, void* stream);

typedef struct crt_adaptive_params {
    double threshold;          /* a block stops at sum_se <= threshold * sum_m                    */
    uint32_t min_samples;      /* ... and not before this many samples                           */
    uint32_t samples_per_pass; /* as crt_render_progressive's (0 = a tenth of the job)           */
    uint32_t flags;            /* CRT_PROGRESS_PREVIEW                                           */
    uint32_t reserved;         /* must be 0 (CRT_E_INVALID otherwise)                            */
} crt_adaptive_params;

/* Called on the calling thread after every pass and update; h_rgb as crt_progress_fn's. A non-zero
 * return stops the render. */
typedef int (*crt_adaptive_fn)(void* user, uint32_t samples_done, uint32_t samples_total,
                               uint32_t active_blocks, uint32_t total_blocks, const double* h_rgb);

/* Blocking adaptive render over devices [0, num_devices), rows dealt as crt_render_progressive's:
 * one masked pass and one update per step on every device, until no block is active, all samples
 * are done, or fn stops it. h_rgb: every pixel's mean over its block's own samples.
 * h_block_samples (HOST, crt_block_count(image_w, image_h) words, or NULL): the frame's block
 * counts in frame block order, the stopped bit cleared. *samples_rendered (or NULL): the sum over
 * the pixels of their counts. */
int crt_render_adaptive(crt_scene* scene, const crt_camera* cam, int num_devices,
                        const crt_adaptive_params* params, crt_adaptive_fn fn, void* user, double* h_rgb,
                        uint32_t* h_block_samples, uint64_t* samples_rendered);

/* ---- denoising ----------------------------------------------------------------------------
 * A frame that stopped early (progressive passes, adaptive sampling) is noisy. The calls below
 * filter it with an edge-stopping a-trous wavelet filter guided by first-hit features and by the
 * per-pixel variance the noise state already holds. Everything here is specified as IEEE f64
 * expressions of + - * / in a fixed order (host and device build with -ffp-contract=off), so a
 * restatement on the CPU gives the same bits (tests/denoise_model.py is one).
 * Limits: the features are those of the first hit only, so detail seen through glass or in
 * mirrors is guided by colour and variance alone; albedo is reported but not divided out before
 * filtering (no albedo demodulation): textures would blur, the reference's materials have none.
 * The filter itself runs on one device; crt_render_denoised_devices renders over several devices
 * and gathers frame, variance and features to device 0 for it.
 * Below, max0(x) = x > 0 ? x : 0 (so -0 and NaN give +0), y(c) = (c0 + c1) + c2 and
 * dot(a, b) = (a0 * b0 + a1 * b1) + a2 * b2. */

/* First-hit features of one pixel. */
typedef struct crt_feature {
    double albedo[3];  /* Lambertian, Metal, DiffuseLight: material colour; Dielectric: 1,1,1; miss: cam->background */
    double normal[3];  /* faces the ray, as crt_hit.normal; miss: 0,0,0 */
    double point[3];   /* as crt_hit.point; miss: 0,0,0 */
    double t;          /* as crt_hit.t; miss: 0 */
    int32_t prim;      /* as crt_hit.prim; -1 = miss */
    uint32_t material; /* as crt_hit.material; miss: 0 */
} crt_feature;         /* 88 bytes */

/* Features of the owned pixels into d_feat (DEVICE, one record per pixel at crt_render_async's
 * pixel addresses: whole frame, or the owned rows packed under CRT_TILING_PACKED; rows not owned
 * are left untouched). One ray per pixel (row, col) from cam->origin through the pixel's centre,
 * no defocus offset and no jitter: per component k
 *   center = (pixel00[k] + pixel_delta_y[k] * row) + pixel_delta_x[k] * col,  d[k] = center - origin[k]
 * (random_ray_through_pixel's order with the random terms left out), over the interval
 * (cam->t_min, +inf), traced as crt_closest_hits traces it. The parity guard count is not touched.
 * The first call for a scene and device builds a table of primitive numbers and uploads it,
 * blocking; after that the call only enqueues on `stream`. Scratch comes from the pass pool. */
int crt_render_features_async(const crt_scene* scene, int device, const crt_camera* cam,
                              const crt_tiling* tiling, crt_feature* d_feat, void* stream);

/* Per-pixel variance of the mean from the noise state d_noise (t, q per pixel), into d_var
 * (DEVICE, 1 double per pixel at d_noise's pixel addresses; owned rows only).
 * n = samples_done when d_blocks is NULL, else the pixel's block word with CRT_BLOCK_STOPPED
 * cleared (block = crt_block_count's numbering over the owned rows). L = the chunk length of
 * cam->samples_per_pixel, K = n / L (integer division), both then taken as doubles:
 *   m = t / (K * L)
 *   v = max0(q / (L * L) - (K * m) * m) / (K * (K - 1))            for K >= 2,
 * the square of crt_noise_estimate's se (its operations in its order, without the final sqrt, and
 * with max0 where it calls fmax: the two differ for -0 and NaN only);
 *   v = m * m for K == 1 (a finite 100 %-error stand-in), v = 0 for K == 0.
 * CRT_E_INVALID (the message names the rule) unless samples_done <= samples_per_pixel and it is a
 * multiple of the chunk length or equals samples_per_pixel; with d_blocks the tiling must have
 * tile_count == 1 or row_block % 4 == 0, as for crt_adaptive_update. Enqueued on `stream`. */
int crt_pixel_variance_async(int device, const crt_camera* cam, const crt_tiling* tiling, const double* d_noise,
                             const uint32_t* d_blocks, uint32_t samples_done, double* d_var, void* stream);

typedef struct crt_denoise_params {
    uint32_t iterations;        /* 1..8; step of iteration i (from 0) is 2^i                     */
    uint32_t normal_squarings;  /* 0..10: normal weight = max0(n_p . n_q)^(2^this)               */
    double sigma_l;             /* colour tolerance in standard errors, finite, > 0              */
    double sigma_p;             /* plane-distance tolerance as a fraction of t_p, finite, > 0    */
    uint32_t flags, reserved;   /* must be 0                                                     */
} crt_denoise_params;

/* The filter. d_rgb (w*h*3), d_var (w*h), d_feat (w*h records): whole-frame, unpacked DEVICE
 * buffers on `device`; d_out (w*h*3) receives the filtered frame and d_var_out (w*h, or NULL) its
 * variance. Neither output may overlap an input or the other output (CRT_E_INVALID). Ping-pong
 * scratch comes from the pass pool. Enqueued on `stream`.
 * Iteration i = 0 .. iterations - 1 maps the current (c, v) (the inputs at i = 0) to (c', v') with
 * step = 2^i; for pixel p = (x, y), features n (normal), P (point), t, prim:
 *   Variance pre-filter: vbar = 0.0; for dy = -1..1 (outer), dx = -1..1 (inner):
 *       vbar = vbar + (g[dy] * g[dx]) * v(q),  q = (clamp(x + dx, 0, w - 1), clamp(y + dy, 0, h - 1)),
 *       g = {1/4, 1/2, 1/4}.
 *   Colour tolerance: D = (sigma_l * sigma_l) * vbar + (1e-6 * (y_p * y_p) + DBL_MIN), y_p = y(c_p).
 *   Taps: W = 0.0, C[j] = 0.0, V = 0.0; for dy = -2..2 (outer), dx = -2..2 (inner),
 *       q = (x + step * dx, y + step * dy), k = h[dy] * h[dx], h = {1/16, 1/4, 3/8, 1/4, 1/16}:
 *     the tap is skipped when q is outside the frame, or when any of c_q's channels or v_q is not
 *     finite, or when exactly one of prim_p, prim_q is < 0;
 *     both prims < 0:  N = 1, b = 0;
 *     otherwise:       N = max0(dot(n_p, n_q)), then N = N * N normal_squarings times,
 *                      e = dot(P_q - P_p, n_p)  (the differences per component first),
 *                      b = (e * e) / ((sigma_p * sigma_p) * (t_p * t_p));
 *     d = y(c_q) - y_p,  a = (d * d) / D,
 *     w = (k * N) / ((1 + a) * (1 + b))                              (one division)
 *     W = W + w;  C[j] = C[j] + w * c_q[j] (j = 0, 1, 2);  V = V + (w * w) * v_q.
 *   Result: c'[j] = C[j] / W, v' = V / (W * W); if any channel of c_p or v_p is not finite, or W
 *   is not > 0 (a NaN included), the pixel is copied through: c' = c_p, v' = v_p.
 * The kernels take small steps from an LDS tile and large steps as gathers; both evaluate these
 * expressions in this order, so the result does not depend on the route. */
int crt_denoise_async(int device, uint32_t w, uint32_t h, const double* d_rgb, const double* d_var,
                      const crt_feature* d_feat, const crt_denoise_params* params, double* d_out,
                      double* d_var_out, void* stream);

/* Blocking denoised render on one device: the passes of crt_render_progressive (adaptive == NULL:
 * all samples) or the masked passes and updates of crt_render_adaptive (its rules for *adaptive;
 * flags must be 0), then crt_render_features_async, crt_pixel_variance_async and
 * crt_denoise_async on the same stream. h_rgb (HOST, image_w*image_h*3) receives the denoised
 * frame; h_noisy (HOST, same size, or NULL) the unfiltered one, bit for bit the frame of
 * crt_render_progressive / crt_render_adaptive on one device; *samples_rendered (or NULL) the sum
 * over the pixels of their sample counts. Over several devices, or with a denoised preview after
 * every pass: crt_render_denoised_devices. */
int crt_render_denoised(crt_scene* scene, int device, const crt_camera* cam, const crt_adaptive_params* adaptive,
                        const crt_denoise_params* denoise, double* h_noisy, double* h_rgb,
                        uint64_t* samples_rendered);

/* Callback of crt_render_denoised_devices, called on the calling thread after every pass (and
 * update). With CRT_PROGRESS_PREVIEW h_rgb is the caller's frame buffer holding the denoised frame
 * of the state so far and h_noisy the caller's unfiltered one (NULL if the caller gave none);
 * without it both are NULL. A non-zero return stops the render. */
typedef int (*crt_denoised_fn)(void* user, uint32_t samples_done, uint32_t samples_total,
                               uint32_t active_blocks, uint32_t total_blocks,
                               const double* h_noisy, const double* h_rgb);

/* Blocking denoised render over devices [0, num_devices): num_devices and CRT_EMULATE_DEVICES as
 * in crt_render_adaptive, rows dealt as crt_tiling{4, n, d}, packed; devices that own no rows are
 * legal. Every device renders its rows, takes their variance and packs the filter's records; device
 * 0 gathers the records and the frame rows and runs the filter over the whole frame.
 *   adaptive == NULL: one plain pass of all samples, as in crt_render_denoised; fn (may be NULL)
 *     is called once, with active_blocks = 0.
 *   adaptive != NULL: the masked passes and updates of crt_render_adaptive, under its rules for
 *     *adaptive; flags may be 0 or CRT_PROGRESS_PREVIEW (the one difference from
 *     crt_render_denoised). min_samples >= samples_per_pixel never stops a block: plain passes
 *     with previews.
 *   CRT_PROGRESS_PREVIEW with fn != NULL: before each call of fn, h_rgb (HOST, image_w*image_h*3)
 *     holds the denoised frame of the state so far and h_noisy (HOST, same size, or NULL) the
 *     unfiltered one; fn receives both pointers. Otherwise both buffers are written once, when the
 *     render ends, and fn receives NULL for both.
 *   A non-zero return from fn stops the render; the frames then describe the samples done so far.
 * Every rule is checked before any device work (CRT_E_INVALID, the message names the rule).
 * Bit contract: h_noisy is the frame crt_render_adaptive (crt_render_progressive when adaptive ==
 * NULL) produces for the same job. h_rgb is crt_denoise_async applied to that frame,
 * crt_pixel_variance_async of the job's noise state (with the block words when adaptive) and
 * crt_render_features_async of the whole frame. Hence h_rgb equals crt_render_denoised's frame on
 * one device, for any num_devices. h_block_samples (or NULL; every word samples_per_pixel when
 * adaptive == NULL) and *samples_rendered (or NULL) mean what they mean in crt_render_adaptive.
 * Device 0 holds the whole-frame records (128 bytes a pixel), the unfiltered frame and the output;
 * every other buffer is a device's own share. */
int crt_render_denoised_devices(crt_scene* scene, const crt_camera* cam, int num_devices,
                                const crt_adaptive_params* adaptive, const crt_denoise_params* denoise,
                                crt_denoised_fn fn, void* user, double* h_noisy, double* h_rgb,
                                uint32_t* h_block_samples, uint64_t* samples_rendered);

/* Instrumented pass: counts the work of the same render (never timed). */
int crt_render_count(const crt_scene* scene, int device, const crt_camera* cam,
                     const crt_tiling* tiling, crt_render_stats* stats);

/* Blocking whole-frame render over devices [0, num_devices): rows are dealt to devices in
 * blocks of 4 (crt_tiling{4, num_devices, d}), rendered concurrently, and gathered into HOST
 * memory h_rgb. */
int crt_render(crt_scene* scene, const crt_camera* cam, int num_devices, double* h_rgb,
               crt_render_stats* stats);

/* crt_render fused with Image::send_as_ppm's integers (image.h:38-56; RGB::as_string
 * rgb.h:99-115, the values crt_ppm_values gives): every device tone-maps its own rows to 8-bit
 * values before the gather, so 3 bytes a pixel cross xGMI and PCIe instead of 24. h_values: host,
 * image_w*image_h*3 int32, identical to crt_ppm_values of crt_render's frame. */
int crt_render_ppm(crt_scene* scene, const crt_camera* cam, int num_devices, int32_t* h_values,
                   crt_render_stats* stats);

/* Closest hits of n rays (host arrays; rays[i] = {ox,oy,oz,dx,dy,dz}) against the scene on
 * `device`, time interval (t_min, t_max) exclusive, as BVH::hit_by (bvh.h:585-715). */
int crt_closest_hits(crt_scene* scene, int device, const double* rays, size_t n,
                     double t_min, double t_max, crt_hit* out);

/* Ray queries on device buffers: crt_closest_hits without the host round trip, through the render
 * kernel's traversal (f32 node test, LDS scene and stack, speculative and sibling-pair walks, f32
 * leaf filters). */
#define CRT_TRACE_ANY   1u  /* occlusion: is there any accepted primitive in the interval */
#define CRT_TRACE_PLAIN 2u  /* hits_kernel's walk (trace()) on the same buffers: the cross-check and the A/B */
typedef struct crt_trace_params {
    double t_min, t_max;      /* exclusive interval, as BVH::hit_by; t_min finite, t_max not NaN (+inf allowed) */
    uint32_t flags, reserved; /* unknown flag bits or reserved != 0: CRT_E_INVALID */
} crt_trace_params;           /* 24 bytes */

/* d_rays: DEVICE memory on `device`, n x {ox, oy, oz, dx, dy, dz}. d_tmax: DEVICE, n doubles, or
 * NULL; with it ray i's upper bound is d_tmax[i] instead of params->t_max (t_min is call-wide).
 * Closest mode (no CRT_TRACE_ANY): d_hits[i] (DEVICE, n records) is exactly the record
 *   crt_closest_hits writes for that ray and interval (a miss: prim = -1, every other field zero);
 *   d_occluded must be NULL.
 * Any mode (CRT_TRACE_ANY): d_occluded[i] (DEVICE, n words) = 1 iff closest mode would report
 *   prim >= 0, else 0; d_hits must be NULL.
 * A ray with a non-finite component, an all-zero direction or a NaN upper bound is outside the
 * contract: it is not traced and is written as a miss.
 * The scene must be resident on `device` (CRT_E_NOT_UPLOADED). The first closest-mode call for a
 * scene and device builds the table of primitive numbers and uploads it, blocking (the table
 * crt_render_features_async uses); after that the call only enqueues on `stream`. Scratch comes
 * from the pass pool. n == 0 is CRT_OK with no work. CRT_E_INVALID, checked before any device work
 * (the message names the rule): n > 2^31 - 1, d_rays or params NULL, t_min not finite, t_max NaN,
 * unknown flags, reserved != 0, an output pointer missing for the mode or given for the other one.
 * Both routes obey the render kernel's run-time switches. */
int crt_trace_async(const crt_scene* scene, int device, const double* d_rays, size_t n,
                    const double* d_tmax, const crt_trace_params* params,
                    crt_hit* d_hits, uint32_t* d_occluded, void* stream);

/* crt_trace_async for HOST arrays, blocking: uploads the scene to `device` if it is not resident,
 * then one upload of the rays (and bounds), one query on a stream of its own, one copy back. Same
 * rules, same results (the C++ drop-in's BVH::hit_by_batch / occluded_batch). */
int crt_trace(crt_scene* scene, int device, const double* rays, size_t n, const double* tmax,
              const crt_trace_params* params, crt_hit* hits, uint32_t* occluded);

/* Radiance queries on device buffers: ray_color (camera.h:205-258) for the caller's own rays, through
 * the render kernel's traversal and its shading, one path a ray. */
#define CRT_RADIANCE_PLAIN 1u /* one thread a path over trace(): the cross-check and the A/B */
typedef struct crt_radiance_params {
    uint32_t max_depth;       /* ray_color's depth (camera.h:207-213) */
    uint32_t base_seed;       /* used only when d_states == NULL */
    double   background[3];   /* finite */
    double   t_min;           /* finite, >= 0, <= 2^100; the camera's is 1e-5 */
    uint32_t flags, reserved; /* unknown flag bits or reserved != 0: CRT_E_INVALID */
} crt_radiance_params;        /* 48 bytes */

/* d_rays: DEVICE memory on `device`, n x {ox, oy, oz, dx, dy, dz}: ray i is path i's first segment.
 * d_states: DEVICE, n words, or NULL. Path i's LCG state before the first draw of ray_color is
 *   d_states[i], or crt_sample_seed(base_seed, (uint32_t)i, 0) when d_states == NULL. Any 32-bit
 *   state is legal (the LCG is mod 2^32).
 * d_rgb: DEVICE, 3n doubles. d_rgb[3i .. 3i + 2] is exactly what that sample adds to a pixel's sum
 *   in crt_render_async. With T the product of the attenuations in bounce order, starting from
 *   (1, 1, 1), and E the background (the path ends at a miss) or the material's precomputed emission
 *   (it ends at a DiffuseLight), channel k is 0.0 + T[k] * E[k]. Every other path writes +0 in every
 *   channel: max_depth == 0 (nothing is traced then), an absorbed ray, a scattered ray with no bounce
 *   left.
 * Every segment is traced over (t_min, +inf). The caller's ray is classified by crt_trace_async's
 * contract before anything is traced: one with a non-finite component or an all-zero direction is a
 * miss, 0.0 + 1 * background[k] (+0 with max_depth == 0). Scattered rays are traced as a render
 * traces them. Dielectric decisions count into the scene's parity guard (crt_render_guard) as a
 * render's do.
 * The scene must be resident on `device` (CRT_E_NOT_UPLOADED). Scratch comes from the pass pool; the
 * call only enqueues on `stream`. n == 0 is CRT_OK with no work. CRT_E_INVALID, checked before any
 * device work (the message names the rule): scene or params NULL, unknown flags, reserved != 0,
 * t_min outside [0, 2^100] or NaN, a background component not finite, n > 2^31 - 1, d_rgb or d_rays
 * NULL with n > 0. Both routes obey the render kernel's run-time switches and give
 * the same bits. One device, one path per ray, one t_min and depth per call. */
int crt_radiance_async(const crt_scene* scene, int device, const double* d_rays, size_t n,
                       const uint32_t* d_states, const crt_radiance_params* params,
                       double* d_rgb, void* stream);

/* crt_radiance_async for HOST arrays, blocking: uploads the scene to `device` if it is not resident,
 * then one upload of the rays (and states), one query on a stream of its own, one copy back. Same
 * rules, same results (the C++ drop-in's Camera::ray_colors). */
int crt_radiance(crt_scene* scene, int device, const double* rays, size_t n, const uint32_t* states,
                 const crt_radiance_params* params, double* rgb);

/* The camera's own rays: random_ray_through_pixel (camera.h:184-200, defocus disk :160-168) as a
 * kernel, one thread a record. Pixels are the tiling's owned pixels, owned rows in order, packed (as
 * under CRT_TILING_PACKED; tiling == NULL: the whole frame): pixel j = k * image_w + col for owned
 * row k. For sample s in [first_sample, first_sample + num_samples), record
 * r = j * num_samples + (s - first_sample) holds
 *   d_rays[6r .. 6r + 5] (DEVICE): the ray whose draws start from the state
 *     crt_sample_seed(cam->base_seed, row * image_w + col, s), row = the frame row of owned row k;
 *   d_states[r] (DEVICE): the state after those draws,
 * so crt_radiance_async on the two buffers with cam's max_depth, background and t_min gives the
 * radiance of the samples crt_render_async sums for that pixel, bit for bit. Enqueues on `stream`.
 * CRT_E_INVALID: cam, d_rays or d_states NULL, a bad tiling, first_sample + num_samples > 2^32 - 1,
 * more than 2^31 - 1 records. No records (no owned rows, num_samples == 0) is CRT_OK. */
int crt_camera_rays_async(int device, const crt_camera* cam, const crt_tiling* tiling,
                          uint32_t first_sample, uint32_t num_samples,
                          double* d_rays, uint32_t* d_states, void* stream);

/* Irradiance probes: a whole probe bake on the device. For each of n points, S directions are drawn
 * on the device, traced by crt_radiance_async's integrator and reduced in a fixed order to nine
 * spherical-harmonic coefficients a colour channel (SPHERE) or one cosine-weighted irradiance value
 * (HEMISPHERE). Every output bit is specified below; it depends on neither the grid nor the batch
 * size nor the radiance route. */
#define CRT_PROBE_SPHERE     0u  /* uniform directions; K = 9 SH coefficients (bands 0..2) per channel */
#define CRT_PROBE_HEMISPHERE 1u  /* cosine-weighted about the normal; K = 1: irradiance */
typedef struct crt_probe_params {
    uint32_t samples;        /* S, 1 .. 2^20 */
    uint32_t max_depth;      /* as crt_radiance_params */
    uint32_t base_seed;
    uint32_t mode;           /* CRT_PROBE_SPHERE or CRT_PROBE_HEMISPHERE */
    double   background[3];  /* finite */
    double   t_min;          /* finite, >= 0, <= 2^100 (crt_radiance_params' rule) */
    uint32_t batch_probes;   /* probes per internal batch; 0 = the library picks. Sizes only: any value gives the same bits */
    uint32_t flags;          /* 0 or CRT_RADIANCE_PLAIN (passed to the radiance query) */
} crt_probe_params;          /* 56 bytes */

/* The bake's first stage, also callable on its own: the rays and LCG states of n probes, S = samples
 * records a probe, record r = p * S + s (probe-major). Of params only samples, base_seed and mode
 * are used, the rest is checked as in crt_probes_async.
 *   The state starts as crt_sample_seed(base_seed, (uint32_t)p, s). u = Vec3D::random_unit_vector
 *   (vec3d.h:64-75) on it, as a render's shading draws it: x, y, z = crt_rand_double(state, -1, 1)
 *   in that order until x*x + y*y + z*z < 1, then each times 1 / sqrt(x*x + y*y + z*z) (IEEE sqrt and
 *   division).
 *   d_rays[6r .. 6r + 5] (DEVICE) = {P, d}, P = d_points[3p .. 3p + 2]; SPHERE: d = u; HEMISPHERE:
 *   d[k] = N[k] + u[k], N = d_normals[3p .. 3p + 2], the caller's unit normal, which the library does
 *   not normalise. d_states[r] (DEVICE) = the state after the draws: the path's state.
 * Lambertian's near_zero substitution (material.h) is not made: a generated ray outside
 * crt_trace_async's contract (a non-finite component, e.g. from a NaN point, or d = 0 when u = -N
 * exactly) is a miss under crt_radiance_async's rule and sees the background.
 * CRT_E_INVALID as crt_probes_async's, and for n * samples > 2^31 - 1 records or a NULL output with
 * n > 0. n == 0 is CRT_OK with no work. Enqueues on `stream`. */
int crt_probe_rays_async(int device, const double* d_points, const double* d_normals, size_t n,
                         const crt_probe_params* params, double* d_rays, uint32_t* d_states, void* stream);

/* d_points: DEVICE memory on `device`, n x 3. d_normals: DEVICE, n x 3, required for HEMISPHERE and
 * NULL for SPHERE. d_coeff: DEVICE, n x K x 3 doubles, d_coeff[(p * K + k) * 3 + j] for probe p,
 * coefficient k, channel j.
 * Paths: L_s = crt_radiance_async's output (max_depth, background, t_min, flags of params) for the ray
 * and state of record p * S + s of crt_probe_rays_async.
 * Basis (SPHERE), with (x, y, z) = d_s:
 *   Y0 = 0.28209479177387814
 *   Y1 = 0.4886025119029199 * y,  Y2 = 0.4886025119029199 * z,  Y3 = 0.4886025119029199 * x
 *   Y4 = 1.0925484305920792 * (x * y),  Y5 = 1.0925484305920792 * (y * z),  Y7 = 1.0925484305920792 * (x * z)
 *   Y6 = 0.31539156525252005 * ((3.0 * z) * z - 1.0)
 *   Y8 = 0.5462742152960396 * (x * x - y * y)
 * HEMISPHERE has the single term Y = 1, used without a multiply.
 * Reduction, per probe p, coefficient k, channel j: the term of sample s is Y_k(d_s) * L_s[j]. Lane l
 * (0..63) starts at 0.0 and adds the terms of samples s = l, l + 64, ... in increasing s. Then for
 * step = 32, 16, 8, 4, 2, 1, lane l < step becomes lane[l] + lane[l + step]. The result is
 * lane[0] * (W / (double)S), W = 12.566370614359172 (4 pi) for SPHERE and 3.141592653589793 for
 * HEMISPHERE (the pdf is cos / pi, so E = pi * mean). No floating-point atomics are used.
 * Batches: the probes are traced in batches of batch_probes whole probes (0: the most whose scratch
 * of 76 bytes a record stays at or under 256 MiB; never fewer than one, never more than 2^31 - 1
 * records), each generated, traced, reduced and freed in order on `stream`, scratch from the pass
 * pool. Nothing is accumulated across batches.
 * max_depth == 0 writes every coefficient +0 and n == 0 is CRT_OK with no work; neither launches a
 * kernel. The scene must be resident on `device` (CRT_E_NOT_UPLOADED). CRT_E_INVALID, checked before
 * any device work (the message names the rule): scene or params NULL, samples outside 1 .. 2^20,
 * unknown mode, unknown flags, t_min outside [0, 2^100] or NaN, a background component not finite,
 * n > 2^31 - 1, d_normals NULL for HEMISPHERE or given for SPHERE, d_points or d_coeff NULL with
 * n > 0. Dielectric decisions count into the scene's parity guard as crt_radiance_async's do.
 * One device, one depth and t_min a call, bands 0..2, no per-probe noise estimate. */
int crt_probes_async(const crt_scene* scene, int device, const double* d_points, const double* d_normals,
                     size_t n, const crt_probe_params* params, double* d_coeff, void* stream);

/* crt_probes_async for HOST arrays, blocking: uploads the scene to `device` if it is not resident,
 * then one upload of the points (and normals), the bake on a stream of its own, one copy back. Same
 * rules, same results (the C++ drop-in's Camera::probes). */
int crt_probes(crt_scene* scene, int device, const double* points, const double* normals, size_t n,
               const crt_probe_params* params, double* coeff);

/* Evaluates SPHERE coefficients: query i reads probe d_index[i] of d_coeff (DEVICE, num_probes x 9 x
 * 3) at the unit direction d_dirs[3i .. 3i + 2] (DEVICE) and writes d_rgb[3i .. 3i + 2] (DEVICE):
 * channel j is the sum over k = 0..8, in k order from 0.0, of A_k * (c[k][j] * Y_k(dir)), with
 * crt_probes_async's basis. `what` = CRT_SH_RADIANCE: every A_k = 1, the band-limited radiance from
 * direction dir. CRT_SH_IRRADIANCE: A_0 = CRT_SH_A0, A_1..3 = CRT_SH_A1, A_4..8 = CRT_SH_A2 (the
 * clamped-cosine lobe's band factors), the irradiance of a surface with normal dir. A query with
 * d_index[i] >= num_probes is written as zeros. m == 0 is CRT_OK with no work. CRT_E_INVALID:
 * what > 1, m > 2^31 - 1, a NULL pointer with m > 0. Enqueues on `stream`. */
#define CRT_SH_RADIANCE   0u
#define CRT_SH_IRRADIANCE 1u
#define CRT_SH_A0 3.141592653589793   /* pi */
#define CRT_SH_A1 2.0943951023931953  /* 2 pi / 3 */
#define CRT_SH_A2 0.7853981633974483  /* pi / 4 */
int crt_sh_eval_async(int device, const double* d_coeff, size_t num_probes, const uint32_t* d_index,
                      const double* d_dirs, size_t m, uint32_t what, double* d_rgb, void* stream);

/* Lens renders: a whole frame through a caller-chosen projection. The rays are generated on the
 * device, traced by crt_radiance_async's integrator unchanged and summed per pixel in
 * crt_render_async's order. Every output bit is specified below (up to the device library's sin and
 * cos for EQUIRECT and FISHEYE); it depends on neither the grid nor the batch size nor the radiance
 * route. */
#define CRT_LENS_PINHOLE       0u  /* the reference camera: cam's own origin, pixel00, deltas, defocus disk */
#define CRT_LENS_ORTHOGRAPHIC  1u
#define CRT_LENS_EQUIRECT      2u
#define CRT_LENS_FISHEYE       3u  /* equidistant */
#define CRT_LENS_CUBE          4u  /* six 90-degree faces stacked top to bottom: image_h == 6 * image_w */
typedef struct crt_lens {
    uint32_t kind, flags;        /* flags: CRT_RADIANCE_PLAIN only; anything else CRT_E_INVALID */
    double origin[3];
    double right[3], up[3], forward[3];  /* the caller's basis, used as given, never normalised */
    double extent_x, extent_y;   /* ORTHOGRAPHIC: half width / half height in world units, > 0;
                                    EQUIRECT: half horizontal / half vertical angle, (0, pi] / (0, pi/2];
                                    FISHEYE: angle from the axis at the frame's left-right / top-bottom edge,
                                    > 0, extent_x^2 + extent_y^2 <= pi^2; PINHOLE, CUBE: must be 0 */
    uint64_t batch_pixels;       /* 0: the most whole pixels whose scratch (76 B a record) stays <= 256 MiB.
                                    Sizes only: any value gives the same bits */
} crt_lens;                      /* 128 bytes */

/* The render's first stage, also callable on its own: the rays and LCG states of the whole frame,
 * num_samples records a pixel, record r = (row * image_w + col) * num_samples + (s - first_sample)
 * for sample s in [first_sample, first_sample + num_samples). Of cam, image_w, image_h and base_seed
 * are used for every kind (PINHOLE also reads origin, pixel00, the deltas and the defocus disk); the
 * rest is checked as in crt_render_lens_async. pi below is the double 3.141592653589793.
 *   The state starts as crt_sample_seed(base_seed, row * image_w + col, s).
 *   PINHOLE: the record of crt_camera_rays_async, byte for byte: with defocus_angle > 0, vx, vy =
 *     crt_rand_double(state, -1, 1) in that order until vx*vx + vy*vy + 0.0*0.0 < 1, then
 *     o = (origin + defocus_disk_x * vx) + defocus_disk_y * vy, else o = origin;
 *     uy = crt_rand_double(state, -0.5, 0.5), then ux likewise; per component
 *     centre = (pixel00 + pixel_delta_y * (double)row) + pixel_delta_x * (double)col,
 *     sample = (centre + pixel_delta_x * ux) + pixel_delta_y * uy,  d = sample - o.
 *     lens->origin, the basis and the extents are not used.
 *   Every other kind draws no defocus: uy = crt_rand_double(state, -0.5, 0.5), then ux likewise (the
 *     pixel_delta_y draw first, as above). With h_face = image_h and row_in_face = row, except for
 *     CUBE, where h_face = image_w, face = row / image_w and row_in_face = row % image_w:
 *       fx = ((double)col + 0.5) + ux,          fy = ((double)row_in_face + 0.5) + uy,
 *       a = fx * (2.0 / (double)image_w) - 1.0,  b = 1.0 - fy * (2.0 / (double)h_face).
 *     With R = right, U = up, F = forward, O = origin, per component:
 *     ORTHOGRAPHIC: o = (O + R * (a * extent_x)) + U * (b * extent_y),  d = F.
 *     EQUIRECT: phi = a * extent_x, theta = b * extent_y, o = O,
 *       d = (R * (cos(theta) * sin(phi)) + U * sin(theta)) + F * (cos(theta) * cos(phi)).
 *     FISHEYE: px = a * extent_x, py = b * extent_y, psi = sqrt(px * px + py * py),
 *       k = psi == 0 ? 1.0 : sin(psi) / psi, o = O,
 *       d = (R * (px * k) + U * (py * k)) + F * cos(psi).
 *     CUBE: u = a, v = -b; the local direction (x, y, z) of face 0..5 (the usual cube-map table, v
 *       pointing down the image):
 *         0 +X (1, -v, -u)   1 -X (-1, -v, u)   2 +Y (u, 1, v)
 *         3 -Y (u, -1, -v)   4 +Z (u, -v, 1)    5 -Z (-u, -v, -1)
 *       o = O,  d = (R * x + U * y) + F * z.
 *   sin, cos and sqrt are the device library's f64 functions (sqrt and the division IEEE); d is not
 *   normalised. d_rays[6r .. 6r + 5] (DEVICE) = {o, d}; d_states[r] (DEVICE) = the state after the
 *   draws: the path's state.
 * A generated ray outside crt_trace_async's contract (a non-finite component, e.g. from a NaN origin)
 * is a miss under crt_radiance_async's rule and sees the background.
 * CRT_E_INVALID as crt_render_lens_async's (samples_per_pixel is not read), and for
 * first_sample + num_samples > 2^32 - 1, more than 2^31 - 1 records, d_rays or d_states NULL.
 * num_samples == 0 is CRT_OK with no work. Enqueues on `stream`. */
int crt_lens_rays_async(int device, const crt_camera* cam, const crt_lens* lens, uint32_t first_sample,
                        uint32_t num_samples, double* d_rays, uint32_t* d_states, void* stream);

/* d_rgb: DEVICE memory on `device`, image_h * image_w * 3 doubles, the whole frame, row-major.
 * Of cam, image_w, image_h, samples_per_pixel, max_depth, background, t_min and base_seed are used
 * for every kind.
 * Paths: L_s = crt_radiance_async's output (cam's max_depth, background, t_min; lens->flags) for the
 * ray and state of crt_lens_rays_async(first_sample = 0, num_samples = samples_per_pixel).
 * Reduction, per pixel and channel, crt_render_async's: with L = crt_sample_chunk_len(spp), chunk c
 * is the sum of L_s for s = c * L .. min(spp, (c + 1) * L) - 1 in that order, starting from 0.0; the
 * chunk sums are added in chunk order; the result is multiplied by 1 / (double)spp. No
 * floating-point atomics are used. With kind PINHOLE the frame is crt_render_async's, bit for bit.
 * Batches: consecutive whole pixels in row-major order, batch_pixels of them (0: the most whose
 * scratch of 76 bytes a record stays at or under 256 MiB; never fewer than one pixel, never more than
 * 2^31 - 1 records), each generated, traced and reduced in order on `stream`, in a scratch buffer the
 * library keeps per device (grown on demand; a second call on the device while one is being enqueued
 * allocates its own and waits for its stream before freeing it). Nothing is carried between batches.
 * max_depth == 0 writes +0 everywhere with a memset and launches nothing. The scene must be resident
 * on `device` (CRT_E_NOT_UPLOADED). CRT_E_INVALID, checked before any device work (the message names
 * the rule): scene, cam, lens or d_rgb NULL; unknown kind; unknown flags; a component of right, up
 * or forward or an extent not finite (for PINHOLE too; the origin is not checked: a non-finite one
 * gives rays outside the query's contract, a frame of the background); an extent outside its range for the kind (see crt_lens); image_h != 6 * image_w for CUBE; image_w,
 * image_h or samples_per_pixel equal to 0; samples_per_pixel > 2^31 - 1; t_min outside [0, 2^100] or
 * NaN; a background component not finite. Dielectric decisions count into the scene's parity guard
 * as crt_radiance_async's do. One device a call, no defocus for the kinds other than PINHOLE. */
int crt_render_lens_async(const crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                          double* d_rgb, void* stream);

/* crt_render_lens_async for a HOST array, blocking: uploads the scene to `device` if it is not
 * resident, then the render on a stream of its own and one copy back. Same rules, same results
 * (the C++ drop-in's Camera::render_lens). */
int crt_render_lens(crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens, double* rgb);

/* ---- cube-map environments --------------------------------------------------------------------
 * What a path sees where it leaves the scene, in place of the constant background, for the
 * radiance, probe and lens calls (not for crt_render_async and its drivers, the lens renders in
 * passes or crt_lens_features_async: those keep the constant). The map has crt_render_lens_async's
 * CUBE layout, so a captured frame is an environment as it is. Every operation of the lookup is an
 * IEEE f64 + - * /, a comparison or a floor; nothing is fused. */
#define CRT_ENV_NEAREST  0u
#define CRT_ENV_BILINEAR 1u
typedef struct crt_env {
    const double* texels;  /* 6n rows x n columns x 3 doubles, row = face * n + row_in_face:
                              the frame crt_render_lens_async writes for CRT_LENS_CUBE with
                              image_w = n, image_h = 6 n. Device memory in the *_async entries. */
    uint32_t face_size;    /* n, 1 <= n <= 16384 */
    uint32_t filter;       /* CRT_ENV_NEAREST | CRT_ENV_BILINEAR */
    double right[3], up[3], forward[3];  /* used as given, never normalised (as crt_lens) */
} crt_env;                 /* 88 bytes */

/* E(d): the value of a path that ends in a miss on a segment with direction d, the path's own
 * (unnormalised) direction: the caller's for a first-segment miss, the scattered one otherwise.
 * With R = right, U = up, F = forward, n = face_size:
 *   1. x = (d0 * R0 + d1 * R1) + d2 * R2, y likewise with U, z with F.
 *   2. ax = |x|, ay = |y|, az = |z|, m = the largest of the three, NaN if any of them is NaN.
 *      If !(m > 0 && m < inf) (zero, NaN or infinite), E(d) = the call's constant background. Rays
 *      outside crt_trace_async's contract are shaded as misses, so they come here too.
 *   3. The face, ties in this order: ax >= ay && ax >= az: x > 0 ? 0 (+X) : 1 (-X); else ay >= az:
 *      y > 0 ? 2 (+Y) : 3 (-Y); else z > 0 ? 4 (+Z) : 5 (-Z).
 *   4. (u, v), the inverse of crt_lens_rays_async's CUBE table, each one division by m:
 *        +X: u = -z / m, v = -y / m     -X: u = z / m, v = -y / m     +Y: u = x / m, v = z / m
 *        -Y: u = x / m, v = -z / m      +Z: u = x / m, v = -y / m     -Z: u = -x / m, v = -y / m
 *   5. h = 0.5 * (double)n, formed once; fx = (u + 1.0) * h, fy = (v + 1.0) * h.
 *   6. NEAREST: col = clamp((int)floor(fx), 0, n - 1), row likewise from fy; E = the texel at row
 *      face * n + row, column col.
 *   7. BILINEAR: gx = fx - 0.5, x0 = floor(gx), wx = gx - x0, the same for y; the columns x0 and
 *      x0 + 1 and the rows y0 and y0 + 1 are each clamped to [0, n - 1] as integers, inside the face
 *      (no texel of another face is read); with cXY the texel at column X, row Y, per channel
 *        a = c00 + wx * (c10 - c00),  b = c01 + wx * (c11 - c01),  E = a + wy * (b - a).
 *      A map of equal finite texels gives that texel exactly.
 * The path's output is 0 + T * E(d) per channel, T its throughput, as it is 0 + T * background
 * without an environment. Floats are converted to integers only after the range check of step 2
 * and the indices are clamped as integers: no d reads outside the map. Texel values are not
 * inspected; a non-finite one propagates as the arithmetic above propagates it.
 *
 * The *_env entries are their namesakes with one more argument: same buffers, same rules, same
 * results for every path that does not end in a miss. CRT_E_INVALID in addition, checked with the
 * other rules before any device work (the message names the rule): env NULL; env->texels NULL;
 * face_size 0 or above 16384; an unknown filter; a component of right, up or forward not finite.
 * max_depth == 0 still writes +0 with a memset. env is read during the call only; the texels must
 * stay valid and unchanged until the enqueued work has run. */
int crt_radiance_env_async(const crt_scene* scene, int device, const double* d_rays, size_t n,
                           const uint32_t* d_states, const crt_radiance_params* params, const crt_env* env,
                           double* d_rgb, void* stream);
int crt_probes_env_async(const crt_scene* scene, int device, const double* d_points, const double* d_normals,
                         size_t n, const crt_probe_params* params, const crt_env* env, double* d_coeff,
                         void* stream);
int crt_render_lens_env_async(const crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                              const crt_env* env, double* d_rgb, void* stream);
/* crt_render_lens for a HOST array, blocking; env->texels is HOST memory here, uploaded for the call
 * and freed after it (the C++ drop-in's Camera::render_lens(world, lens, env)). */
int crt_render_lens_env(crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                        const crt_env* env, double* rgb);

/* ---- environments sampled by luminance: next-event estimation with MIS ----------------------
 * As above, a path finds the environment only by bouncing into it. A crt_env_sampler draws
 * directions from a distribution built on the map's luminance, and the *_env_sampled entries send a
 * shadow ray that way at every Lambertian bounce and combine it with the escape the scatter produces
 * by the balance heuristic. An addition to the ABI (no existing call changes, CRT_ABI_VERSION stays).
 * Tables are doubles; every operation below is an IEEE f64 + - * /, a sqrt, a comparison or a
 * floor; nothing is fused.
 *
 * crt_env_sampler_create blocks. It records *env (device texels, n = face_size, filter, basis; the
 * texels must stay valid and unchanged for the sampler's life) and builds on `device`, with rows
 * r = face * n + row_in_face, the map's own layout:
 *   Y = (0.2126 * r + 0.7152 * g) + 0.0722 * b, then Y = Y > 0 ? Y : 0 (NaN and negatives give 0);
 *   uc = ((double)col + 0.5) * (2.0 / (double)n) - 1.0, vc likewise from row_in_face,
 *   sc = (1.0 + uc * uc) + vc * vc,  w[r][col] = Y / (sc * sqrt(sc))   (luminance times the texel's
 *     solid angle up to the constant 4 / n^2);
 *   c[r][0] = 0.0 + w[r][0],  c[r][k] = c[r][k - 1] + w[r][k];
 *   m[0] = 0.0 + c[0][n - 1],  m[r] = m[r - 1] + c[r][n - 1],  W = m[6n - 1].
 * The sums are sequential in that order. CRT_E_INVALID (the message names the rule): env or out
 * NULL; crt_env's rules (above); face_size above 2048; a basis whose Gram matrix (the nine dot
 * products of right, up, forward, each (a0 b0 + a1 b1) + a2 b2) differs from the identity by more
 * than 1e-9 in any entry (the densities below are solid-angle densities only for an orthonormal
 * basis); these are checked before any device work; then !(W > 0 && W < inf), read back after the
 * build (an all-black, NaN or overflowing map).
 * crt_env_sampler_view gives the recorded crt_env, the device pointers of w (6n x n), c (6n x n)
 * and m (6n) and W. crt_env_sampler_free(NULL) is CRT_OK.
 *
 * env_pdf(d), the solid-angle density of d: steps 1 to 5 of E(d). If d has no major axis (step 2),
 *   env_pdf = 0. Else col, row as in step 6, whatever the filter; s = (1.0 + u * u) + v * v,
 *   hh = h * h,  env_pdf = ((w[face * n + row][col] / W) * hh) * (s * sqrt(s)).
 * env_sample(xi1, xi2, xi3, xi4): r = the number of rows with m[r] <= xi1 * W, clamped to 6n - 1;
 *   k = the number of columns with c[r][k] <= xi2 * c[r][n - 1], clamped to n - 1; face = r / n,
 *   row_in_face = r % n; fx = (double)k + xi3, fy = (double)row_in_face + xi4,
 *   u = fx * (2.0 / (double)n) - 1.0, v likewise from fy; (x, y, z) from crt_lens_rays_async's CUBE
 *   table; d_s = (R * x + U * y) + F * z per component.
 *
 * The estimator is crt_radiance_env_async's integrator with these additions. A path carries acc,
 * +0 per channel at its start, and pb, the previous bounce's solid-angle density: "none" at the
 * start and after a Metal or Dielectric bounce. pi is the double 3.141592653589793; dot products
 * are (a0 b0 + a1 b1) + a2 b2.
 *   Light hit: acc = acc + T * emit, the path ends.
 *   Lambertian bounce, after the material's own draws, the throughput multiply and the depth
 *   decrement, if depth left > 0: xi1..xi4 = crt_rand_double(state, 0, 1) in that order (always
 *     drawn); d_s = env_sample(xi); c_s = (n . d_s) / sqrt(d_s . d_s), n the hit normal facing the
 *     ray; pb_s = c_s / pi; pe_s = env_pdf(d_s). If c_s > 0 && pe_s > 0, the segment from the hit
 *     point along d_s over (t_min, +inf) is traced, and any hit means occluded; if it is free,
 *     f = pb_s / (pe_s + pb_s), e = E(d_s), acc = acc + (T * e) * f per channel. Then
 *     pb = ((n . nd) / sqrt(nd . nd)) / pi for the scattered direction nd (the nd = n fallback
 *     included).
 *   Metal or Dielectric bounce: pb = none.
 *   Escape along d: e = E(d); f = 1.0 if pb is none, else pe = env_pdf(d) and
 *     f = (pe + pb) > 0 ? pb / (pe + pb) : 0.0; acc = acc + (T * e) * f per channel, the path ends.
 *   The output is acc: absorbed paths and paths out of depth write what they gathered.
 * A path with no Lambertian bounce, and every path with max_depth == 1, gets
 * crt_radiance_env_async's bytes. Rays the query contract refuses stay first-segment misses with
 * f = 1. Neither the grid nor the route (CRT_RADIANCE_PLAIN) changes a bit.
 *
 * The *_env_sampled entries are the *_env entries with the sampler in place of the environment, whose
 * recorded copy is used: same buffers, same rules. CRT_E_INVALID in addition, before any device
 * work: sampler NULL; a sampler built on another device. max_depth == 0 is still a memset. The
 * probes' and the lens frames' first segments have pb = none. */
typedef struct crt_env_sampler crt_env_sampler;
struct crt_env_sampler_view {      /* the entry below has the same name: no typedef, say `struct` */
    crt_env env;                    /* as recorded by create */
    const double *w, *c, *m;        /* DEVICE: 6n x n, 6n x n, 6n doubles */
    double W;
};                                  /* 120 bytes */
int crt_env_sampler_create(int device, const crt_env* env, crt_env_sampler** out);
int crt_env_sampler_free(crt_env_sampler* sampler);
int crt_env_sampler_view(const crt_env_sampler* sampler, struct crt_env_sampler_view* out);
int crt_radiance_env_sampled_async(const crt_scene* scene, int device, const double* d_rays, size_t n,
                                   const uint32_t* d_states, const crt_radiance_params* params,
                                   const crt_env_sampler* sampler, double* d_rgb, void* stream);
int crt_probes_env_sampled_async(const crt_scene* scene, int device, const double* d_points,
                                 const double* d_normals, size_t n, const crt_probe_params* params,
                                 const crt_env_sampler* sampler, double* d_coeff, void* stream);
int crt_render_lens_env_sampled_async(const crt_scene* scene, int device, const crt_camera* cam,
                                      const crt_lens* lens, const crt_env_sampler* sampler, double* d_rgb,
                                      void* stream);
/* crt_render_lens_env with luminance sampling: env->texels is HOST memory; the call uploads it,
 * builds a sampler, renders, and frees both. crt_env_sampler_create's rules hold. */
int crt_render_lens_env_sampled(crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                                const crt_env* env, double* rgb);

/* ---- the scene's own lights sampled: next-event estimation with MIS --------------------------
 * In the radiance, probe and lens calls a path finds a DiffuseLight only by bouncing into it. A
 * crt_light_sampler draws points on the scene's emitting primitives, and the *_lights entries send a
 * shadow ray to one at every Lambertian bounce and combine it with the bounce's own light hits by
 * the balance heuristic. An addition to the ABI (no existing call changes, CRT_ABI_VERSION stays).
 * Tables are doubles; every operation below is an IEEE f64 + - * /, a sqrt or a comparison; nothing
 * is fused; dot products are (a0 b0 + a1 b1) + a2 b2; pi is the double 3.141592653589793.
 *
 * crt_light_sampler_create blocks. The scene must be resident on `device` (crt_scene_upload). The
 * lights are the flattened primitives whose material is CRT_DIFFUSE_LIGHT (a Box gives its six
 * parallelograms), listed in ascending flattened primitive index, the index crt_hit.prim reports,
 * so a pick does not depend on the BVH parameters. For light i:
 *   e = color * param per channel;  Y = (0.2126 * e0 + 0.7152 * e1) + 0.0722 * e2, then
 *   Y = Y > 0 ? Y : 0 (NaN and negatives give 0);
 *   A = sqrt(cr . cr) with cr = s1 x s2 = (s1y s2z - s1z s2y, s1z s2x - s1x s2z, s1x s2y - s1y s2x)
 *   for a parallelogram, A = (4.0 * pi) * (r * r) for a sphere;
 *   w[i] = Y * A;  cdf[0] = 0.0 + w[0],  cdf[i] = cdf[i - 1] + w[i];  W = cdf[L - 1].
 * The sums are sequential in that order. Beside them the sampler keeps the lights' slot references
 * (what a hit's ref is: the slot's index in its kind's array, the high bit set for a parallelogram)
 * sorted ascending with w in the same order, so a hit finds its light's w by binary search.
 * CRT_E_INVALID (the message names the rule): scene or out NULL; a scene not resident on `device`;
 * a scene with no light; !(W > 0 && W < inf).
 * crt_light_sampler_view gives L, the device pointers and W. crt_light_sampler_free(NULL) is CRT_OK.
 * The sampler reads the scene's device copy at every call: free it before the scene.
 *
 * light_pick(xi1) = the number of entries with cdf[k] <= xi1 * W, clamped to L - 1 (the clamp covers
 *   the largest rnd_01 value, which exceeds 1, and NaN).
 * light_point(i, state): parallelogram: xi2, xi3 = crt_rand_double(state, 0, 1) in that order,
 *   p = (v + s1 * xi2) + s2 * xi3 per component. Sphere: u = random_unit_vector(state) (the rejection
 *   loop of the Lambertian scatter: its draw count varies), p = c + u * |r|. Neither uses sin or cos:
 *   that is why spheres are sampled by area over the whole surface and not by the cone they subtend.
 * light_pdf, the solid-angle density with which the sampler produces the point where a ray (o, d)
 *   actually hit light j at t, with the hit's normal n (either side) and front flag, the same
 *   function for shadow hits and bounce hits: v = d * t, vv = v . v,
 *   pl = ((w_j / W) / A_j) * ((vv * sqrt(vv)) / |n . v|); pl = 0 where w_j is not > 0; for a sphere
 *   pl = 0 unless the hit is on the geometric outside, front == (r > 0) (hollow spheres have r < 0).
 *
 * The estimator is crt_radiance_async's integrator with a constant background and these additions.
 * A path carries acc, +0 per channel at its start, and pb, "none" at its start and after a Metal or
 * Dielectric bounce.
 *   Light hit on an ordinary segment: f = 1.0 if pb is none, else pl = light_pdf(hit) and
 *     f = (pl + pb) > 0 ? pb / (pl + pb) : 0.0; acc = acc + (T * emit) * f, the path ends.
 *   Lambertian bounce, after the material's own draws, the throughput multiply and the depth
 *   decrement, if depth left > 0: xi1 = crt_rand_double(state, 0, 1) (always drawn);
 *     i = light_pick(xi1); p_l = light_point(i) (its draws are always made); d_s = p_l - o, o the hit
 *     point; c_s = (n . d_s) / sqrt(d_s . d_s), n the hit normal facing the ray;
 *     pb = ((n . nd) / sqrt(nd . nd)) / pi for the scattered direction nd. No shadow ray is sent if
 *     !(c_s > 0) (NaN and a zero-length d_s fall here) or, for a sphere, if !(u . d_s < 0) (a point
 *     on the far side, which the near side hides). Otherwise the segment from o along d_s over
 *     (t_min, +inf) is traced as any segment is, closest hit. It contributes only if it finds a hit
 *     whose ref is light i's slot: then pl = light_pdf(that hit), pb_s = c_s / pi, and if
 *     pl > 0 && pl < inf, acc = acc + (T * emit_i) * (pb_s / (pl + pb_s)). Any other hit, or none,
 *     adds nothing (a nearer light k that hides light i drops the sample; the bounce strategy's hit
 *     on k is weighted with k's own density, so the two weights sum to 1 wherever a contribution is
 *     not zero). The path then goes on along nd.
 *   Metal or Dielectric bounce: pb = none.
 *   Escape: acc = acc + T * background, no weight (nothing samples the background).
 *   The output is acc: absorbed paths and paths out of depth write what they gathered.
 * A path with no Lambertian bounce, and every path with max_depth == 1, gets crt_radiance_async's
 * bytes. Rays the query contract refuses stay first-segment misses. Neither the grid nor the route
 * (CRT_RADIANCE_PLAIN) changes a bit.
 *
 * The *_lights entries are crt_radiance_async, crt_probes_async, crt_render_lens_async and
 * crt_render_lens with the sampler as one more argument: same buffers, same rules. CRT_E_INVALID in
 * addition, before any device work: lights NULL; a sampler of another scene; a sampler built on
 * another device. max_depth == 0 is still a memset. The probes' and the lens frames' first segments
 * have pb = none. Lights together with an environment: the *_lit entries (below). */
typedef struct crt_light_sampler crt_light_sampler;
struct crt_light_sampler_view {    /* the entry below has the same name: no typedef, say `struct` */
    uint32_t num_lights;            /* L */
    int32_t device;
    const uint32_t *prim, *ref;     /* DEVICE, pick order: flattened primitive index, slot reference */
    const uint32_t* sorted_ref;     /* DEVICE: the slot references ascending */
    const double *w, *cdf;          /* DEVICE, pick order */
    const double* sorted_w;         /* DEVICE: w in sorted_ref's order */
    double W;
};                                  /* 64 bytes */
int crt_light_sampler_create(const crt_scene* scene, int device, crt_light_sampler** out);
int crt_light_sampler_free(crt_light_sampler* lights);
int crt_light_sampler_view(const crt_light_sampler* lights, struct crt_light_sampler_view* out);
int crt_radiance_lights_async(const crt_scene* scene, int device, const double* d_rays, size_t n,
                              const uint32_t* d_states, const crt_radiance_params* params,
                              const crt_light_sampler* lights, double* d_rgb, void* stream);
int crt_probes_lights_async(const crt_scene* scene, int device, const double* d_points,
                            const double* d_normals, size_t n, const crt_probe_params* params,
                            const crt_light_sampler* lights, double* d_coeff, void* stream);
int crt_render_lens_lights_async(const crt_scene* scene, int device, const crt_camera* cam,
                                 const crt_lens* lens, const crt_light_sampler* lights, double* d_rgb,
                                 void* stream);
/* crt_render_lens with the lights sampled: uploads the scene if needed, builds a sampler, renders,
 * frees it. crt_light_sampler_create's rules hold. */
int crt_render_lens_lights(crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens, double* rgb);

/* ---- lens renders in passes ------------------------------------------------------------------
 * A lens render cut into passes, with the state the camera-agnostic calls read: crt_noise_estimate,
 * crt_adaptive_update, crt_pixel_variance_async and crt_denoise_async take d_sum, d_noise, block
 * words and crt_feature records from these calls exactly as from the reference camera's.
 *
 * One pass: samples [first_sample, first_sample + num_samples) of a job of cam->samples_per_pixel
 * samples (that total fixes L = crt_sample_chunk_len(spp) and the seeds), over the whole frame; no
 * tiling. d_sum (image_h * image_w * 3), d_noise (image_h * image_w * 2, or NULL) and d_rgb (as
 * d_sum, or NULL) are DEVICE buffers of the whole frame, row-major.
 * Rules: crt_render_lens_async's on scene, cam and lens, then crt_render_pass_async's on
 * first_sample, num_samples and d_sum; at most 2^31 - 1 pixels; with d_blocks, first_sample +
 * num_samples < 2^31. All are checked before any device work (CRT_E_INVALID, the message names the
 * rule).
 * Paths: the ray and state of sample s of pixel p are crt_lens_rays_async's; L_s is
 * crt_radiance_async's output for them, as in crt_render_lens_async.
 * Accumulation, per pixel and channel, crt_render_pass_async's: chunk c of the pass is the sum of
 * its L_s (s = first_sample + c * L .. min(first_sample + num_samples, first_sample + (c + 1) * L) - 1)
 * in sample order, starting from 0.0. A pass with first_sample == 0 starts the running sum from
 * chunk 0's sum (not from 0.0 plus it) and overwrites d_sum and d_noise; any other pass starts from
 * the stored d_sum. The chunk sums are added in chunk order. With d_noise: for every chunk of the
 * pass that has L samples, in chunk order, y = (r + g) + b of the chunk's sum, t = t + y and
 * q = q + y * y, where t and q start from 0 in a pass with first_sample == 0 and from the stored
 * values otherwise; a ragged last chunk is left out. With d_rgb: the frame so far, sum *
 * (1 / (double)(first_sample + num_samples)). No floating-point atomics are used; the bits depend
 * on neither the grid nor lens->batch_pixels nor the radiance route (CRT_RADIANCE_PLAIN in
 * lens->flags) nor active_hint. Passes issued once each, in increasing order, end in
 * crt_render_lens_async's frame bit for bit; with kind PINHOLE every pass leaves
 * crt_render_pass_async's d_sum, d_noise and d_rgb.
 * d_blocks (DEVICE, crt_block_count(image_w, image_h) words, or NULL: every pixel) makes it a masked
 * pass over the frame's 16 x 4 blocks: only the blocks with d_blocks[b] == first_sample are
 * generated, traced and accumulated, and their words become first_sample + num_samples. A skipped
 * block gets what crt_render_pass_masked_async gives a skipped block: with first_sample > 0, d_sum
 * and d_noise are left alone and d_rgb gets sum * (1 / (double)n) for the block's own count n (0
 * when n = 0); with first_sample == 0 its pixels' d_sum, d_noise and d_rgb are written 0.
 * Stopped blocks cost no rays: the active blocks' pixels are compacted into a list on the device
 * (its order affects no bit) and only they are generated and traced. The radiance query needs its
 * record count on the host, so WITH d_blocks THE CALL WAITS FOR `stream` ONCE to read the number of
 * active pixels (4 bytes); active_hint is accepted for symmetry with crt_render_pass_masked_async
 * and sizes nothing. Without d_blocks the call only enqueues on `stream`.
 * Batches: whole pixels, lens->batch_pixels of them (0: as crt_render_lens_async's, for num_samples
 * records a pixel), each generated, traced and accumulated in order, in crt_render_lens_async's
 * scratch buffer. max_depth == 0: every L_s is +0; the pass makes the additions above with +0 and launches
 * no trace. The scene must be resident on `device` (CRT_E_NOT_UPLOADED). */
int crt_render_lens_pass_async(const crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                               uint32_t first_sample, uint32_t num_samples, double* d_sum, double* d_noise,
                               double* d_rgb, uint32_t* d_blocks, uint32_t active_hint, void* stream);

/* The ray through the centre of every pixel, no draws: d_rays (DEVICE, image_h * image_w * 6
 * doubles) record row * image_w + col = {o, d}.
 *   PINHOLE: crt_render_features_async's ray: centre = (pixel00 + pixel_delta_y * (double)row) +
 *     pixel_delta_x * (double)col, o = origin, d = centre - origin (the random terms left out, not
 *     multiplied by zero).
 *   Every other kind: crt_lens_rays_async's expressions with fx = (double)col + 0.5 and
 *     fy = (double)row_in_face + 0.5 (ux and uy left out), a and b and the kind's o and d unchanged.
 * crt_lens_rays_async's rules on cam and lens; d_rays not NULL; at most 2^31 - 1 pixels. Enqueued. */
int crt_lens_centre_rays_async(int device, const crt_camera* cam, const crt_lens* lens, double* d_rays, void* stream);

/* First-hit features through a lens: d_feat (DEVICE, image_h * image_w records, row-major). The
 * centre ray of crt_lens_centre_rays_async is traced over (cam->t_min, +inf) as crt_trace_async
 * traces it; t, point, normal, prim and material are the crt_hit's, albedo and the miss record are as
 * crt_feature defines them. For PINHOLE the records equal crt_render_features_async's byte for byte.
 * ORTHOGRAPHIC's d = forward is not normalised, so its t is in units of |forward|. The parity guard
 * is not touched. Rays and hits (120 bytes a pixel) come from the pass pool; the first closest-hit
 * query for a scene and device uploads a table, blocking, after that the call only enqueues. */
int crt_lens_features_async(const crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                            crt_feature* d_feat, void* stream);

/* Blocking lens render in passes on one device: crt_render_adaptive's loop with the lens pass in
 * place of the masked pass. Uploads the scene if it is not resident.
 *   adaptive == NULL: plain passes of a tenth of the job each (at least one chunk), no previews; fn
 *     gets active_blocks = total_blocks while samples remain, 0 after the last pass.
 *   adaptive != NULL: crt_render_adaptive's rules for *adaptive (flags 0 or CRT_PROGRESS_PREVIEW);
 *     after every masked pass crt_adaptive_update, unchanged.
 *   The loop ends when no block is active, all samples are done, or fn (may be NULL) returns non-zero.
 *   denoise != NULL (crt_denoise_async's rules): crt_lens_features_async once, then
 *     crt_pixel_variance_async (with the block words when adaptive) and crt_denoise_async, unchanged;
 *     h_rgb is the denoised frame and h_noisy (HOST, or NULL) the unfiltered one. A CUBE frame's six
 *     faces are contiguous image_w x image_w sub-frames and are filtered one at a time (six
 *     crt_denoise_async calls), so no tap crosses from a face into an unrelated one.
 *   denoise == NULL: h_rgb is the unfiltered frame: every pixel's sum times 1 / its block's own
 *     count; h_noisy must be NULL (CRT_E_INVALID).
 *   With CRT_PROGRESS_PREVIEW and fn the frames are produced (and filtered) before every call of fn,
 *   which receives the caller's h_noisy and h_rgb; else once at the end, and fn receives NULL for both.
 *   h_block_samples (or NULL) and *samples_rendered (or NULL) as crt_render_denoised_devices'.
 * Limits: EQUIRECT taps do not wrap at the +-extent_x seam; ORTHOGRAPHIC's t is in units of |forward|.
 * Every rule is checked before any device work. */
int crt_render_lens_passes(crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                           const crt_adaptive_params* adaptive, const crt_denoise_params* denoise,
                           crt_denoised_fn fn, void* user, double* h_noisy, double* h_rgb,
                           uint32_t* h_block_samples, uint64_t* samples_rendered);

/* ---- an environment and the scene's lights together, also in passes ---------------------------
 * The two next-event estimators above under one argument, and the lens passes with it. An addition to
 * the ABI (no existing call changes, CRT_ABI_VERSION stays). Every operation is an IEEE f64 + - * /,
 * a sqrt or a comparison; nothing is fused; dot products are (a0 b0 + a1 b1) + a2 b2; pi is the
 * double 3.141592653589793. env_sample, env_pdf, light_pick, light_point and light_pdf are the
 * functions of the two sections above, unchanged.
 *
 * A lighting is two independent choices: the environment (none: the constant background; a plain
 * crt_env; or a crt_env_sampler) and the lights (none, or a crt_light_sampler). A path carries acc,
 * +0 per channel at its start, and pb, "none" at its start and after a Metal or Dielectric bounce.
 *   A segment ends on a DiffuseLight: without a light sampler acc = acc + T * emit. With one, f = 1.0
 *     if pb is none, else pl = light_pdf(hit) and f = (pl + pb) > 0 ? pb / (pl + pb) : 0.0;
 *     acc = acc + (T * emit) * f. The path ends.
 *   A segment escapes along d: with no environment acc = acc + T * background; with a plain one
 *     acc = acc + T * E(d); with a sampler f = 1.0 if pb is none, else pe = env_pdf(d) and
 *     f = (pe + pb) > 0 ? pb / (pe + pb) : 0.0; acc = acc + (T * E(d)) * f. The path ends.
 *   Metal or Dielectric bounce: pb = none.
 *   Lambertian bounce at o with the normal n facing the ray, after the material's own draws, the
 *   throughput multiply and the depth decrement, if depth left > 0, in this order:
 *     1. With an env sampler: xi1..xi4 = crt_rand_double(state, 0, 1) (always drawn);
 *        d_e = env_sample(xi); c_e = (n . d_e) / sqrt(d_e . d_e); pe = env_pdf(d_e);
 *        ray_e = c_e > 0 && pe > 0.
 *     2. With a light sampler: xi1 (always drawn); i = light_pick(xi1); p_l = light_point(i) (its
 *        draws are always made); d_l = p_l - o; c_l = (n . d_l) / sqrt(d_l . d_l);
 *        ray_l = c_l > 0 && (light i is a parallelogram || u . d_l < 0).
 *     3. pb = ((n . nd) / sqrt(nd . nd)) / pi for the scattered direction nd.
 *     4. If ray_e: the segment from o along d_e over (t_min, +inf) is traced; any hit occludes. If it
 *        is free, pb_e = c_e / pi and acc = acc + (T * E(d_e)) * (pb_e / (pe + pb_e)).
 *     5. If ray_l: the segment along d_l is traced, closest hit. It counts only if the hit's ref is
 *        light i's slot: then pl = light_pdf(that hit), pb_l = c_l / pi, and if pl > 0 && pl < inf,
 *        acc = acc + (T * emit_i) * (pb_l / (pl + pb_l)).
 *     6. The path goes on along nd.
 *   The output is acc: absorbed paths and paths out of depth write what they gathered.
 * All of step 1's draws precede step 2's, and acc receives step 4's term before step 5's. No segment
 * draws a number, so an implementation may make step 2's draws after step 4's segment has returned
 * (to hold less across it): the values are the same.
 * Each sample is weighted against pb alone, and that is not an omission. A direction from o either
 * ends on a primitive or leaves the scene, so the map and the lights are disjoint emitters: the map's
 * sampler never produces a contribution a light could also have produced, nor the reverse. On each
 * emitter exactly two strategies compete, that emitter's own sampler and the bounce, and the balance
 * heuristic over those two is complete: wherever a contribution is not zero, the two weights sum to 1.
 * Consequences: a lighting with only a sampler gives crt_radiance_env_sampled_async's bytes, with only
 * lights crt_radiance_lights_async's, with only a plain env crt_radiance_env_async's, with nothing
 * crt_radiance_async's (the entries below forward to the same launches). Every path without a
 * Lambertian bounce, and every path with max_depth == 1, gets crt_radiance_env_async's bytes, or
 * crt_radiance_async's without an environment. Rays the query contract refuses stay first-segment
 * misses with f = 1. Neither the grid nor the route (CRT_RADIANCE_PLAIN) changes a bit.
 *
 * The *_lit entries are crt_radiance_async, crt_probes_async, crt_render_lens_async and
 * crt_render_lens_pass_async with the lighting as one more argument: same buffers, same rules.
 * CRT_E_INVALID in addition, before any device work (the message names the rule): lighting NULL; env
 * and sampler both set; reserved != 0; for the members given, the rules of the *_env entries
 * (crt_env's), of the *_env_sampled entries (a sampler built on another device) and of the *_lights
 * entries (a sampler of another scene or device). max_depth == 0 is still a memset. The probes' and
 * the lens frames' first segments have pb = none.
 * crt_render_lens_pass_lit_async is crt_render_lens_pass_async in every rule, buffer and bit, with
 * the lit estimator's output as L_s: accumulation, masks, the active-pixel list, the one stream wait
 * with d_blocks and the batches are untouched. crt_lens_features_async is unchanged under a lighting:
 * a miss keeps the constant background as its albedo. */
typedef struct crt_lighting {          /* 32 bytes */
    const crt_env* env;                /* plain environment (DEVICE texels), or NULL */
    const crt_env_sampler* sampler;    /* luminance-sampled environment, or NULL; not with env */
    const crt_light_sampler* lights;   /* the scene's lights sampled, or NULL */
    uint64_t reserved;                 /* 0 */
} crt_lighting;
int crt_radiance_lit_async(const crt_scene* scene, int device, const double* d_rays, size_t n,
                           const uint32_t* d_states, const crt_radiance_params* params,
                           const crt_lighting* lighting, double* d_rgb, void* stream);
int crt_probes_lit_async(const crt_scene* scene, int device, const double* d_points, const double* d_normals,
                         size_t n, const crt_probe_params* params, const crt_lighting* lighting,
                         double* d_coeff, void* stream);
int crt_render_lens_lit_async(const crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                              const crt_lighting* lighting, double* d_rgb, void* stream);
int crt_render_lens_pass_lit_async(const crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                                   const crt_lighting* lighting, uint32_t first_sample, uint32_t num_samples,
                                   double* d_sum, double* d_noise, double* d_rgb, uint32_t* d_blocks,
                                   uint32_t active_hint, void* stream);
/* Blocking, host arrays: crt_render_lens and crt_render_lens_passes under a lighting made for the
 * call. env is NULL or has its texels in HOST memory (uploaded once, freed at the end); importance
 * and lights are 0 or 1: importance builds a crt_env_sampler on the uploaded texels
 * (crt_env_sampler_create's rules; CRT_E_INVALID without env), lights a crt_light_sampler of the
 * uploaded scene (crt_light_sampler_create's rules). crt_render_lens_passes_lit builds both once,
 * before the first pass, and frees them at the end; its loop is crt_render_lens_passes'. */
int crt_render_lens_lit(crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                        const crt_env* env, int importance, int lights, double* rgb);
int crt_render_lens_passes_lit(crt_scene* scene, int device, const crt_camera* cam, const crt_lens* lens,
                               const crt_env* env, int importance, int lights,
                               const crt_adaptive_params* adaptive, const crt_denoise_params* denoise,
                               crt_denoised_fn fn, void* user, double* h_noisy, double* h_rgb,
                               uint32_t* h_block_samples, uint64_t* samples_rendered);

/* The integers Image::send_as_ppm prints (image.h:38-56; RGB::as_string rgb.h:99-115 with its
 * defaults: Reinhard tone map by luminance, gamma 2, static_cast<int>(255.999999 * v)) for the
 * n-pixel frame d_rgb (device memory on `device`, row-major RGB f64, e.g. crt_render_async's
 * output), computed on the GPU; h_values (host, 3n int32) receives them, identical to the
 * x86-64 reference build's (NaN / out of range -> INT_MIN). Synchronous on `stream`. */
int crt_ppm_values(int device, const double* d_rgb, size_t n, int32_t* h_values, void* stream);

/* Writes w x h pixel values (3 per pixel) as Image::send_as_ppm does: "P3\nw h\n255\n", then
 * one "r g b\n" line per pixel, rows top to bottom. */
int crt_ppm_write(const char* path, uint32_t w, uint32_t h, const int32_t* values);

/* Parity guard of the renders of `scene` on `device` since its upload (or the last reset):
 * *schlick_undecided = Dielectric reflect-or-refract decisions (material.h:199-210) whose branch
 * would differ for a pow(1 - cos, 5) one ulp away from the kernel's correctly rounded value
 * (cpp_raytracer_amd/csrc/crt_schlick.h). glibc's pow, which the reference calls, is within one
 * ulp but not correctly rounded, so a render during which this stays 0 took every such branch as
 * the reference does. Synchronizes the device; reset != 0 zeroes the count. */
int crt_render_guard(crt_scene* scene, int device, uint64_t* schlick_undecided, int reset);

/* ---- launch plans ---------------------------------------------------------------------- */
/* What the host would decide for a launch of one of the three scene kernels, from the scene's size
 * alone: the class, the stack entry width, the instance and the LDS layout. Host only: no device is
 * touched and nothing is uploaded (a host-built scene that has not been uploaded yet is staged on
 * the host, as its first upload would). The values come from the code the launches run (the layout
 * steps and the launchers' own additions), and the CRT_* switches (CRT_NO_LDS_SCENE,
 * CRT_FORCE_GSTACK, CRT_NO_LDS_TOP, CRT_FOUR_WAVES, CRT_TRACE_FAST, CRT_F64_*, CRT_GENERIC_QUADS)
 * are read when the plan is asked, where a launch reads the last four when the scene is uploaded.
 * TRACE and RADIANCE plans are those of a query with 0 <= t_min <= 2^100 and no PLAIN flag.
 * An addition to the ABI (no existing call changes, CRT_ABI_VERSION stays): `reserved` words are
 * zero and later fields take their place. */
enum { CRT_PLAN_RENDER = 0, CRT_PLAN_TRACE = 1, CRT_PLAN_RADIANCE = 2 };
enum { CRT_PLAN_LDS_SCENE = 0, CRT_PLAN_LDS_STACK = 1, CRT_PLAN_HBM_STACK = 2 };
#define CRT_PLAN_ABSENT 0xffffffffu /* an lds_* region the instance does not have */
typedef struct crt_launch_plan_info {
    uint32_t kernel;        /* CRT_PLAN_RENDER / TRACE / RADIANCE                              */
    uint32_t klass;         /* CRT_PLAN_LDS_SCENE: the scene and the stack in LDS; LDS_STACK: the
                             * top of the node array and the stack; HBM_STACK: the top alone     */
    uint32_t entry_bytes;   /* stack entry width: 2 or 4                                       */
    uint32_t five_waves;    /* render: the five-waves-per-SIMD instance                         */
    uint32_t prim_mode;     /* 0 sphere-only, 1 general, 2 flat parallelograms                  */
    uint32_t plain_route;   /* trace: an LDS-scene launch takes the plain loop (no dynamic LDS)
                             * unless CRT_TRACE_FAST is set; the layout is the fast instance's    */
    uint32_t depth;         /* BVH levels: the stack holds levels 0..depth                      */
    uint32_t block;         /* threads per block                                                */
    uint64_t num_nodes;     /* device nodes, the pad and the sentinel included                  */
    uint32_t stack_bytes, level, sentinel;
    uint32_t hbm_stack_levels; /* HBM_STACK: levels allocated per lane (3 below level 0), else 0 */
    /* dev::Work's layout: byte offsets and 16-byte padded sizes; the scene regions are meaningful
     * for LDS_SCENE only, lds_stack for LDS_SCENE and LDS_STACK */
    uint32_t lds_nodes, lds_refs, lds_spheres, lds_quads, lds_quadf, lds_sph64, lds_stack;
    uint32_t bytes_nodes, bytes_refs, bytes_spheres, bytes_quads, bytes_quadf, bytes_sph64;
    uint32_t ntop, all_nodes; /* LDS_STACK, HBM_STACK: bytes of f32 nodes staged at offset 0 / in all */
    /* the launchers' additions (CRT_PLAN_ABSENT: none) and their sizes */
    uint32_t lds_cam, lds_acc, lds_inv64;
    uint32_t bytes_cam, bytes_acc, bytes_inv64;
    uint32_t total_lds;     /* the dynamic LDS the launch requests                              */
    uint32_t budget;        /* the budget the class was admitted under                          */
    uint32_t spheres_f32, quads_f32, quads_flat, f32_ok; /* the instance's f32 flags            */
    uint32_t reserved[9];
} crt_launch_plan_info; /* 200 bytes */
int crt_launch_plan(const crt_scene* scene, uint32_t kernel, crt_launch_plan_info* out);

/* ---- the stackless walk's miss links ----------------------------------------------------- */
/* The five-wave LDS-scene render instances walk the BVH without a stack: a ray's DFS order is
 * fixed by the signs of its direction (its octant: bit k set when d[k] < 0), so the node a pop
 * would return is a function of (node, octant), tabulated once per scene. Additions to the ABI (no
 * existing call changes, CRT_ABI_VERSION stays).
 * crt_walk_links: the table of `scene` over its device-order nodes (the pad and the sentinel
 * included): 8 uint16 entries a node, entry [node * 8 + octant] = the reference (node index * 32)
 * of the node the walk continues at when it does not descend from `node`. It is the table stored
 * with the scene (built and validated once), the bytes every device copy uploads. Host only for a
 * host-built scene; a scene built on a device got it from that device's nodes at its creation.
 * *num_nodes = the nodes of the table, 0 when the scene has none (its references do not fit 16
 * bits, or the table did not validate); `links` may be null to ask for the size, else `capacity`
 * (entries) must be at least 8 * *num_nodes.
 * crt_walk_links_validate: the check every upload runs, on a caller's table for `scene`: *ok = 1
 * when under each octant every link is the node that follows the node's subtree in that octant's
 * DFS order and following links from any node reaches the sentinel within num_nodes steps.
 * crt_last_walk: the walk the last render launch on `device` took for `scene`
 * (crt_render_async, its pass forms, crt_render_count, the blocking renders): CRT_WALK_NONE before
 * the first one. A diagnostic, not synchronized: with renders of one scene copy from several threads
 * it is one of theirs. CRT_NO_LINK_WALK=1, read at each launch, keeps every launch on the stack walk. */
enum { CRT_WALK_NONE = 0, CRT_WALK_STACK = 1, CRT_WALK_LINKS = 2 };
int crt_walk_links(crt_scene* scene, uint16_t* links, size_t capacity, size_t* num_nodes);
int crt_walk_links_validate(crt_scene* scene, const uint16_t* links, size_t entries, int* ok);
int crt_last_walk(const crt_scene* scene, int device, uint32_t* walk);

#ifdef __cplusplus
}
#endif

#endif /* CRT_RENDER_H */
