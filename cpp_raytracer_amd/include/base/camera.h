// Drop-in for the reference's base/camera.h. Same fluent setters and render() entry points;
// render runs the per-pixel / per-sample loop on the MI355X GPUs of this process through the C ABI
// (crt_render: rows dealt to every visible device in 4-row blocks, tiles gathered to the host).
// There is no CPU fallback: without a GPU render prints the reason and exits, as the reference does
// on its own errors.
//
// RNG: the reference seeds one LCG per OpenMP thread (rand_util.h:106); here each (pixel, sample)
// gets its own state crt_sample_seed(base, pixel, sample), with base = one next_seed() of
// SeedSeqGenerator per render, so output does not depend on scheduling or device count.
#ifndef CAMERA_H
#define CAMERA_H

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <numbers>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "acceleration/bvh.h"
#include "math/ray3d.h"
#include "util/image.h"
#include "util/progressbar.h"

// Extension (not in the reference): the knobs of Camera::render_denoised (crt_denoise_params).
struct DenoiseOptions {
    unsigned iterations = 5;        // a-trous iterations: steps 1, 2, 4, ... (1..8)
    unsigned normal_squarings = 7;  // normal weight = max(0, n_p . n_q)^(2^this) (0..10)
    double sigma_l = 1;             // colour tolerance in standard errors
    double sigma_p = 0.05;          // plane-distance tolerance as a fraction of the hit distance
};

// Extension (not in the reference): the projection of Camera::render_lens (crt_lens, whose fields
// these are). The factories orthonormalise the basis: forward is normalised, right = unit(forward x
// up), then up = right x forward; the library uses the basis as given.
struct Lens {
    uint32_t kind = CRT_LENS_PINHOLE;
    Point3D origin{0, 0, 0};
    Vec3D right{1, 0, 0}, up{0, 1, 0}, forward{0, 0, -1};
    double extent_x = 0, extent_y = 0;
    uint64_t batch_pixels = 0;  // sizes the internal batches only
    bool plain = false;         // CRT_RADIANCE_PLAIN: the same bits either way

    // the camera's own projection: render_lens then gives render()'s picture
    static Lens pinhole() { return Lens{}; }
    static Lens looking(uint32_t kind, const Point3D& origin, const Vec3D& forward, const Vec3D& up, double ex, double ey) {
        Lens l;
        l.kind = kind;
        l.origin = origin;
        l.forward = forward.unit_vector();
        l.right = cross(l.forward, up).unit_vector();
        l.up = cross(l.right, l.forward);
        l.extent_x = ex;
        l.extent_y = ey;
        return l;
    }
    // half_w, half_h: the half width and half height of the view in world units
    static Lens orthographic(const Point3D& origin, const Vec3D& forward, const Vec3D& up, double half_w, double half_h) {
        return looking(CRT_LENS_ORTHOGRAPHIC, origin, forward, up, half_w, half_h);
    }
    // a latitude-longitude panorama: the whole sphere by default
    static Lens equirect(const Point3D& origin, const Vec3D& forward = Vec3D{0, 0, -1}, const Vec3D& up = Vec3D{0, 1, 0},
                         double half_angle_x = std::numbers::pi, double half_angle_y = std::numbers::pi / 2) {
        return looking(CRT_LENS_EQUIRECT, origin, forward, up, half_angle_x, half_angle_y);
    }
    // equidistant fisheye: the angles from the axis at the frame's left-right and top-bottom edges
    static Lens fisheye(const Point3D& origin, const Vec3D& forward = Vec3D{0, 0, -1}, const Vec3D& up = Vec3D{0, 1, 0},
                        double edge_angle_x = std::numbers::pi / 2, double edge_angle_y = std::numbers::pi / 2) {
        return looking(CRT_LENS_FISHEYE, origin, forward, up, edge_angle_x, edge_angle_y);
    }
    // six 90-degree faces +X -X +Y -Y +Z -Z stacked top to bottom: the image must be w x 6w
    static Lens cube(const Point3D& origin, const Vec3D& forward = Vec3D{0, 0, -1}, const Vec3D& up = Vec3D{0, 1, 0}) {
        return looking(CRT_LENS_CUBE, origin, forward, up, 0, 0);
    }

    crt_lens as_crt() const {
        crt_lens l{};
        l.kind = kind;
        l.flags = plain ? CRT_RADIANCE_PLAIN : 0u;
        for (size_t k = 0; k < 3; ++k) {
            l.origin[k] = origin[k];
            l.right[k] = right[k];
            l.up[k] = up[k];
            l.forward[k] = forward[k];
        }
        l.extent_x = extent_x;
        l.extent_y = extent_y;
        l.batch_pixels = batch_pixels;
        return l;
    }
};

// Extension (not in the reference): a cube-map environment for Camera::render_lens(world, lens, env)
// (crt_env with the texels in host memory): what paths that leave the scene see in place of the
// camera's constant background. The factory takes a cube frame as render_lens returns it for
// Lens::cube (w x 6w) and builds the basis as Lens's factories do. importance: render_lens samples the
// map by luminance at every Lambertian bounce and weights it against the bounce's own escape
// (crt_render_lens_env_sampled: next-event estimation with MIS), so a small bright region of the map
// is no longer found by chance alone. The face size is then at most 2048.
struct Environment {
    std::vector<double> texels;  // 6n rows x n columns x 3
    uint32_t face_size = 0;
    uint32_t filter = CRT_ENV_BILINEAR;
    Vec3D right{1, 0, 0}, up{0, 1, 0}, forward{0, 0, -1};
    bool importance = false;

    static Environment from_cube(const Image& frame, const Vec3D& forward = Vec3D{0, 0, -1},
                                 const Vec3D& up = Vec3D{0, 1, 0}, uint32_t filter = CRT_ENV_BILINEAR,
                                 bool importance = false) {
        Environment e;
        e.face_size = static_cast<uint32_t>(frame.width());
        e.filter = filter;
        e.importance = importance;
        e.forward = forward.unit_vector();
        e.right = cross(e.forward, up).unit_vector();
        e.up = cross(e.right, e.forward);
        e.texels.resize(frame.width() * frame.height() * 3);
        for (size_t r = 0; r < frame.height(); ++r)
            for (size_t c = 0; c < frame.width(); ++c) {
                const RGB& p = frame[r][c];
                double* t = &e.texels[(r * frame.width() + c) * 3];
                t[0] = p.r; t[1] = p.g; t[2] = p.b;
            }
        if (frame.height() != 6 * frame.width()) e.face_size = 0;  // not a cube frame: the library refuses it
        return e;
    }

    crt_env as_crt() const {
        crt_env v{};
        v.texels = texels.data();
        v.face_size = face_size;
        v.filter = filter;
        for (size_t k = 0; k < 3; ++k) {
            v.right[k] = right[k];
            v.up[k] = up[k];
            v.forward[k] = forward[k];
        }
        return v;
    }
};

// Extension (not in the reference): the world's own lights as something to sample, for
// Camera::render_lens(world, lens, lights) (crt_render_lens_lights): every Lambertian bounce also sends
// a shadow ray to a point on a DiffuseLight primitive, weighted against the bounce's own light hits
// (next-event estimation with MIS), so a small light is no longer found by chance alone. The world must
// hold at least one light. A Lights belongs to the world it was made of.
struct Lights {
    const void* world = nullptr;
    template <typename T>
    static Lights of(const T& world) {
        Lights l;
        l.world = &world;
        return l;
    }
};

// Extension (not in the reference): what lights a lens render, two independent choices: an Environment
// (its importance decides between the sampled and the plain map) or none, and the world's Lights or none
// (crt_render_lens_lit, crt_render_lens_passes_lit). With both, every Lambertian bounce samples the map
// and the lights, each weighted against the bounce. Both are borrowed for the call.
struct Lighting {
    const Environment* env = nullptr;
    const Lights* lights = nullptr;
};

class Camera {
    size_t image_w = 1280, image_h = 720;
    double viewport_w = 0, viewport_h = 0;
    Vec3D pixel_delta_x, pixel_delta_y;
    Ray3D camera{.origin = Point3D{0, 0, 0}, .dir = Vec3D{0, 0, -1}};
    std::optional<Point3D> camera_lookat;
    Vec3D view_up_dir{0, 1, 0};
    Vec3D cam_basis_x, cam_basis_y, cam_basis_z;
    std::optional<double> focus_dist;
    double defocus_angle = 0;
    Vec3D defocus_disk_x, defocus_disk_y;
    Point3D pixel00_loc;
    size_t samples_per_pixel = 1;
    size_t max_depth = 10;
    std::optional<double> vertical_fov{90}, horizontal_fov;
    RGB background{RGB::from_mag(0.5)};
    crt_camera_settings settings{};
    crt_camera resolved{};

    static Vec3D v(const double* p) { return Vec3D{p[0], p[1], p[2]}; }
    static void put(double* p, const Vec3D& a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }

    // Camera::init (camera.h:87-157), computed by crt_camera_resolve; the same state updates
    // (direction from the lookat point, default focus distance) are kept here.
    void init() {
        if (camera_lookat) camera.dir = *camera_lookat - camera.origin;
        if (!focus_dist) focus_dist = camera.dir.mag();
        // the ABI carries these as 32-bit counts: refuse values a cast would truncate
        const auto u32 = [](size_t x, const char* what) {
            if (x > UINT32_MAX) {
                std::cout << "Error: Camera: " << what << " = " << x
                          << " exceeds the render path's 32-bit range (4294967295)" << std::endl;
                std::exit(-1);
            }
            return static_cast<uint32_t>(x);
        };
        crt_camera_settings s{};
        s.image_w = u32(image_w, "image width");
        s.image_h = u32(image_h, "image height");
        s.samples_per_pixel = u32(samples_per_pixel, "samples_per_pixel");
        s.max_depth = u32(max_depth, "max_depth");
        put(s.center, camera.origin);
        put(s.direction, camera.dir);
        put(s.up, view_up_dir);
        s.has_focus_dist = 1;
        s.focus_dist = *focus_dist;
        s.fov_is_vertical = vertical_fov.has_value();
        s.fov = vertical_fov ? *vertical_fov : *horizontal_fov;
        s.defocus_angle = defocus_angle;
        s.background[0] = background.r;
        s.background[1] = background.g;
        s.background[2] = background.b;
        if (crt_camera_resolve(&s, &resolved)) crt_api::die("crt_camera_resolve");
        settings = s;
        const double aspect = static_cast<double>(image_w) / static_cast<double>(image_h);
        if (vertical_fov) {
            viewport_h = 2 * *focus_dist * std::tan(*vertical_fov / 2);
            viewport_w = viewport_h * aspect;
        } else {
            viewport_w = 2 * *focus_dist * std::tan(*horizontal_fov / 2);
            viewport_h = viewport_w / aspect;
        }
        cam_basis_z = -camera.dir.unit_vector();
        cam_basis_x = cross(view_up_dir, cam_basis_z).unit_vector();
        cam_basis_y = cross(cam_basis_z, cam_basis_x);
        pixel_delta_x = v(resolved.pixel_delta_x);
        pixel_delta_y = v(resolved.pixel_delta_y);
        pixel00_loc = v(resolved.pixel00);
        defocus_disk_x = v(resolved.defocus_disk_x);
        defocus_disk_y = v(resolved.defocus_disk_y);
    }

    // CRT_DUMP_SCENE=<file>: write the flattened world + camera as a CRTS file (the format of
    // cpp_raytracer_amd.SceneData) and exit instead of rendering (scene-provenance tests)
    void dump_and_exit(const crt_api::GpuScene& g, const char* path) {
        std::FILE* f = std::fopen(path, "wb");
        if (!f) crt_api::die(std::string("cannot open ") + path);
        const uint32_t ver = 1;
        const uint64_t nm = g.material_records.size(), no = g.object_records.size();
        std::fwrite("CRTS", 1, 4, f);
        std::fwrite(&ver, 4, 1, f);
        std::fwrite(&nm, 8, 1, f);
        std::fwrite(&no, 8, 1, f);
        std::fwrite(&settings, sizeof settings, 1, f);
        std::fwrite(g.material_records.data(), sizeof(crt_material), nm, f);
        std::fwrite(g.object_records.data(), sizeof(crt_object), no, f);
        std::fclose(f);
        std::exit(0);
    }

    Image render_scene(const crt_api::GpuScene& g) {
        crt_scene* scene = g.get();
        init();
        if (const char* dump = std::getenv("CRT_DUMP_SCENE")) dump_and_exit(g, dump);
        resolved.base_seed = SeedSeqGenerator::get_instance().next_seed();
        int devices = 0;
        if (crt_device_count(&devices) || devices == 0) crt_api::die("Camera::render");
        if (const char* e = std::getenv("CRT_NUM_DEVICES")) devices = std::max(1, std::min(devices, std::atoi(e)));
        std::cout << "Rendering " << image_w << " x " << image_h << " image (" << samples_per_pixel
                  << " spp) on " << devices << " GPU" << (devices > 1 ? "s" : "") << std::endl;
        std::vector<double> rgb(image_w * image_h * 3);
        crt_render_stats stats{};
        auto t0 = std::chrono::steady_clock::now();
        if (crt_render(scene, &resolved, devices, rgb.data(), &stats)) crt_api::die("Camera::render");
        auto ms = ms_diff(t0, std::chrono::steady_clock::now());
        // parity guard (crt_render_guard): Dielectric branches a one-ulp different pow could flip
        uint64_t undecided = 0;
        for (int d = 0; d < devices; ++d) {
            uint64_t n = 0;
            if (crt_render_guard(scene, d, &n, 1) == 0) undecided += n;
        }
        if (undecided)
            std::cerr << "Camera::render: " << undecided << " Dielectric reflect-or-refract decision(s) depend on "
                      << "the last bit of pow(1 - cos, 5); the CPU reference's glibc may take the other branch there"
                      << std::endl;
        std::cout << "Rendering " << image_w << " x " << image_h << " image: Finished in " << ms << "ms\n"
                  << std::endl;
        auto img = Image::with_dimensions(image_w, image_h);
        for (size_t r = 0; r < image_h; ++r)
            for (size_t c = 0; c < image_w; ++c) {
                const double* p = &rgb[(r * image_w + c) * 3];
                img[r][c] = RGB::from_mag(p[0], p[1], p[2]);
            }
        return img;
    }

    // render_scene in passes (crt_render_progressive): one ProgressBar tick and one on_pass call
    // per pass; on_pass returning false stops the render with the image of the samples so far
    struct ProgressiveCtx {
        ProgressBar<>* bar;
        const std::function<bool(size_t, size_t, double)>* on_pass;
    };
    static int progressive_pass(void* user, uint32_t done, uint32_t total, double noise, const double*) {
        auto* ctx = static_cast<ProgressiveCtx*>(user);
        ctx->bar->complete_iteration();
        return (*ctx->on_pass && !(*ctx->on_pass)(done, total, noise)) ? 1 : 0;
    }

    Image render_scene_progressive(const crt_api::GpuScene& g, size_t samples_per_pass,
                                   const std::function<bool(size_t, size_t, double)>& on_pass) {
        crt_scene* scene = g.get();
        init();
        if (const char* dump = std::getenv("CRT_DUMP_SCENE")) dump_and_exit(g, dump);
        resolved.base_seed = SeedSeqGenerator::get_instance().next_seed();
        int devices = 0;
        if (crt_device_count(&devices) || devices == 0) crt_api::die("Camera::render_progressive");
        if (const char* e = std::getenv("CRT_NUM_DEVICES")) devices = std::max(1, std::min(devices, std::atoi(e)));
        if (samples_per_pass > UINT32_MAX) samples_per_pass = UINT32_MAX;
        // the passes crt_render_progressive will run: whole chunks, 0 = a tenth of the samples
        const size_t chunk = crt_sample_chunk_len(resolved.samples_per_pixel);
        size_t per_pass = samples_per_pass ? samples_per_pass : std::max<size_t>(1, samples_per_pixel / 10);
        per_pass = (per_pass + chunk - 1) / chunk * chunk;
        ProgressBar<> bar((samples_per_pixel + per_pass - 1) / per_pass,
                          "Rendering " + std::to_string(image_w) + " x " + std::to_string(image_h) + " image (" +
                              std::to_string(samples_per_pixel) + " spp) in passes on " + std::to_string(devices) +
                              " GPU" + (devices > 1 ? "s" : ""));
        std::vector<double> rgb(image_w * image_h * 3);
        ProgressiveCtx ctx{&bar, &on_pass};
        uint32_t done = 0;
        if (crt_render_progressive(scene, &resolved, devices, static_cast<uint32_t>(samples_per_pass),
                                   on_pass ? CRT_PROGRESS_NOISE : 0u, progressive_pass, &ctx, rgb.data(), &done))
            crt_api::die("Camera::render_progressive");
        if (done < samples_per_pixel)
            std::cout << "Rendering stopped after " << done << " of " << samples_per_pixel << " spp\n" << std::endl;
        auto img = Image::with_dimensions(image_w, image_h);
        for (size_t r = 0; r < image_h; ++r)
            for (size_t c = 0; c < image_w; ++c) {
                const double* p = &rgb[(r * image_w + c) * 3];
                img[r][c] = RGB::from_mag(p[0], p[1], p[2]);
            }
        return img;
    }

    // render_scene_progressive with adaptive sampling (crt_render_adaptive): blocks of 16 x 4
    // pixels stop once their noise is at most `threshold`
    struct AdaptiveCtx {
        ProgressBar<>* bar;
        const std::function<bool(size_t, size_t, size_t, size_t)>* on_pass;
    };
    static int adaptive_pass(void* user, uint32_t done, uint32_t total, uint32_t active, uint32_t blocks,
                             const double*) {
        auto* ctx = static_cast<AdaptiveCtx*>(user);
        ctx->bar->complete_iteration();
        return (*ctx->on_pass && !(*ctx->on_pass)(done, total, active, blocks)) ? 1 : 0;
    }

    Image render_scene_adaptive(const crt_api::GpuScene& g, double threshold, size_t min_samples,
                                size_t samples_per_pass,
                                const std::function<bool(size_t, size_t, size_t, size_t)>& on_pass) {
        crt_scene* scene = g.get();
        init();
        if (const char* dump = std::getenv("CRT_DUMP_SCENE")) dump_and_exit(g, dump);
        resolved.base_seed = SeedSeqGenerator::get_instance().next_seed();
        int devices = 0;
        if (crt_device_count(&devices) || devices == 0) crt_api::die("Camera::render_adaptive");
        if (const char* e = std::getenv("CRT_NUM_DEVICES")) devices = std::max(1, std::min(devices, std::atoi(e)));
        if (samples_per_pass > UINT32_MAX) samples_per_pass = UINT32_MAX;
        const size_t chunk = crt_sample_chunk_len(resolved.samples_per_pixel);
        size_t per_pass = samples_per_pass ? samples_per_pass : std::max<size_t>(1, samples_per_pixel / 10);
        per_pass = (per_pass + chunk - 1) / chunk * chunk;
        if (min_samples == 0) min_samples = 2 * per_pass;  // two passes' worth
        if (min_samples > UINT32_MAX) min_samples = UINT32_MAX;
        ProgressBar<> bar((samples_per_pixel + per_pass - 1) / per_pass,
                          "Rendering " + std::to_string(image_w) + " x " + std::to_string(image_h) + " image (up to " +
                              std::to_string(samples_per_pixel) + " spp, adaptive) on " + std::to_string(devices) +
                              " GPU" + (devices > 1 ? "s" : ""));
        std::vector<double> rgb(image_w * image_h * 3);
        AdaptiveCtx ctx{&bar, &on_pass};
        crt_adaptive_params prm{};
        prm.threshold = threshold;
        prm.min_samples = static_cast<uint32_t>(min_samples);
        prm.samples_per_pass = static_cast<uint32_t>(samples_per_pass);
        uint64_t rendered = 0;
        if (crt_render_adaptive(scene, &resolved, devices, &prm, adaptive_pass, &ctx, rgb.data(), nullptr, &rendered))
            crt_api::die("Camera::render_adaptive");
        std::cout << "Rendered " << static_cast<double>(rendered) / static_cast<double>(image_w * image_h)
                  << " spp on average (of " << samples_per_pixel << ")\n" << std::endl;
        auto img = Image::with_dimensions(image_w, image_h);
        for (size_t r = 0; r < image_h; ++r)
            for (size_t c = 0; c < image_w; ++c) {
                const double* p = &rgb[(r * image_w + c) * 3];
                img[r][c] = RGB::from_mag(p[0], p[1], p[2]);
            }
        return img;
    }

    // render_scene followed by the denoiser: every sample, or with adaptive_threshold >= 0 an
    // adaptive render at that threshold. devices == 1: on GPU 0 (crt_render_denoised); 0 (all
    // visible) or any other count: rendered over that many GPUs, filtered on GPU 0
    // (crt_render_denoised_devices), the same picture
    Image render_scene_denoised(const crt_api::GpuScene& g, const DenoiseOptions& opt, double adaptive_threshold,
                                int devices) {
        crt_scene* scene = g.get();
        init();
        if (const char* dump = std::getenv("CRT_DUMP_SCENE")) dump_and_exit(g, dump);
        resolved.base_seed = SeedSeqGenerator::get_instance().next_seed();
        int visible = 0;
        if (crt_device_count(&visible) || visible == 0) crt_api::die("Camera::render_denoised");
        const bool adaptive = adaptive_threshold >= 0;
        const bool one = devices == 1;
        if (!one) {  // the count the render will use (crt_render_denoised_devices' rule)
            devices = devices <= 0 ? visible : std::min(devices, visible);
            if (const char* e = std::getenv("CRT_EMULATE_DEVICES")) devices = std::max(1, std::min(std::atoi(e), 64));
        }
        std::cout << "Rendering " << image_w << " x " << image_h << " image (" << (adaptive ? "up to " : "")
                  << samples_per_pixel << " spp" << (adaptive ? ", adaptive" : "") << ", denoised) on " << devices << " GPU"
                  << (devices > 1 ? "s" : "") << std::endl;
        std::vector<double> rgb(image_w * image_h * 3);
        crt_denoise_params dp{};
        dp.iterations = opt.iterations;
        dp.normal_squarings = opt.normal_squarings;
        dp.sigma_l = opt.sigma_l;
        dp.sigma_p = opt.sigma_p;
        crt_adaptive_params ap{};
        ap.threshold = adaptive_threshold;
        {  // render_adaptive's defaults: passes of a tenth of the samples, a floor of two passes
            const size_t chunk = crt_sample_chunk_len(resolved.samples_per_pixel);
            const size_t per_pass = (std::max<size_t>(1, samples_per_pixel / 10) + chunk - 1) / chunk * chunk;
            ap.min_samples = static_cast<uint32_t>(std::min<size_t>(2 * per_pass, UINT32_MAX));
        }
        uint64_t rendered = 0;
        auto t0 = std::chrono::steady_clock::now();
        if (one ? crt_render_denoised(scene, 0, &resolved, adaptive ? &ap : nullptr, &dp, nullptr, rgb.data(), &rendered)
                : crt_render_denoised_devices(scene, &resolved, devices, adaptive ? &ap : nullptr, &dp, nullptr, nullptr,
                                              nullptr, rgb.data(), nullptr, &rendered))
            crt_api::die("Camera::render_denoised");
        auto ms = ms_diff(t0, std::chrono::steady_clock::now());
        std::cout << "Rendered " << static_cast<double>(rendered) / static_cast<double>(image_w * image_h)
                  << " spp on average (of " << samples_per_pixel << "), denoised: Finished in " << ms << "ms\n"
                  << std::endl;
        auto img = Image::with_dimensions(image_w, image_h);
        for (size_t r = 0; r < image_h; ++r)
            for (size_t c = 0; c < image_w; ++c) {
                const double* p = &rgb[(r * image_w + c) * 3];
                img[r][c] = RGB::from_mag(p[0], p[1], p[2]);
            }
        return img;
    }

    // lit: over crt_render_lens_lit whatever is set (Camera::render_lens(world, lens, Lighting))
    Image render_scene_lens(const crt_api::GpuScene& g, const Lens& lens, const Environment* env = nullptr,
                            bool lights = false, bool lit = false) {
        init();
        resolved.base_seed = SeedSeqGenerator::get_instance().next_seed();
        const crt_lens l = lens.as_crt();
        std::vector<double> rgb(image_w * image_h * 3);
        if (lit) {
            crt_env e{};
            if (env) e = env->as_crt();
            if (crt_render_lens_lit(g.get(), 0, &resolved, &l, env ? &e : nullptr, env && env->importance ? 1 : 0, lights ? 1 : 0,
                                    rgb.data()))
                crt_api::die("crt_render_lens_lit");
        } else if (lights) {
            if (crt_render_lens_lights(g.get(), 0, &resolved, &l, rgb.data())) crt_api::die("crt_render_lens_lights");
        } else if (env) {
            const crt_env e = env->as_crt();
            if (env->importance) {
                if (crt_render_lens_env_sampled(g.get(), 0, &resolved, &l, &e, rgb.data())) crt_api::die("crt_render_lens_env_sampled");
            } else if (crt_render_lens_env(g.get(), 0, &resolved, &l, &e, rgb.data())) {
                crt_api::die("crt_render_lens_env");
            }
        } else if (crt_render_lens(g.get(), 0, &resolved, &l, rgb.data())) {
            crt_api::die("crt_render_lens");
        }
        auto img = Image::with_dimensions(image_w, image_h);
        for (size_t r = 0; r < image_h; ++r)
            for (size_t c = 0; c < image_w; ++c) {
                const double* p = &rgb[(r * image_w + c) * 3];
                img[r][c] = RGB::from_mag(p[0], p[1], p[2]);
            }
        return img;
    }

    static void check_lighting(const void* world, const Lighting& lit) {
        if (lit.lights && lit.lights->world != world) crt_api::die("Camera::render_lens: the Lights were made of another world");
    }

    // render_scene_lens in passes (crt_render_lens_passes): the callback ticks the bar and asks on_pass
    struct LensPassCtx {
        ProgressBar<>* bar;
        const std::function<bool(size_t, size_t)>* on_pass;
    };
    static int lens_pass(void* user, uint32_t done, uint32_t total, uint32_t, uint32_t, const double*, const double*) {
        auto* ctx = static_cast<LensPassCtx*>(user);
        if (ctx->bar) ctx->bar->complete_iteration();
        return (ctx->on_pass && *ctx->on_pass && !(*ctx->on_pass)(done, total)) ? 1 : 0;
    }

    // progressive: plain passes of samples_per_pass samples (no block ever stops); else every sample, or
    // with adaptive_threshold >= 0 an adaptive render, then the denoiser (a cube map one face at a time)
    Image render_scene_lens_passes(const crt_api::GpuScene& g, const Lens& lens, bool progressive, size_t samples_per_pass,
                                   const std::function<bool(size_t, size_t)>& on_pass, const DenoiseOptions& opt,
                                   double adaptive_threshold, const Lighting* lit = nullptr) {
        init();
        resolved.base_seed = SeedSeqGenerator::get_instance().next_seed();
        const crt_lens l = lens.as_crt();
        const size_t chunk = crt_sample_chunk_len(resolved.samples_per_pixel);
        if (samples_per_pass > UINT32_MAX) samples_per_pass = UINT32_MAX;
        size_t per_pass = samples_per_pass ? samples_per_pass : std::max<size_t>(1, samples_per_pixel / 10);
        per_pass = (per_pass + chunk - 1) / chunk * chunk;
        const bool adaptive = !progressive && adaptive_threshold >= 0;
        crt_adaptive_params ap{};
        ap.threshold = adaptive ? adaptive_threshold : 0;
        // progressive: min_samples >= samples_per_pixel never stops a block; adaptive: render_adaptive's
        // floor of two passes
        ap.min_samples = adaptive ? static_cast<uint32_t>(std::min<size_t>(2 * per_pass, UINT32_MAX)) : UINT32_MAX;
        ap.samples_per_pass = static_cast<uint32_t>(samples_per_pass);
        crt_denoise_params dp{};
        dp.iterations = opt.iterations;
        dp.normal_squarings = opt.normal_squarings;
        dp.sigma_l = opt.sigma_l;
        dp.sigma_p = opt.sigma_p;
        std::vector<double> rgb(image_w * image_h * 3);
        uint64_t rendered = 0;
        int rc;
        // under a Lighting: the same loop over crt_render_lens_passes_lit, the lighting made once for the call
        crt_env e{};
        if (lit && lit->env) e = lit->env->as_crt();
        const crt_env* pe = lit && lit->env ? &e : nullptr;
        const int importance = lit && lit->env && lit->env->importance ? 1 : 0, lights = lit && lit->lights ? 1 : 0;
        if (progressive) {
            ProgressBar<> bar((samples_per_pixel + per_pass - 1) / per_pass,
                              "Rendering " + std::to_string(image_w) + " x " + std::to_string(image_h) + " lens image (" +
                                  std::to_string(samples_per_pixel) + " spp) in passes");
            LensPassCtx ctx{&bar, &on_pass};
            rc = lit ? crt_render_lens_passes_lit(g.get(), 0, &resolved, &l, pe, importance, lights, &ap, nullptr, lens_pass, &ctx,
                                                  nullptr, rgb.data(), nullptr, &rendered)
                     : crt_render_lens_passes(g.get(), 0, &resolved, &l, &ap, nullptr, lens_pass, &ctx, nullptr, rgb.data(),
                                              nullptr, &rendered);
        } else {
            std::cout << "Rendering " << image_w << " x " << image_h << " lens image (" << (adaptive ? "up to " : "")
                      << samples_per_pixel << " spp" << (adaptive ? ", adaptive" : "") << ", denoised)" << std::endl;
            rc = lit ? crt_render_lens_passes_lit(g.get(), 0, &resolved, &l, pe, importance, lights, adaptive ? &ap : nullptr, &dp,
                                                  nullptr, nullptr, nullptr, rgb.data(), nullptr, &rendered)
                     : crt_render_lens_passes(g.get(), 0, &resolved, &l, adaptive ? &ap : nullptr, &dp, nullptr, nullptr, nullptr,
                                              rgb.data(), nullptr, &rendered);
        }
        if (rc) crt_api::die("Camera::render_lens passes");
        const double mean = static_cast<double>(rendered) / static_cast<double>(image_w * image_h);
        if (!progressive || mean < static_cast<double>(samples_per_pixel))
            std::cout << "Rendered " << mean << " spp on average (of " << samples_per_pixel << ")\n" << std::endl;
        auto img = Image::with_dimensions(image_w, image_h);
        for (size_t r = 0; r < image_h; ++r)
            for (size_t c = 0; c < image_w; ++c) {
                const double* p = &rgb[(r * image_w + c) * 3];
                img[r][c] = RGB::from_mag(p[0], p[1], p[2]);
            }
        return img;
    }

public:
    // Extension (not in the reference): render (adaptive_threshold < 0: every sample) or
    // render_adaptive (blocks stop at that threshold, default pass length and sample floor), then
    // the feature-guided a-trous denoiser of crt_denoise_async over the frame. Guided
    // by first-hit normals, positions and the per-pixel variance; what is seen through glass or in
    // mirrors is filtered by colour and variance alone, and albedo is not divided out.
    // devices: 1 = everything on one GPU; 0 = rendered over all visible GPUs, or over that many,
    // and filtered on GPU 0 (the same picture for any count).
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_denoised(const T& world, DenoiseOptions options = {}, double adaptive_threshold = -1, int devices = 1) {
        if constexpr (std::is_same_v<T, BVH>) {
            return render_scene_denoised(world.gpu_scene(), options, adaptive_threshold, devices);
        } else if constexpr (std::is_same_v<T, Scene>) {
            return render_denoised(BVH(world), options, adaptive_threshold, devices);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_denoised(s, options, adaptive_threshold, devices);
        }
    }

    // Extension (not in the reference): render_progressive with adaptive sampling. Blocks of
    // 16 x 4 pixels stop between passes once the sum of their pixels' standard errors is at most
    // `threshold` times the sum of their means, not before min_samples samples (0 = two passes'
    // worth); later passes trace the other blocks only. Ticks a ProgressBar once a pass and prints
    // the mean samples per pixel rendered. on_pass(samples done, samples in all, active blocks,
    // blocks in all) returning false stops the render. When no block stops (min_samples >=
    // samples_per_pixel never stops one) the image is render()'s bit for bit.
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_adaptive(const T& world, double threshold, size_t min_samples = 0, size_t samples_per_pass = 0,
                          std::function<bool(size_t done, size_t total, size_t active, size_t blocks)> on_pass = {}) {
        if constexpr (std::is_same_v<T, BVH>) {
            return render_scene_adaptive(world.gpu_scene(), threshold, min_samples, samples_per_pass, on_pass);
        } else if constexpr (std::is_same_v<T, Scene>) {
            return render_adaptive(BVH(world), threshold, min_samples, samples_per_pass, on_pass);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_adaptive(s, threshold, min_samples, samples_per_pass, on_pass);
        }
    }

    // Extension (not in the reference): render in passes of samples_per_pass samples per pixel
    // (0 = a tenth of them; rounded up to whole sample chunks), ticking a ProgressBar once a pass.
    // on_pass(samples done, samples in all, relative noise of the frame so far) returning false
    // stops the render and returns the image of the samples rendered so far. Rendered to the end,
    // the image is render()'s bit for bit.
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_progressive(const T& world, size_t samples_per_pass = 0,
                             std::function<bool(size_t done, size_t total, double noise)> on_pass = {}) {
        if constexpr (std::is_same_v<T, BVH>) {
            return render_scene_progressive(world.gpu_scene(), samples_per_pass, on_pass);
        } else if constexpr (std::is_same_v<T, Scene>) {
            return render_progressive(BVH(world), samples_per_pass, on_pass);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_progressive(s, samples_per_pass, on_pass);
        }
    }

    // camera.h:264-297: a BVH renders through its own node arrays; any other Hittable renders
    // with the semantics of its own hit_by (one always-entered leaf in object order)
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render(const T& world) {
        if constexpr (std::is_same_v<T, BVH>) {
            return render_scene(world.gpu_scene());
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene(s);
        }
    }

    // camera.h:301-303: a Scene renders through BVH(world)
    Image render(const Scene& world) { return render(BVH(world)); }

    // Extension (not in the reference): ray_color (camera.h:205-258) for the caller's own rays, one
    // path a ray with this camera's max_depth and background (crt_radiance: one upload, one launch,
    // one copy back). Element i is what the sample starting on rays[i] with the LCG state
    // states[i] adds to a pixel's sum in render(). An empty `states` seeds path i like sample 0 of
    // pixel i of a render (crt_sample_seed with the next seed of the SeedSeqGenerator). A ray with
    // a non-finite component or an all-zero direction sees the background.
    std::vector<RGB> ray_colors(const std::vector<Ray3D>& rays, const std::vector<uint32_t>& states, const BVH& world) {
        if (!states.empty() && states.size() != rays.size()) crt_api::die("Camera::ray_colors: one state a ray, or none");
        init();
        crt_radiance_params p{};
        p.max_depth = resolved.max_depth;
        p.base_seed = states.empty() ? SeedSeqGenerator::get_instance().next_seed() : 0u;
        for (int k = 0; k < 3; ++k) p.background[k] = resolved.background[k];
        p.t_min = resolved.t_min;
        const std::vector<double> r = BVH::crt_rays(rays);
        std::vector<double> rgb(rays.size() * 3);
        if (crt_radiance(world.gpu_scene().get(), 0, r.data(), rays.size(), states.empty() ? nullptr : states.data(), &p,
                         rgb.data()))
            crt_api::die("crt_radiance");
        std::vector<RGB> out;
        out.reserve(rays.size());
        for (size_t i = 0; i < rays.size(); ++i) out.push_back(RGB::from_mag(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]));
        return out;
    }

    // Extension (not in the reference): a probe bake (crt_probes: one upload, the bake, one copy
    // back). For each point, `samples` directions are drawn on the device, path-traced with this
    // camera's max_depth, background and t_min, and reduced in crt_probes_async's fixed order, seeded
    // with the next seed of the SeedSeqGenerator. mode CRT_PROBE_SPHERE: `normals` must be empty, nine
    // spherical-harmonic coefficients (bands 0..2) a point; CRT_PROBE_HEMISPHERE: one unit normal a
    // point, one cosine-weighted irradiance value a point. Returns the coefficients, K RGBs a point:
    // element p * K + k is coefficient k of point p.
    std::vector<RGB> probes(const BVH& world, const std::vector<Point3D>& points, const std::vector<Vec3D>& normals,
                            uint32_t samples, uint32_t mode = CRT_PROBE_SPHERE) {
        if (!normals.empty() && normals.size() != points.size()) crt_api::die("Camera::probes: one normal a point, or none");
        init();
        crt_probe_params p{};
        p.samples = samples;
        p.max_depth = resolved.max_depth;
        p.base_seed = SeedSeqGenerator::get_instance().next_seed();
        p.mode = mode;
        for (int k = 0; k < 3; ++k) p.background[k] = resolved.background[k];
        p.t_min = resolved.t_min;
        const size_t n = points.size(), K = mode == CRT_PROBE_SPHERE ? 9 : 1;
        std::vector<double> pts(n * 3), nrm(normals.size() * 3), coeff(n * K * 3);
        for (size_t i = 0; i < n; ++i)
            for (size_t k = 0; k < 3; ++k) pts[3 * i + k] = points[i][k];
        for (size_t i = 0; i < normals.size(); ++i)
            for (size_t k = 0; k < 3; ++k) nrm[3 * i + k] = normals[i][k];
        if (crt_probes(world.gpu_scene().get(), 0, pts.data(), normals.empty() ? nullptr : nrm.data(), n, &p, coeff.data()))
            crt_api::die("crt_probes");
        std::vector<RGB> out;
        out.reserve(n * K);
        for (size_t i = 0; i < n * K; ++i) out.push_back(RGB::from_mag(coeff[3 * i], coeff[3 * i + 1], coeff[3 * i + 2]));
        return out;
    }

    // Extension (not in the reference): a whole frame through `lens` (crt_render_lens: one upload,
    // the render, one copy back) with this camera's image size, samples, max_depth, background and
    // t_min, seeded with the next seed of the SeedSeqGenerator. Panoramic, fisheye, cube-map and
    // orthographic frames; with Lens::pinhole() the picture is render()'s. A cube map needs an image
    // of w x 6w.
    Image render_lens(const BVH& world, const Lens& lens) { return render_scene_lens(world.gpu_scene(), lens); }
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_lens(const T& world, const Lens& lens) {
        if constexpr (std::is_same_v<T, Scene>) {
            return render_lens(BVH(world), lens);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_lens(s, lens);
        }
    }
    // Extension (not in the reference): render_lens lit by a cube-map environment (crt_render_lens_env, or
    // crt_render_lens_env_sampled for an Environment with importance): paths that leave the scene see
    // env in place of the constant background.
    Image render_lens(const BVH& world, const Lens& lens, const Environment& env) {
        return render_scene_lens(world.gpu_scene(), lens, &env);
    }
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_lens(const T& world, const Lens& lens, const Environment& env) {
        if constexpr (std::is_same_v<T, Scene>) {
            return render_lens(BVH(world), lens, env);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_lens(s, lens, &env);
        }
    }
    // Extension (not in the reference): render_lens with the world's own lights sampled (crt_render_lens_lights).
    Image render_lens(const BVH& world, const Lens& lens, const Lights& lights) {
        if (lights.world != &world) crt_api::die("Camera::render_lens: the Lights were made of another world");
        return render_scene_lens(world.gpu_scene(), lens, nullptr, true);
    }
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_lens(const T& world, const Lens& lens, const Lights& lights) {
        if (lights.world != &world) crt_api::die("Camera::render_lens: the Lights were made of another world");
        if constexpr (std::is_same_v<T, Scene>) {
            return render_scene_lens(BVH(world).gpu_scene(), lens, nullptr, true);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_lens(s, lens, nullptr, true);
        }
    }

    // Extension (not in the reference): render_lens under a Lighting, an Environment and the world's Lights
    // together or either alone (crt_render_lens_lit), and the same in passes and denoised
    // (crt_render_lens_passes_lit); with nothing set they are the calls without a Lighting.
    Image render_lens(const BVH& world, const Lens& lens, const Lighting& lit) {
        check_lighting(&world, lit);
        return render_scene_lens(world.gpu_scene(), lens, lit.env, lit.lights != nullptr, true);
    }
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_lens(const T& world, const Lens& lens, const Lighting& lit) {
        check_lighting(&world, lit);
        if constexpr (std::is_same_v<T, Scene>) {
            return render_scene_lens(BVH(world).gpu_scene(), lens, lit.env, lit.lights != nullptr, true);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_lens(s, lens, lit.env, lit.lights != nullptr, true);
        }
    }
    Image render_lens_progressive(const BVH& world, const Lens& lens, const Lighting& lit, size_t samples_per_pass = 0,
                                  std::function<bool(size_t done, size_t total)> on_pass = {}) {
        check_lighting(&world, lit);
        return render_scene_lens_passes(world.gpu_scene(), lens, true, samples_per_pass, on_pass, {}, -1, &lit);
    }
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_lens_progressive(const T& world, const Lens& lens, const Lighting& lit, size_t samples_per_pass = 0,
                                  std::function<bool(size_t done, size_t total)> on_pass = {}) {
        check_lighting(&world, lit);
        if constexpr (std::is_same_v<T, Scene>) {
            return render_scene_lens_passes(BVH(world).gpu_scene(), lens, true, samples_per_pass, on_pass, {}, -1, &lit);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_lens_passes(s, lens, true, samples_per_pass, on_pass, {}, -1, &lit);
        }
    }
    Image render_lens_denoised(const BVH& world, const Lens& lens, const Lighting& lit, DenoiseOptions options = {},
                               double adaptive_threshold = -1) {
        check_lighting(&world, lit);
        return render_scene_lens_passes(world.gpu_scene(), lens, false, 0, {}, options, adaptive_threshold, &lit);
    }
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_lens_denoised(const T& world, const Lens& lens, const Lighting& lit, DenoiseOptions options = {},
                               double adaptive_threshold = -1) {
        check_lighting(&world, lit);
        if constexpr (std::is_same_v<T, Scene>) {
            return render_scene_lens_passes(BVH(world).gpu_scene(), lens, false, 0, {}, options, adaptive_threshold, &lit);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_lens_passes(s, lens, false, 0, {}, options, adaptive_threshold, &lit);
        }
    }

    // Extension (not in the reference): render_lens in passes of samples_per_pass samples per pixel (0 = a
    // tenth of them; rounded up to whole sample chunks) over crt_render_lens_passes, ticking a ProgressBar
    // once a pass. on_pass(samples done, samples in all) returning false stops the render and returns
    // the image of the samples rendered so far. Rendered to the end, the image is render_lens' bit for bit.
    Image render_lens_progressive(const BVH& world, const Lens& lens, size_t samples_per_pass = 0,
                                  std::function<bool(size_t done, size_t total)> on_pass = {}) {
        return render_scene_lens_passes(world.gpu_scene(), lens, true, samples_per_pass, on_pass, {}, -1);
    }
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_lens_progressive(const T& world, const Lens& lens, size_t samples_per_pass = 0,
                                  std::function<bool(size_t done, size_t total)> on_pass = {}) {
        if constexpr (std::is_same_v<T, Scene>) {
            return render_lens_progressive(BVH(world), lens, samples_per_pass, on_pass);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_lens_passes(s, lens, true, samples_per_pass, on_pass, {}, -1);
        }
    }

    // Extension (not in the reference): render_lens (adaptive_threshold < 0: every sample) or an adaptive
    // lens render (blocks stop at that threshold, render_adaptive's pass length and sample floor), then
    // render_denoised's filter guided by the first hits seen through the lens; a cube map is filtered one
    // face at a time. With Lens::pinhole() the picture is render_denoised's on one GPU. Panorama taps do not
    // wrap at the left-right seam.
    Image render_lens_denoised(const BVH& world, const Lens& lens, DenoiseOptions options = {}, double adaptive_threshold = -1) {
        return render_scene_lens_passes(world.gpu_scene(), lens, false, 0, {}, options, adaptive_threshold);
    }
    template <typename T>
    requires std::is_base_of_v<Hittable, T>
    Image render_lens_denoised(const T& world, const Lens& lens, DenoiseOptions options = {}, double adaptive_threshold = -1) {
        if constexpr (std::is_same_v<T, Scene>) {
            return render_lens_denoised(BVH(world), lens, options, adaptive_threshold);
        } else {
            crt_api::GpuScene s(world, 32, 12, true);
            return render_scene_lens_passes(s, lens, false, 0, {}, options, adaptive_threshold);
        }
    }

    Camera& set_camera_center(const Point3D& p) { camera.origin = p; return *this; }
    Camera& set_camera_direction(const Vec3D& d) { camera.dir = d; return *this; }
    Camera& set_camera_direction_towards(const Point3D& p) {
        camera.dir = p - camera.origin;
        camera_lookat.reset();
        return *this;
    }
    Camera& set_camera_lookat(const Point3D& p) { camera_lookat = p; return *this; }
    Camera& set_focus_distance(double d) { focus_dist = d; return *this; }
    Camera& set_defocus_angle(double deg) { defocus_angle = deg * std::numbers::pi / 180; return *this; }
    Camera& turn_blur_off() { defocus_angle = 0; return *this; }
    Camera& set_camera_up_direction(const Vec3D& d) { view_up_dir = d; return *this; }
    Camera& set_image_width(size_t w) { image_w = w; return *this; }
    Camera& set_image_height(size_t h) { image_h = h; return *this; }
    Camera& set_image_dimensions(size_t w, size_t h) { image_w = w; image_h = h; return *this; }
    Camera& set_image_by_width_and_aspect_ratio(size_t w, double aspect) {
        auto h = static_cast<size_t>(std::round(static_cast<double>(w) / aspect));
        return set_image_dimensions(w, std::max(size_t{1}, h));
    }
    Camera& set_image_by_height_and_aspect_ratio(size_t h, double aspect) {
        auto w = static_cast<size_t>(std::round(static_cast<double>(h) * aspect));
        return set_image_dimensions(std::max(size_t{1}, w), h);
    }
    Camera& set_samples_per_pixel(size_t s) { samples_per_pixel = s; return *this; }
    Camera& set_max_depth(size_t d) { max_depth = d; return *this; }
    Camera& set_vertical_fov(double deg) {
        vertical_fov = deg * std::numbers::pi / 180;
        horizontal_fov.reset();
        return *this;
    }
    Camera& set_horizontal_fov(double deg) {
        horizontal_fov = deg * std::numbers::pi / 180;
        vertical_fov.reset();
        return *this;
    }
    Camera& set_background(const RGB& c) { background = c; return *this; }

    void print_to(std::ostream& os) {
        init();
        os << "Camera {\n"
           << "\tImage dimensions: " << image_w << " x " << image_h << '\n'
           << "\tViewport dimensions: " << viewport_w << " x " << viewport_h << '\n'
           << "\tpixel_delta_x: " << pixel_delta_x << '\n'
           << "\tpixel_delta_y: " << pixel_delta_y << '\n'
           << "\tCamera center: " << camera.origin << '\n'
           << "\tCamera direction: " << camera.dir << '\n'
           << "\tUp direction: " << view_up_dir << '\n'
           << "\tCamera orientation x-, y-, and z- orthonormal basis vectors {"
           << "\n\t\tx: " << cam_basis_x << "\n\t\ty: " << cam_basis_y << "\n\t\tz: " << cam_basis_z << "\n\t}\n"
           << "\tFocus distance: " << *focus_dist << '\n'
           << "\tDefocus angle: " << defocus_angle << " rad, " << defocus_angle * 180 / std::numbers::pi
           << " degrees\n"
           << "\tDefocus dist x-, y- orthonormal basis vectors {"
           << "\n\t\tx: " << defocus_disk_x << "\n\t\ty: " << defocus_disk_y << "\n\t}\n"
           << "\tTop-left pixel's center on viewport: " << pixel00_loc << '\n'
           << "\tSamples per pixel: " << samples_per_pixel << '\n'
           << "\tMaximum bounces per ray: " << max_depth << '\n'
           << "\tVertical FOV (-1 means not given): " << vertical_fov.value_or(-1) << " rad, "
           << (vertical_fov ? *vertical_fov * 180 / std::numbers::pi : -1) << " degrees\n"
           << "\tHorizontal FOV (-1 means not given): " << horizontal_fov.value_or(-1) << " rad, "
           << (horizontal_fov ? *horizontal_fov * 180 / std::numbers::pi : -1) << " degrees\n}";
    }
};

inline std::ostream& operator<<(std::ostream& os, Camera cam) {
    cam.print_to(os);
    return os;
}

#endif
