// Camera::render_lens_progressive and Camera::render_lens_denoised (the drop-in's extensions over
// crt_render_lens_passes) from the middle of the Cornell box (src/main.cpp:326-363), 24 samples a pixel:
// a fisheye 40 x 24 frame and a 4 x 24 cube map rendered in passes to the end against render_lens with
// the same seed, a progressive render stopped by on_pass after two passes against crt_render_lens_passes
// stopped the same way, and render_lens_denoised with Lens::pinhole() against render_denoised, plain and
// adaptive. Prints "lens passes <passes> stopped <samples> lit <n>" and exits non-zero on the first
// differing byte (tests/test_gpu_lens_passes_cpp.py).
//   lens_passes_e2e <seed>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <vector>

#include "acceleration/bvh.h"
#include "base/camera.h"
#include "base/scene.h"
#include "shapes/shapes.h"

static bool same(const Image& a, const Image& b, size_t w, size_t h, const char* what, size_t* lit = nullptr) {
    for (size_t r = 0; r < h; ++r)
        for (size_t c = 0; c < w; ++c) {
            const double x[3] = {a[r][c].r, a[r][c].g, a[r][c].b}, y[3] = {b[r][c].r, b[r][c].g, b[r][c].b};
            if (std::memcmp(x, y, sizeof x) != 0) {
                std::cout << what << ": pixel " << r << " " << c << " differs" << std::endl;
                return false;
            }
            if (lit && (x[0] > 0 || x[1] > 0 || x[2] > 0)) ++*lit;
        }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const uint32_t seed = static_cast<uint32_t>(std::strtoul(argv[1], nullptr, 10));
    auto red = std::make_shared<Lambertian>(RGB::from_mag(.65, .05, .05));
    auto white = std::make_shared<Lambertian>(RGB::from_mag(.73, .73, .73));
    auto green = std::make_shared<Lambertian>(RGB::from_mag(.12, .45, .15));
    auto light = std::make_shared<DiffuseLight>(RGB::from_mag(1, 1, 1), 15);
    Scene world;
    world.add(std::make_shared<Parallelogram>(Point3D(555, 0, 0), Vec3D(0, 555, 0), Vec3D(0, 0, 555), green));
    world.add(std::make_shared<Parallelogram>(Point3D(0, 0, 0), Vec3D(0, 555, 0), Vec3D(0, 0, 555), red));
    world.add(std::make_shared<Parallelogram>(Point3D(343, 554, 332), Vec3D(-130, 0, 0), Vec3D(0, 0, -105), light));
    world.add(std::make_shared<Parallelogram>(Point3D(0, 0, 0), Vec3D(555, 0, 0), Vec3D(0, 0, 555), white));
    world.add(std::make_shared<Parallelogram>(Point3D(555, 555, 555), Vec3D(-555, 0, 0), Vec3D(0, 0, -555), white));
    world.add(std::make_shared<Parallelogram>(Point3D(0, 0, 555), Vec3D(555, 0, 0), Vec3D(0, 555, 0), white));
    world.add(std::make_shared<Box>(Point3D(130, 0, 65), Point3D(295, 165, 230), white));
    world.add(std::make_shared<Box>(Point3D(265, 0, 295), Point3D(430, 330, 460), white));
    BVH bvh(world);

    const Point3D eye(278, 400, 120);
    const RGB sky = RGB::from_mag(0.125, 0.25, 0.5);
    const uint32_t spp = 24;
    auto& seeds = SeedSeqGenerator::get_instance();
    size_t lit = 0, passes = 0;

    // 1. in passes to the end: render_lens' image
    const Lens lenses[2] = {Lens::fisheye(eye, Vec3D(0, 0, 1)), Lens::cube(eye, Vec3D(0, 0, 1))};
    const size_t dims[2][2] = {{40, 24}, {4, 24}};
    for (uint32_t i = 0; i < 2; ++i) {
        Camera cam;
        cam.set_image_dimensions(dims[i][0], dims[i][1]).set_samples_per_pixel(spp).set_max_depth(50).set_background(sky);
        seeds.set_seed(seed + i);
        const Image want = cam.render_lens(bvh, lenses[i]);
        seeds.set_seed(seed + i);
        size_t last = 0;
        const Image got = cam.render_lens_progressive(bvh, lenses[i], 8, [&](size_t done, size_t total) {
            if (total != spp || done != last + 8) std::exit(3);
            last = done;
            ++passes;
            return true;
        });
        if (last != spp || !same(got, want, dims[i][0], dims[i][1], i ? "cube in passes" : "fisheye in passes", &lit)) return 1;
    }

    // 2. stopped by on_pass after the second pass: the mean of 8 samples, as the C entry stopped alike
    size_t stopped = 0;
    {
        Camera cam;
        cam.set_image_dimensions(40, 24).set_samples_per_pixel(spp).set_max_depth(50).set_background(sky);
        seeds.set_seed(seed + 7);
        const Image got = cam.render_lens_progressive(world, lenses[0], 4, [&](size_t done, size_t) {
            stopped = done;
            return done < 8;
        });
        crt_camera c{};
        c.image_w = 40;
        c.image_h = 24;
        c.samples_per_pixel = spp;
        c.max_depth = 50;
        c.background[0] = sky.r;
        c.background[1] = sky.g;
        c.background[2] = sky.b;
        c.t_min = 1e-5;
        c.base_seed = static_cast<uint32_t>(2'483'477u * (seed + 7) + 2'987'434'823u);  // next_seed() after set_seed
        const crt_lens l = lenses[0].as_crt();
        crt_adaptive_params ap{};
        ap.min_samples = UINT32_MAX;
        ap.samples_per_pass = 4;
        std::vector<double> rgb(40 * 24 * 3, -1.0);
        uint64_t rendered = 0;
        auto stop = [](void*, uint32_t done, uint32_t, uint32_t, uint32_t, const double*, const double*) { return done >= 8 ? 1 : 0; };
        if (crt_render_lens_passes(bvh.gpu_scene().get(), 0, &c, &l, &ap, nullptr, stop, nullptr, nullptr, rgb.data(), nullptr,
                                   &rendered)) {
            std::cout << "crt_render_lens_passes: " << crt_last_error() << std::endl;
            return 1;
        }
        if (rendered != 8u * 40 * 24 || stopped != 8) return 1;
        for (size_t r = 0; r < 24; ++r)
            for (size_t col = 0; col < 40; ++col) {
                const double v[3] = {got[r][col].r, got[r][col].g, got[r][col].b};
                if (std::memcmp(v, &rgb[(r * 40 + col) * 3], sizeof v) != 0) {
                    std::cout << "stopped render: pixel " << r << " " << col << " differs" << std::endl;
                    return 1;
                }
            }
    }

    // 3. PINHOLE denoised is render_denoised, every sample and adaptive
    for (double threshold : {-1.0, 0.05}) {
        Camera cam;
        cam.set_image_dimensions(40, 24).set_samples_per_pixel(40).set_max_depth(50).set_background(sky);
        cam.set_camera_center(Point3D(278, 278, -800)).set_camera_lookat(Point3D(278, 278, 0)).set_vertical_fov(40);
        seeds.set_seed(seed + 11);
        const Image want = cam.render_denoised(bvh, DenoiseOptions{3, 7, 1, 0.05}, threshold);
        seeds.set_seed(seed + 11);
        const Image got = cam.render_lens_denoised(bvh, Lens::pinhole(), DenoiseOptions{3, 7, 1, 0.05}, threshold);
        if (!same(got, want, 40, 24, threshold < 0 ? "pinhole denoised" : "pinhole adaptive denoised", &lit)) return 1;
    }
    std::cout << "lens passes " << passes << " stopped " << stopped << " lit " << lit << std::endl;
    return 0;
}
