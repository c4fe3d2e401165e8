// The drop-in's three calls under a Lighting (Camera::render_lens, render_lens_progressive and
// render_lens_denoised with an Environment and the world's Lights) against the two blocking entries
// they go over, crt_render_lens_lit and crt_render_lens_passes_lit, called directly on the same BVH: a
// 4 x 24 cube map from the middle of the Cornell box (src/main.cpp:326-363), 16 samples a pixel, under a
// 2 x 12 map with one bright texel, sampled (importance) and plain, with the seed the camera takes from
// the SeedSeqGenerator. Prints "<what> differs <k> of <n>" (the pixels that differ from the frame with
// the lights alone) and exits non-zero on the first byte that differs (tests/test_gpu_lighting_cpp.py).
//   lighting_e2e <seed>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "acceleration/bvh.h"
#include "base/camera.h"
#include "base/scene.h"
#include "shapes/shapes.h"

static bool equal(const Image& got, const std::vector<double>& want, size_t w, size_t h, const char* what) {
    for (size_t r = 0; r < h; ++r)
        for (size_t col = 0; col < w; ++col) {
            const RGB& p = got[r][col];
            const double v[3] = {p.r, p.g, p.b};
            if (std::memcmp(v, &want[(r * w + col) * 3], sizeof v) != 0) {
                std::cout << what << ": pixel " << r << " " << col << " differs" << std::endl;
                return false;
            }
        }
    return true;
}

static size_t differing(const std::vector<double>& a, const std::vector<double>& b) {
    size_t k = 0;
    for (size_t i = 0; i < a.size(); i += 3)
        if (std::memcmp(&a[i], &b[i], 3 * sizeof(double)) != 0) ++k;
    return k;
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
    const uint32_t spp = 16;
    const size_t w = 4, h = 24;
    const Lens lens = Lens::cube(eye, Vec3D(0, 0, 1));
    const Lights lights = Lights::of(bvh);
    auto sky_map = Image::with_dimensions(2, 12);
    for (size_t r = 0; r < 12; ++r)
        for (size_t c = 0; c < 2; ++c) sky_map[r][c] = RGB::from_mag(0.25 + 0.125 * r, 0.5, 1.0 - 0.0625 * c);
    sky_map[11][1] = RGB::from_mag(400, 300, 200);  // one bright texel for the sampler to find
    Camera cam;
    cam.set_image_dimensions(w, h).set_samples_per_pixel(spp).set_max_depth(50).set_background(sky);

    if (argc > 2 && std::string(argv[2]) == "foreign") {  // Lights of another world: the call dies with a message
        Scene other;
        other.add(std::make_shared<Sphere>(Point3D(0, 0, 0), 1.0, light));
        BVH other_bvh(other);
        const Lights foreign = Lights::of(other_bvh);
        const Lighting lit{nullptr, &foreign};
        (void)cam.render_lens_progressive(bvh, lens, lit);
        return 0;  // not reached
    }

    crt_camera c{};  // the fields a non-pinhole lens render reads
    c.image_w = static_cast<uint32_t>(w);
    c.image_h = static_cast<uint32_t>(h);
    c.samples_per_pixel = spp;
    c.max_depth = 50;
    c.background[0] = sky.r;
    c.background[1] = sky.g;
    c.background[2] = sky.b;
    c.t_min = 1e-5;
    c.base_seed = static_cast<uint32_t>(2'483'477u * seed + 2'987'434'823u);  // next_seed() after set_seed
    const crt_lens l = lens.as_crt();
    std::vector<double> only(w * h * 3, -1.0);
    if (crt_render_lens_lights(bvh.gpu_scene().get(), 0, &c, &l, only.data())) {
        std::cout << "crt_render_lens_lights: " << crt_last_error() << std::endl;
        return 1;
    }
    for (const bool importance : {true, false}) {
        const Environment env = Environment::from_cube(sky_map, Vec3D(0, 0, -1), Vec3D(0, 1, 0), CRT_ENV_NEAREST, importance);
        const Lighting lit{&env, &lights};
        const crt_env e = env.as_crt();
        const std::string tag = importance ? "sampled" : "plain";
        std::vector<double> rgb(w * h * 3, -1.0), den(w * h * 3, -1.0);
        if (crt_render_lens_lit(bvh.gpu_scene().get(), 0, &c, &l, &e, importance ? 1 : 0, 1, rgb.data())) {
            std::cout << "crt_render_lens_lit: " << crt_last_error() << std::endl;
            return 1;
        }
        SeedSeqGenerator::get_instance().set_seed(seed);
        if (!equal(cam.render_lens(bvh, lens, lit), rgb, w, h, "render_lens")) return 1;
        std::cout << tag << " render_lens differs " << differing(rgb, only) << " of " << w * h << std::endl;
        // passes rendered to the end are the one-shot frame, bit for bit
        size_t passes = 0;
        SeedSeqGenerator::get_instance().set_seed(seed);
        const Image prog = cam.render_lens_progressive(bvh, lens, lit, 4, [&](size_t, size_t) { return ++passes, true; });
        if (!equal(prog, rgb, w, h, "render_lens_progressive")) return 1;
        std::cout << tag << " render_lens_progressive passes " << passes << std::endl;
        // denoised: crt_render_lens_passes_lit with the options' parameters
        const DenoiseOptions opt{};
        crt_denoise_params dp{};
        dp.iterations = opt.iterations;
        dp.normal_squarings = opt.normal_squarings;
        dp.sigma_l = opt.sigma_l;
        dp.sigma_p = opt.sigma_p;
        uint64_t rendered = 0;
        if (crt_render_lens_passes_lit(bvh.gpu_scene().get(), 0, &c, &l, &e, importance ? 1 : 0, 1, nullptr, &dp, nullptr, nullptr,
                                       nullptr, den.data(), nullptr, &rendered)) {
            std::cout << "crt_render_lens_passes_lit: " << crt_last_error() << std::endl;
            return 1;
        }
        SeedSeqGenerator::get_instance().set_seed(seed);
        if (!equal(cam.render_lens_denoised(bvh, lens, lit, opt), den, w, h, "render_lens_denoised")) return 1;
        std::cout << tag << " render_lens_denoised differs " << differing(den, rgb) << " of " << w * h << std::endl;
        if (rendered != static_cast<uint64_t>(spp) * w * h) return 1;
    }
    // a Lighting with nothing set is the call without one
    std::vector<double> flat(w * h * 3, -1.0);
    if (crt_render_lens(bvh.gpu_scene().get(), 0, &c, &l, flat.data())) return 1;
    SeedSeqGenerator::get_instance().set_seed(seed);
    if (!equal(cam.render_lens(bvh, lens, Lighting{}), flat, w, h, "render_lens, nothing set")) return 1;
    std::cout << "nothing set equals crt_render_lens" << std::endl;
    return 0;
}
