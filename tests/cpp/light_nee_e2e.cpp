// Camera::render_lens(world, lens, lights) (the drop-in's extension over crt_render_lens_lights) against
// crt_render_lens_lights called directly on the same BVH: a 4 x 24 cube map from the middle of the
// Cornell box (src/main.cpp:326-363), 16 samples a pixel, with the seed the camera takes from the
// SeedSeqGenerator. Prints "lights differs <k> of <n>" (the pixels that differ from the unsampled frame
// of crt_render_lens) and exits non-zero on the first byte that differs between the two sampled frames
// (tests/test_gpu_light_nee_cpp.py).
//   light_nee_e2e <seed>
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
    Camera cam;
    cam.set_image_dimensions(w, h).set_samples_per_pixel(spp).set_max_depth(50).set_background(sky);
    SeedSeqGenerator::get_instance().set_seed(seed);
    const Image got = cam.render_lens(bvh, lens, lights);

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
    std::vector<double> rgb(w * h * 3, -1.0), flat(w * h * 3, -1.0);
    if (crt_render_lens_lights(bvh.gpu_scene().get(), 0, &c, &l, rgb.data()) ||
        crt_render_lens(bvh.gpu_scene().get(), 0, &c, &l, flat.data())) {
        std::cout << "crt_render_lens(_lights): " << crt_last_error() << std::endl;
        return 1;
    }
    size_t differs = 0;
    for (size_t r = 0; r < h; ++r)
        for (size_t col = 0; col < w; ++col) {
            const RGB& p = got[r][col];
            const double v[3] = {p.r, p.g, p.b};
            if (std::memcmp(v, &rgb[(r * w + col) * 3], sizeof v) != 0) {
                std::cout << "pixel " << r << " " << col << " differs" << std::endl;
                return 1;
            }
            if (std::memcmp(v, &flat[(r * w + col) * 3], sizeof v) != 0) ++differs;
        }
    std::cout << "lights differs " << differs << " of " << w * h << std::endl;
    return 0;
}
