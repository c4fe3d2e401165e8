// Camera::ray_colors (the drop-in's extension over crt_radiance) against crt_radiance called directly
// on the same BVH, for 4096 seeded rays inside the Cornell box (src/main.cpp:326-363) with explicit LCG
// states. Prints "lit <k> dark <m> of <n>" and exits non-zero on the first differing byte
// (tests/test_gpu_radiance_cpp.py).
//   radiance_e2e <seed>
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

static uint32_t lcg;
static double rnd(double lo, double hi) {
    lcg = lcg * 1664525u + 1013904223u;
    return lo + (hi - lo) * (static_cast<double>(lcg >> 8) / 16777216.0);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    lcg = static_cast<uint32_t>(std::strtoul(argv[1], nullptr, 10));
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

    const size_t n = 4096;
    std::vector<Ray3D> rays(n);
    std::vector<uint32_t> states(n);
    for (size_t i = 0; i < n; ++i) {
        rays[i].origin = Point3D(rnd(5, 550), rnd(5, 550), rnd(-300, 550));  // some start outside, in the dark
        rays[i].dir = Vec3D(rnd(-1, 1), rnd(-1, 1), rnd(-1, 1));
        lcg = lcg * 1664525u + 1013904223u;
        states[i] = lcg;
    }
    rays[9].dir = Vec3D(0, 0, 0);  // outside the contract: the background
    const RGB sky = RGB::from_mag(0.125, 0.25, 0.5);
    Camera cam;
    cam.set_max_depth(50).set_background(sky);
    const std::vector<RGB> colors = cam.ray_colors(rays, states, bvh);
    if (colors.size() != n) return 1;

    crt_radiance_params p{};
    p.max_depth = 50;
    p.background[0] = sky.r;
    p.background[1] = sky.g;
    p.background[2] = sky.b;
    p.t_min = 1e-5;
    const std::vector<double> r = BVH::crt_rays(rays);
    std::vector<double> rgb(3 * n, -1.0);
    if (crt_radiance(bvh.gpu_scene().get(), 0, r.data(), n, states.data(), &p, rgb.data())) {
        std::cout << "crt_radiance: " << crt_last_error() << std::endl;
        return 1;
    }
    size_t lit = 0, dark = 0;
    for (size_t i = 0; i < n; ++i) {
        const double c[3] = {colors[i].r, colors[i].g, colors[i].b};
        if (std::memcmp(c, &rgb[3 * i], sizeof c) != 0) {
            std::cout << "path " << i << " differs" << std::endl;
            return 1;
        }
        if (c[0] == 0 && c[1] == 0 && c[2] == 0) ++dark;
        else ++lit;
    }
    if (colors[9].r != sky.r || colors[9].g != sky.g || colors[9].b != sky.b) {
        std::cout << "the ray without a direction did not see the background" << std::endl;
        return 1;
    }
    if (cam.ray_colors(rays, {}, bvh).size() != n) return 1;  // default seeding
    std::cout << "lit " << lit << " dark " << dark << " of " << n << std::endl;
    return 0;
}
