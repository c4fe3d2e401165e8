// Camera::probes (the drop-in's extension over crt_probes) against crt_probes called directly on the
// same BVH, for 8 points on the floor of the Cornell box (src/main.cpp:326-363) in both modes, 256
// samples a probe, with the seed the camera takes from the SeedSeqGenerator. Prints
// "probes <n> sphere <k> hemisphere <m>" (the probes with a non-zero first coefficient) and exits
// non-zero on the first differing byte (tests/test_gpu_probes_cpp.py).
//   probes_e2e <seed>
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

    const size_t n = 8;
    const uint32_t samples = 256;
    std::vector<Point3D> points;
    std::vector<Vec3D> normals;
    for (size_t i = 0; i < n; ++i) {  // a row of floor points in front of the boxes, lifted off the floor
        points.push_back(Point3D(40 + 65.0 * static_cast<double>(i), 1e-3, 30));
        normals.push_back(Vec3D(0, 1, 0));
    }
    const RGB sky = RGB::from_mag(0.125, 0.25, 0.5);
    Camera cam;
    cam.set_max_depth(50).set_background(sky);

    size_t lit[2] = {0, 0};
    for (uint32_t mode : {CRT_PROBE_SPHERE, CRT_PROBE_HEMISPHERE}) {
        const size_t K = mode == CRT_PROBE_SPHERE ? 9 : 1;
        SeedSeqGenerator::get_instance().set_seed(seed + mode);
        const std::vector<RGB> got =
            cam.probes(bvh, points, mode == CRT_PROBE_HEMISPHERE ? normals : std::vector<Vec3D>{}, samples, mode);
        if (got.size() != n * K) return 1;

        crt_probe_params p{};
        p.samples = samples;
        p.max_depth = 50;
        p.base_seed = static_cast<uint32_t>(2'483'477u * (seed + mode) + 2'987'434'823u);  // next_seed() after set_seed
        p.mode = mode;
        p.background[0] = sky.r;
        p.background[1] = sky.g;
        p.background[2] = sky.b;
        p.t_min = 1e-5;
        std::vector<double> pts(3 * n), nrm(3 * n), coeff(3 * n * K, -1.0);
        for (size_t i = 0; i < n; ++i)
            for (size_t k = 0; k < 3; ++k) {
                pts[3 * i + k] = points[i][k];
                nrm[3 * i + k] = normals[i][k];
            }
        if (crt_probes(bvh.gpu_scene().get(), 0, pts.data(), mode == CRT_PROBE_HEMISPHERE ? nrm.data() : nullptr, n, &p,
                       coeff.data())) {
            std::cout << "crt_probes: " << crt_last_error() << std::endl;
            return 1;
        }
        for (size_t i = 0; i < n * K; ++i) {
            const double c[3] = {got[i].r, got[i].g, got[i].b};
            if (std::memcmp(c, &coeff[3 * i], sizeof c) != 0) {
                std::cout << "mode " << mode << " coefficient " << i << " differs" << std::endl;
                return 1;
            }
        }
        for (size_t i = 0; i < n; ++i)
            if (got[i * K].r > 0 && got[i * K].g > 0 && got[i * K].b > 0) ++lit[mode];
    }
    std::cout << "probes " << n << " sphere " << lit[0] << " hemisphere " << lit[1] << std::endl;
    return 0;
}
