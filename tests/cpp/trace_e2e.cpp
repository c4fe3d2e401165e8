// BVH::hit_by_batch and BVH::occluded_batch (the drop-in's extensions over crt_trace) against
// BVH::hit_by called ray by ray, on a sphere world and a box room, 200 seeded rays each over two
// intervals. Prints "<world> <interval> hits <k> of <n>" per case and exits non-zero on the first
// difference (tests/test_gpu_trace_cpp.py).
//   trace_e2e <seed>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <vector>

#include "acceleration/bvh.h"
#include "base/scene.h"
#include "shapes/shapes.h"

static const double kInf = std::numeric_limits<double>::infinity();
static uint32_t lcg;
static double rnd(double lo, double hi) {
    lcg = lcg * 1664525u + 1013904223u;
    return lo + (hi - lo) * (static_cast<double>(lcg >> 8) / 16777216.0);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same_vec(const Vec3D& a, const Vec3D& b) {
    return same_bits(a.x, b.x) && same_bits(a.y, b.y) && same_bits(a.z, b.z);
}

static int check(const char* name, const BVH& bvh, const std::vector<Ray3D>& rays, const Interval& t) {
    const auto batch = bvh.hit_by_batch(rays, t);
    const auto occ = bvh.occluded_batch(rays, t);
    if (batch.size() != rays.size() || occ.size() != rays.size()) return 1;
    size_t hits = 0;
    for (size_t i = 0; i < rays.size(); ++i) {
        const auto one = bvh.hit_by(rays[i], t);
        if (one.has_value() != batch[i].has_value() || one.has_value() != occ[i]) {
            std::cout << name << ": ray " << i << " differs in being hit" << std::endl;
            return 1;
        }
        if (!one) continue;
        ++hits;
        const hit_info &a = *one, &b = *batch[i];
        if (!same_bits(a.hit_time, b.hit_time) || !same_vec(a.hit_point, b.hit_point) ||
            !same_vec(a.unit_surface_normal, b.unit_surface_normal) || a.hit_from_outside != b.hit_from_outside ||
            a.material != b.material) {
            std::cout << name << ": ray " << i << " differs in its record" << std::endl;
            return 1;
        }
    }
    std::cout << name << " (" << t.min << ", " << t.max << ") hits " << hits << " of " << rays.size() << std::endl;
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    lcg = static_cast<uint32_t>(std::strtoul(argv[1], nullptr, 10));
    auto grey = std::make_shared<Lambertian>(RGB::from_mag(0.5));
    auto metal = std::make_shared<Metal>(RGB::from_mag(0.8, 0.7, 0.6), 0.1);
    auto glass = std::make_shared<Dielectric>(1.5);

    Scene spheres;
    for (int i = 0; i < 60; ++i)
        spheres.add(std::make_shared<Sphere>(Point3D(rnd(-8, 8), rnd(-8, 8), rnd(-8, 8)), rnd(0.4, 1.5),
                                             i % 3 == 0 ? std::shared_ptr<Material>(grey)
                                                        : i % 3 == 1 ? std::shared_ptr<Material>(metal)
                                                                     : std::shared_ptr<Material>(glass)));
    Scene room;  // five walls and two boxes
    room.add(std::make_shared<Parallelogram>(Point3D(-10, -10, -10), Vec3D(20, 0, 0), Vec3D(0, 0, 20), grey));
    room.add(std::make_shared<Parallelogram>(Point3D(-10, 10, -10), Vec3D(20, 0, 0), Vec3D(0, 0, 20), grey));
    room.add(std::make_shared<Parallelogram>(Point3D(-10, -10, -10), Vec3D(0, 20, 0), Vec3D(0, 0, 20), metal));
    room.add(std::make_shared<Parallelogram>(Point3D(10, -10, -10), Vec3D(0, 20, 0), Vec3D(0, 0, 20), metal));
    room.add(std::make_shared<Parallelogram>(Point3D(-10, -10, -10), Vec3D(20, 0, 0), Vec3D(0, 20, 0), grey));
    room.add(std::make_shared<Box>(Point3D(-6, -10, -6), Point3D(-1, 2, -1), grey));
    room.add(std::make_shared<Box>(Point3D(2, -10, 0), Point3D(7, -4, 5), glass));

    std::vector<Ray3D> rays(200);
    for (auto& r : rays) {
        r.origin = Point3D(rnd(-9, 9), rnd(-9, 9), rnd(-9, 9));
        r.dir = Vec3D(rnd(-1, 1), rnd(-1, 1), rnd(-1, 1));
    }
    rays[7].dir = Vec3D(0, 0, 1);   // axis-aligned
    rays[8].dir = Vec3D(-2, 0, 0);
    BVH a(spheres), b(room);
    int rc = 0;
    rc |= check("spheres", a, rays, Interval(1e-5, kInf));
    rc |= check("spheres", a, rays, Interval(0.5, 6.0));
    rc |= check("room", b, rays, Interval(1e-5, kInf));
    rc |= check("room", b, rays, Interval(2.0, 9.0));
    return rc;
}
