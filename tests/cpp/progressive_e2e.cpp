// config1_e2e.cpp's scene rendered in passes: Camera::render_progressive (the drop-in's
// extension over crt_render_progressive) and Image::send_as_ppm. Rendered to the end, the PPM
// bytes equal config1_e2e's (tests/test_gpu_progressive_cpp.py).
//   progressive_e2e <seed> <out.ppm>
#include <cstdlib>
#include <iostream>
#include <memory>

#include "base/camera.h"
#include "base/scene.h"
#include "shapes/shapes.h"
#include "util/rand_util.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    SeedSeqGenerator::get_instance().set_seed(static_cast<uint32_t>(std::strtoul(argv[1], nullptr, 10)));
    Scene world;
    world.add(std::make_shared<Sphere>(Point3D(0, -1000, 0), 1000, std::make_shared<Lambertian>(RGB::from_mag(0.5))));
    world.add(std::make_shared<Sphere>(Point3D(0, 1, 0), 1, std::make_shared<Lambertian>(RGB::from_mag(0.4, 0.2, 0.1))));
    size_t passes = 0;
    Camera()
        .set_image_by_width_and_aspect_ratio(400, 16. / 9.)
        .set_vertical_fov(20)
        .set_camera_center(Point3D(13, 2, 3))
        .set_camera_lookat(Point3D(0, 0, 0))
        .set_samples_per_pixel(1)
        .set_max_depth(50)
        .set_background(RGB::from_mag(0.7, 0.8, 1))
        .render_progressive(world, 0, [&](size_t done, size_t total, double) {
            ++passes;
            std::cout << "pass " << passes << ": " << done << " / " << total << " spp" << std::endl;
            return true;
        })
        .send_as_ppm(argv[2]);
    return passes == 1 ? 0 : 3;  // 1 spp is one (ragged) chunk: one pass
}
