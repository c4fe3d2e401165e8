// config1_e2e.cpp's scene at 100 x 56 and 12 spp, three times from the same seed: Camera::render,
// Camera::render_adaptive (the drop-in's extension over crt_render_adaptive) with min_samples =
// samples_per_pixel, which never stops a block, and render_adaptive with a stopping rule that the
// sky's blocks meet. The first two PPMs are equal byte for byte
// (tests/test_gpu_adaptive_cpp.py).
//   adaptive_e2e <seed> <render.ppm> <never_stop.ppm> <adaptive.ppm>
#include <cstdlib>
#include <iostream>
#include <memory>

#include "base/camera.h"
#include "base/scene.h"
#include "shapes/shapes.h"
#include "util/rand_util.h"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const auto seed = static_cast<uint32_t>(std::strtoul(argv[1], nullptr, 10));
    Scene world;
    world.add(std::make_shared<Sphere>(Point3D(0, -1000, 0), 1000, std::make_shared<Lambertian>(RGB::from_mag(0.5))));
    world.add(std::make_shared<Sphere>(Point3D(0, 1, 0), 1, std::make_shared<Lambertian>(RGB::from_mag(0.4, 0.2, 0.1))));
    Camera cam;
    cam.set_image_by_width_and_aspect_ratio(100, 16. / 9.)
        .set_vertical_fov(20)
        .set_camera_center(Point3D(13, 2, 3))
        .set_camera_lookat(Point3D(0, 0, 0))
        .set_samples_per_pixel(12)
        .set_max_depth(50)
        .set_background(RGB::from_mag(0.7, 0.8, 1));
    SeedSeqGenerator::get_instance().set_seed(seed);
    cam.render(world).send_as_ppm(argv[2]);

    size_t passes = 0, last_active = 0;
    auto on_pass = [&](size_t done, size_t total, size_t active, size_t blocks) {
        ++passes;
        last_active = active;
        std::cout << "pass " << passes << ": " << done << " / " << total << " spp, " << active << " of " << blocks
                  << " blocks active" << std::endl;
        return true;
    };
    SeedSeqGenerator::get_instance().set_seed(seed);
    cam.render_adaptive(world, 0.0, 12, 4, on_pass).send_as_ppm(argv[3]);
    if (passes != 3 || last_active == 0) return 3;  // three passes of 4, no block stopped

    passes = 0;
    SeedSeqGenerator::get_instance().set_seed(seed);
    cam.render_adaptive(world, 0.05, 8, 4, on_pass).send_as_ppm(argv[4]);
    return passes >= 2 && passes <= 3 ? 0 : 4;
}
