// denoise_e2e.cpp's adaptive job (config1_e2e.cpp's scene at 100 x 56 and 12 spp, threshold 0.05,
// options of its own) through Camera::render_denoised with devices = 0: rendered over all visible
// devices (CRT_EMULATE_DEVICES=3 in tests/test_gpu_denoise_devices_cpp.py) and filtered on device
// 0 (crt_render_denoised_devices). The PPM equals Image::send_as_ppm's integers of the Python
// path's denoised frame on one device.
//   denoise_devices_e2e <seed> <adaptive.ppm>
#include <cstdlib>
#include <iostream>
#include <memory>

#include "base/camera.h"
#include "base/scene.h"
#include "shapes/shapes.h"
#include "util/rand_util.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
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
    DenoiseOptions opt;
    opt.iterations = 3;
    opt.normal_squarings = 5;
    opt.sigma_l = 3;
    opt.sigma_p = 0.1;
    SeedSeqGenerator::get_instance().set_seed(seed);
    cam.render_denoised(world, opt, 0.05, 0).send_as_ppm(argv[2]);
    return 0;
}
