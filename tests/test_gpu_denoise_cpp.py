"""Camera::render_denoised of the C++ drop-in end to end on the GPU: tests/cpp/denoise_e2e.cpp
renders config1_e2e.cpp's scene at 100 x 56 and 12 spp through it, every sample with the default
options and adaptively with options of its own, and writes both with Image::send_as_ppm. Each PPM
equals the integers crt_ppm_values gives for the Python path's denoised frame of the same job."""
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
SEED = 4155677120  # tests/test_gpu_cpp_e2e.py: the render's base seed is then 7


def ppm_of(crt, frame, path):
    import torch
    t = torch.from_numpy(frame).cuda()
    crt.write_ppm(path, crt.ppm_values(0, t.data_ptr(), frame.shape[0], frame.shape[1]))
    return path.read_bytes()


def test_denoised_ppms_equal_the_python_paths(crt, tmp_path):
    from cpp_raytracer_amd import camera_with
    exe = tmp_path / "denoise_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "denoise_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    outs = [tmp_path / f"{n}.ppm" for n in ("plain", "adaptive")]
    r = subprocess.run([str(exe), str(SEED), *map(str, outs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    print(r.stdout[-1200:])
    assert "Rendered 12 spp on average (of 12), denoised" in r.stdout
    plain, adaptive = (p.read_bytes() for p in outs)
    assert plain.startswith(b"P3\n100 56\n255\n") and adaptive.startswith(b"P3\n100 56\n255\n")

    d = crt.SceneData.named("config1")
    d.camera = camera_with(d.camera, image_w=100, image_h=56, samples_per_pixel=12)
    s = crt.GpuScene(d)
    cam = crt.resolve_camera(d.camera, 7)
    den, raw, _ = s.render_denoised(cam, crt.denoise_params(), noisy=True)  # both bindings' defaults
    assert plain == ppm_of(crt, den, tmp_path / "py_plain.ppm")
    assert plain != ppm_of(crt, raw, tmp_path / "py_raw.ppm")  # the filter changed the picture
    # render_denoised(world, opt, 0.05): passes of a tenth of 12 samples, rounded up to a chunk of 4; a floor of two passes
    den, _, rendered = s.render_denoised(cam, crt.denoise_params(3, 5, 3.0, 0.1), threshold=0.05, min_samples=8)
    assert adaptive == ppm_of(crt, den, tmp_path / "py_adaptive.ppm")
    assert 8 * 100 * 56 <= rendered < 12 * 100 * 56  # the sky's blocks stopped at the floor
