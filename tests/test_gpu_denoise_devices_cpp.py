"""Camera::render_denoised over several devices end to end on the GPU: tests/cpp/denoise_devices_e2e.cpp
renders tests/cpp/denoise_e2e.cpp's adaptive job (config1_e2e.cpp's scene at 100 x 56 and 12 spp)
through render_denoised(world, opt, 0.05, 0) in a C++ process with CRT_EMULATE_DEVICES=3 and writes
it with Image::send_as_ppm. The PPM equals the integers crt_ppm_values gives for the Python path's
denoised frame of the same job, on one device and over three emulated ones."""
import os
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


def test_denoised_ppm_over_three_devices_equals_the_python_paths(crt, tmp_path, monkeypatch):
    from cpp_raytracer_amd import camera_with
    exe = tmp_path / "denoise_devices_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "denoise_devices_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    out = tmp_path / "adaptive.ppm"
    r = subprocess.run([str(exe), str(SEED), str(out)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "CRT_EMULATE_DEVICES": "3"})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    print(r.stdout[-1200:])
    assert "(up to 12 spp, adaptive, denoised) on 3 GPUs" in r.stdout
    got = out.read_bytes()
    assert got.startswith(b"P3\n100 56\n255\n")

    d = crt.SceneData.named("config1")
    d.camera = camera_with(d.camera, image_w=100, image_h=56, samples_per_pixel=12)
    s = crt.GpuScene(d)
    cam = crt.resolve_camera(d.camera, 7)
    prm = crt.denoise_params(3, 5, 3.0, 0.1)
    # render_denoised(world, opt, 0.05, 0): passes of a tenth of 12 samples, rounded up to a chunk of 4; a floor of two passes
    den, raw, rendered = s.render_denoised(cam, prm, threshold=0.05, min_samples=8, noisy=True)
    assert 8 * 100 * 56 <= rendered < 12 * 100 * 56  # the sky's blocks stopped at the floor
    assert got == ppm_of(crt, den, tmp_path / "py_one.ppm")
    assert got != ppm_of(crt, raw, tmp_path / "py_raw.ppm")  # the filter changed the picture
    monkeypatch.setenv("CRT_EMULATE_DEVICES", "3")
    den3, _, rendered3 = s.render_denoised(cam, prm, threshold=0.05, min_samples=8, num_devices=0)
    assert rendered3 == rendered
    assert got == ppm_of(crt, den3, tmp_path / "py_three.ppm")
