"""CPU-side checks of the progressive-render entry points: the chunk length, the Python binding,
the checkpoint guard of ProgressiveRender.resume, and the C++ drop-in's render_progressive
compiling and linking. No kernel runs here (tests/test_gpu_progressive.py runs them)."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
NEW = ("crt_sample_chunk_len", "crt_render_pass_async", "crt_noise_estimate", "crt_render_progressive")


@pytest.mark.parametrize("spp,want", [(1, 4), (22, 4), (768, 4), (769, 5), (1000, 6)])
def test_sample_chunk_len(crt, spp, want):
    # launch_render: chunk_len = max(4, (spp + 191) / 192)
    assert crt.sample_chunk_len(spp) == want
    assert crt.lib().crt_sample_chunk_len(spp) == want


def test_exports_contain_progressive_entry_points(crt):
    from cpp_raytracer_amd._capi import EXPORTS, PROGRESS_FN
    for name in NEW:
        assert name in EXPORTS
        assert hasattr(crt.lib(), name)
    assert EXPORTS["crt_render_progressive"][1][5] is PROGRESS_FN
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays


def _state(cam, **over):
    s = {"sum": np.zeros((cam.image_h, cam.image_w, 3)), "noise": np.zeros((cam.image_h, cam.image_w, 2)),
         "samples_done": 8, "spp": int(cam.samples_per_pixel), "base_seed": int(cam.base_seed),
         "width": int(cam.image_w), "height": int(cam.image_h), "tiling": np.array([1, 1, 0, 0], np.uint32)}
    s.update(over)
    return s


@pytest.mark.parametrize("over", [dict(spp=24), dict(base_seed=6), dict(width=51), dict(height=31),
                                  dict(samples_done=7), dict(samples_done=23), dict(sum=np.zeros((30, 49, 3)))])
def test_resume_rejects_a_state_of_another_job(crt, over):
    """A checkpoint continues only the job it was taken from: other samples per pixel (another
    chunking), another seed or frame size, or a samples_done off the pass boundaries is refused
    before anything touches a device."""
    from cpp_raytracer_amd import camera_with
    from cpp_raytracer_amd.progressive import ProgressiveRender
    d = crt.SceneData.named("config1")
    d.camera = camera_with(d.camera, image_w=50, image_h=30, samples_per_pixel=22)
    scene = crt.GpuScene(d)
    cam = crt.resolve_camera(d.camera, 5)
    with pytest.raises(crt.CrtError, match="resume"):
        ProgressiveRender.resume(scene, cam, _state(cam, **over))


def test_pass_rules_are_checked_before_any_device_work(crt):
    """crt_render_pass_async names the broken rule; the checks come before the device is looked
    at, so they hold on a machine without one."""
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named("config1")
    d.camera = camera_with(d.camera, image_w=50, image_h=30, samples_per_pixel=22)
    scene = crt.GpuScene(d)
    cam = crt.resolve_camera(d.camera, 5)
    fake = 4096  # never dereferenced: every call below is refused
    for first, count, ptr, word in [(2, 4, fake, "multiple of the chunk length"), (0, 0, fake, "num_samples is 0"),
                                    (20, 4, fake, "exceeds samples_per_pixel"), (0, 6, fake, "neither a multiple"),
                                    (0, 8, 0, "d_sum is null")]:
        with pytest.raises(crt.CrtError, match=word):
            scene.render_pass(0, cam, first, count, ptr)


def test_progressive_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "progressive_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "progressive_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
