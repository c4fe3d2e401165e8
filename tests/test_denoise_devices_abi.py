"""CPU-side checks of crt_render_denoised_devices: the export, and every argument rule, refused
with CRT_E_INVALID and a message naming it before any device work (so they hold on a machine
without a GPU: a call that got as far as looking for a device would fail with CRT_E_NODEVICE
instead). No kernel runs here (tests/test_gpu_denoise_devices.py runs them)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
W, H = 50, 30
POISON = 0xDEADBEEF


def test_export_and_callback_type(crt):
    from cpp_raytracer_amd import _capi
    assert "crt_render_denoised_devices" in _capi.EXPORTS
    assert hasattr(crt.lib(), "crt_render_denoised_devices")
    res, args = _capi.EXPORTS["crt_render_denoised_devices"]
    assert res is C.c_int and len(args) == 11 and args[5] is _capi.DENOISED_FN
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays


@pytest.fixture
def job(crt):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named("config1")
    d.camera = camera_with(d.camera, image_w=W, image_h=H, samples_per_pixel=22)
    return crt.GpuScene(d), crt.resolve_camera(d.camera, 5)


def params(crt, **over):
    p = crt.denoise_params(5, 7, 1.0, 0.05)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def refused(crt, word, scene, cam, adaptive, denoise, out):
    """The call fails with CRT_E_INVALID naming `word`, and *samples_rendered is zeroed."""
    from cpp_raytracer_amd import _capi
    rendered = C.c_uint64(POISON)
    rc = crt.lib().crt_render_denoised_devices(scene, C.byref(cam) if cam is not None else None, 3,
                                               C.byref(adaptive) if adaptive is not None else None,
                                               C.byref(denoise) if denoise is not None else None, _capi.DENOISED_FN(),
                                               None, None, out, None, C.byref(rendered))
    msg = crt.lib().crt_last_error()
    assert rc == -1, (rc, msg)
    assert word in msg, msg
    assert b"crt_render_denoised_devices" in msg
    assert rendered.value == 0


def test_null_arguments(crt, job):
    scene, cam = job
    out = np.zeros((H, W, 3))
    ok = params(crt)
    refused(crt, b"null argument", None, cam, None, ok, out.ctypes.data)
    refused(crt, b"null argument", scene.handle, None, None, ok, out.ctypes.data)
    refused(crt, b"h_rgb is null", scene.handle, cam, None, ok, None)
    refused(crt, b"parameters are null", scene.handle, cam, None, None, out.ctypes.data)


BAD_PARAMS = [
    (dict(iterations=0), b"iterations = 0 is outside 1..8"), (dict(iterations=9), b"iterations = 9 is outside 1..8"),
    (dict(normal_squarings=11), b"normal_squarings = 11 is outside 0..10"),
    (dict(sigma_l=0.0), b"sigma_l must be finite and > 0"), (dict(sigma_l=float("nan")), b"sigma_l must be finite and > 0"),
    (dict(sigma_p=-0.5), b"sigma_p must be finite and > 0"), (dict(sigma_p=float("inf")), b"sigma_p must be finite and > 0"),
    (dict(flags=1), b"denoise flags must be 0"), (dict(reserved=7), b"denoise reserved must be 0"),
]


@pytest.mark.parametrize("over,word", BAD_PARAMS, ids=[f"{next(iter(o))}={next(iter(o.values()))}" for o, _ in BAD_PARAMS])
def test_denoise_parameter_rules(crt, job, over, word):
    scene, cam = job
    out = np.zeros((H, W, 3))
    refused(crt, word, scene.handle, cam, None, params(crt, **over), out.ctypes.data)


def test_adaptive_parameter_rules(crt, job):
    from cpp_raytracer_amd import _capi
    scene, cam = job
    out = np.zeros((H, W, 3))
    ok = params(crt)
    for prm, word in [(_capi.AdaptiveParams(0.1, 8, 8, 1, 0), b"unknown adaptive flags"),  # CRT_PROGRESS_NOISE
                      (_capi.AdaptiveParams(0.1, 8, 8, 3, 0), b"unknown adaptive flags"),
                      (_capi.AdaptiveParams(0.1, 8, 8, 4, 0), b"unknown adaptive flags"),
                      (_capi.AdaptiveParams(0.1, 8, 8, 0, 1), b"adaptive reserved must be 0"),
                      (_capi.AdaptiveParams(0.1, 8, 8, 2, 9), b"adaptive reserved must be 0"),
                      (_capi.AdaptiveParams(-1.0, 8, 8, 0, 0), b"threshold must be finite"),
                      (_capi.AdaptiveParams(float("nan"), 8, 8, 2, 0), b"threshold must be finite"),
                      (_capi.AdaptiveParams(float("inf"), 8, 8, 0, 0), b"threshold must be finite")]:
        refused(crt, word, scene.handle, cam, prm, ok, out.ctypes.data)


def test_job_rules(crt, job):
    from cpp_raytracer_amd import _capi
    scene, cam = job
    out = np.zeros((H, W, 3))
    ok = params(crt)
    ad = _capi.AdaptiveParams(0.1, 8, 8, _capi.CRT_PROGRESS_PREVIEW, 0)
    for field, value, word in [("samples_per_pixel", 0, b"samples_per_pixel is 0"), ("image_w", 0, b"empty image"),
                               ("image_h", 0, b"empty image"), ("samples_per_pixel", 1 << 31, b"below 2^31")]:
        bad = _capi.Camera.from_buffer_copy(bytes(cam))
        setattr(bad, field, value)
        for adaptive in (None, ad):
            refused(crt, word, scene.handle, bad, adaptive, ok, out.ctypes.data)


def test_python_binding_rules(crt, job):
    scene, cam = job
    with pytest.raises(crt.CrtError, match="device must be 0"):
        scene.render_denoised(cam, device=1, num_devices=2)
    with pytest.raises(crt.CrtError, match="preview needs an adaptive render"):
        scene.render_denoised(cam, num_devices=2, preview=True, callback=lambda *a: 0)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*iterations = 0"):
        scene.render_denoised(cam, params(crt, iterations=0), num_devices=3)


def test_denoise_devices_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "denoise_devices_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "denoise_devices_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
