"""CPU-side checks of the denoising entry points: the exports, the struct mirrors, and every
argument rule, refused with CRT_E_INVALID and a message naming it before any device work (so they
hold on a machine without a GPU: a call that got as far as looking for a device would fail with
CRT_E_NODEVICE instead). No kernel runs here (tests/test_gpu_denoise.py runs them)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
NEW = ("crt_render_features_async", "crt_pixel_variance_async", "crt_denoise_async", "crt_render_denoised")
FAKE = 1 << 20  # device pointers that are never dereferenced: every call given them is refused first
W, H = 50, 30


def test_exports_and_struct_mirrors(crt):
    from cpp_raytracer_amd import _capi
    for name in NEW:
        assert name in _capi.EXPORTS
        assert hasattr(crt.lib(), name)
    assert C.sizeof(_capi.Feature) == 88 and crt.FEATURE_DTYPE.itemsize == 88
    for (name, _), field in zip(_capi.Feature._fields_, crt.FEATURE_DTYPE.names):
        assert name == field
        assert getattr(_capi.Feature, name).offset == crt.FEATURE_DTYPE.fields[name][1]
        assert getattr(_capi.Feature, name).size == crt.FEATURE_DTYPE.fields[name][0].itemsize
    assert C.sizeof(_capi.DenoiseParams) == 32
    assert [f for f, _ in _capi.DenoiseParams._fields_] == ["iterations", "normal_squarings", "sigma_l", "sigma_p",
                                                           "flags", "reserved"]
    p = crt.denoise_params()
    assert (p.iterations, p.normal_squarings, p.flags, p.reserved) == (5, 7, 0, 0) and p.sigma_l > 0 and p.sigma_p > 0
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays


@pytest.fixture
def job(crt):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named("config1")
    d.camera = camera_with(d.camera, image_w=W, image_h=H, samples_per_pixel=22)
    return crt.GpuScene(d), crt.resolve_camera(d.camera, 5)


def buffers():
    """Disjoint fake device addresses: rgb, var, feat, out, var_out."""
    n = W * H
    rgb = FAKE
    var = rgb + n * 24
    feat = var + n * 8
    out = feat + n * 88
    var_out = out + n * 24
    return rgb, var, feat, out, var_out


BAD_PARAMS = [
    (dict(iterations=0), "iterations = 0 is outside 1..8"), (dict(iterations=9), "iterations = 9 is outside 1..8"),
    (dict(normal_squarings=11), "normal_squarings = 11 is outside 0..10"),
    (dict(sigma_l=0.0), "sigma_l must be finite and > 0"), (dict(sigma_l=-1.0), "sigma_l must be finite and > 0"),
    (dict(sigma_l=float("nan")), "sigma_l must be finite and > 0"), (dict(sigma_l=float("inf")), "sigma_l must be finite and > 0"),
    (dict(sigma_p=0.0), "sigma_p must be finite and > 0"), (dict(sigma_p=-0.5), "sigma_p must be finite and > 0"),
    (dict(sigma_p=float("nan")), "sigma_p must be finite and > 0"), (dict(sigma_p=float("inf")), "sigma_p must be finite and > 0"),
    (dict(flags=1), "denoise flags must be 0"), (dict(reserved=7), "denoise reserved must be 0"),
]


def params(crt, **over):
    p = crt.denoise_params(5, 7, 4.0, 0.05)
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("over,word", BAD_PARAMS, ids=[f"{next(iter(o))}={next(iter(o.values()))}" for o, _ in BAD_PARAMS])
def test_filter_parameter_rules(crt, job, over, word):
    scene, cam = job
    rgb, var, feat, out, var_out = buffers()
    with pytest.raises(crt.CrtError, match=r"\(-1\).*" + word):
        crt.denoise(0, W, H, rgb, var, feat, params(crt, **over), out, var_out)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*" + word):
        scene.render_denoised(cam, params(crt, **over))


def test_filter_buffer_rules(crt):
    rgb, var, feat, out, var_out = buffers()
    n = W * H
    ok = params(crt)
    for args, word in [
            ((rgb, var, feat, ok, 0, var_out), "d_out is null"),
            ((0, var, feat, ok, out, var_out), "null input"), ((rgb, 0, feat, ok, out, 0), "null input"),
            ((rgb, var, 0, ok, out, 0), "null input"), ((rgb, var, feat, None, out, 0), "parameters are null"),
            ((rgb, var, feat, ok, rgb, 0), "d_out aliases d_rgb"),
            ((rgb, var, feat, ok, rgb + n * 24 - 8, 0), "d_out aliases d_rgb"),  # overlaps the last double
            ((rgb, var, feat, ok, var - n * 24 + 8, 0), "d_out aliases d_rgb"),
            ((rgb, var, feat, ok, feat + 88, 0), "d_out aliases d_feat"),
            ((rgb, var, feat, ok, var, 0), "d_out aliases d_var"),
            ((rgb, var, feat, ok, out, var), "d_var_out aliases d_var"),
            ((rgb, var, feat, ok, out, rgb + 16), "d_var_out aliases d_rgb"),
            ((rgb, var, feat, ok, out, feat + 8 * n), "d_var_out aliases d_feat"),
            ((rgb, var, feat, ok, out, out + 24), "d_var_out aliases d_out")]:
        with pytest.raises(crt.CrtError, match=r"\(-1\).*" + word):
            crt.denoise(0, W, H, *args)


def test_feature_and_variance_rules(crt, job):
    from cpp_raytracer_amd import Tiling
    scene, cam = job
    with pytest.raises(crt.CrtError, match=r"\(-1\).*d_feat is null"):
        scene.render_features(0, cam, 0)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*d_var is null"):
        crt.pixel_variance(0, cam, FAKE, 0, 8)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*null argument"):
        crt.pixel_variance(0, cam, 0, FAKE, 8)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*exceeds samples_per_pixel"):
        crt.pixel_variance(0, cam, FAKE, 2 * FAKE, 24)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*not a pass boundary"):
        crt.pixel_variance(0, cam, FAKE, 2 * FAKE, 10)  # 22 spp: chunks of 4
    for t in (Tiling(2, 2, 0, 0), Tiling(6, 3, 1, 1)):
        with pytest.raises(crt.CrtError, match=r"\(-1\).*row_block a multiple of 4"):
            crt.pixel_variance(0, cam, FAKE, 2 * FAKE, 8, blocks_ptr=3 * FAKE, tiling=t)


def test_driver_rules(crt, job):
    from cpp_raytracer_amd import _capi
    scene, cam = job
    out = np.zeros((H, W, 3))
    ok = params(crt)
    call = crt.lib().crt_render_denoised
    assert call(scene.handle, 0, C.byref(cam), None, C.byref(ok), None, None, None) == -1
    assert b"h_rgb is null" in crt.lib().crt_last_error()
    assert call(scene.handle, 0, C.byref(cam), None, None, None, out.ctypes.data, None) == -1
    assert b"parameters are null" in crt.lib().crt_last_error()
    for prm, word in [(_capi.AdaptiveParams(0.1, 8, 8, 2, 0), b"adaptive flags must be 0"),
                      (_capi.AdaptiveParams(0.1, 8, 8, 0, 1), b"adaptive reserved must be 0"),
                      (_capi.AdaptiveParams(-1.0, 8, 8, 0, 0), b"threshold must be finite"),
                      (_capi.AdaptiveParams(float("nan"), 8, 8, 0, 0), b"threshold must be finite")]:
        assert call(scene.handle, 0, C.byref(cam), C.byref(prm), C.byref(ok), None, out.ctypes.data, None) == -1
        assert word in crt.lib().crt_last_error()


def test_denoise_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "denoise_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "denoise_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
