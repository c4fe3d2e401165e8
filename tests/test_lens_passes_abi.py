"""CPU-side checks of the lens pass entries crt_render_lens_pass_async, crt_lens_centre_rays_async,
crt_lens_features_async and crt_render_lens_passes: the header, the exports and the ctypes mirror
agree, and every argument rule is refused with CRT_E_INVALID and a message naming it before any device
work (so they hold on a machine without a GPU). No kernel runs here (tests/test_gpu_lens_passes.py,
test_gpu_lens_features.py and test_gpu_lens_driver.py run them)."""
import ctypes as C
import math
import re

import pytest

from conftest import ROOT
from test_lens_abi import FAKE, RULES, make, rule_ids, scene  # noqa: F401 (scene is a fixture)

HEADER = ROOT / "include" / "crt_render.h"
FNS = ["crt_render_lens_pass_async", "crt_lens_centre_rays_async", "crt_lens_features_async", "crt_render_lens_passes"]
NARGS = dict(zip(FNS, (12, 5, 6, 12)))


def test_header_exports_and_package_agree(crt):
    from cpp_raytracer_amd import _capi
    text = HEADER.read_text()
    for fn in FNS:
        proto = re.search(rf"int {fn}\((.*?)\);", text, re.S).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        assert len(proto.split(",")) == len(_capi.EXPORTS[fn][1]) == NARGS[fn], fn
        assert hasattr(crt.lib(), fn)
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+2\b", text)
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays
    assert "LensRender" in crt.__all__
    from cpp_raytracer_amd.lens_passes import LensRender
    assert crt.LensRender is LensRender
    for m in ("render_lens_pass", "lens_centre_rays", "lens_features", "render_lens_passes"):
        assert callable(getattr(crt.GpuScene, m)), m
    for m in ("step", "finished", "noise", "frame", "features", "denoised", "block_samples", "samples_rendered",
              "state", "resume"):
        assert hasattr(LensRender, m), m
    assert "WAITS FOR `stream` ONCE" in text  # the header says where a masked pass synchronizes


def call(crt, scene, fn, cam, lens, first=0, count=4, d_sum=2 * FAKE, blocks=0, out=3 * FAKE, scene_null=False,
         adaptive=None, denoise=None, h_noisy=0):
    lib = crt.lib()
    pc = C.byref(cam) if cam is not None else None
    pl = C.byref(lens) if lens is not None else None
    h = None if scene_null else scene.handle
    if fn == "crt_render_lens_pass_async":
        rc = lib.crt_render_lens_pass_async(h, 0, pc, pl, first, count, C.c_void_p(d_sum or None), None, None,
                                            C.c_void_p(blocks or None), 0, None)
    elif fn == "crt_lens_centre_rays_async":
        rc = lib.crt_lens_centre_rays_async(0, pc, pl, C.c_void_p(out or None), None)
    elif fn == "crt_lens_features_async":
        rc = lib.crt_lens_features_async(h, 0, pc, pl, C.c_void_p(out or None), None)
    else:
        from cpp_raytracer_amd import _capi
        rc = lib.crt_render_lens_passes(h, 0, pc, pl, C.byref(adaptive) if adaptive is not None else None,
                                        C.byref(denoise) if denoise is not None else None, _capi.DENOISED_FN(), None,
                                        C.c_void_p(h_noisy or None), C.c_void_p(out or None), None, None)
    return rc, lib.crt_last_error().decode()


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("kind,over,cam_over,word", RULES, ids=rule_ids(RULES))
def test_every_lens_rule(crt, scene, fn, kind, over, cam_over, word):
    cam, lens = make(crt, kind, cam_over, over)
    rc, msg = call(crt, scene, fn, cam, lens)
    assert rc == -1 and re.search(fn + ": .*" + word, msg), (rc, msg)


@pytest.mark.parametrize("fn", FNS)
def test_null_pointers(crt, scene, fn):
    cam, lens = make(crt)
    rc, msg = call(crt, scene, fn, None, lens)
    assert rc == -1 and fn + ": cam is null" in msg, (rc, msg)
    rc, msg = call(crt, scene, fn, cam, None)
    assert rc == -1 and fn + ": lens is null" in msg, (rc, msg)
    if fn != "crt_lens_centre_rays_async":
        rc, msg = call(crt, scene, fn, cam, lens, scene_null=True)
        assert rc == -1 and fn + ": scene is null" in msg, (rc, msg)
    if fn == "crt_render_lens_pass_async":
        rc, msg = call(crt, scene, fn, cam, lens, d_sum=0)
        assert rc == -1 and fn + ": d_sum is null" in msg, (rc, msg)
    else:
        rc, msg = call(crt, scene, fn, cam, lens, out=0)
        assert rc == -1 and re.search(fn + ": (d_rays|d_feat|h_rgb) is null", msg), (rc, msg)


def test_samples_per_pixel(crt, scene):
    for fn in (FNS[0], FNS[3]):
        for spp, word in ((0, "samples_per_pixel must not be 0"), (1 << 31, "samples_per_pixel exceeds 2^31-1")):
            cam, lens = make(crt, cam_over=dict(samples_per_pixel=spp))
            rc, msg = call(crt, scene, fn, cam, lens)
            assert rc == -1 and fn + ": " + word in msg, (rc, msg)
    # the centre rays and the features do not read it
    cam, lens = make(crt, cam_over=dict(samples_per_pixel=0))
    for fn in FNS[1:3]:
        assert call(crt, scene, fn, cam, lens)[0] in (-3, -4)


@pytest.mark.parametrize("kind", [0, 2, 4])
def test_pass_boundaries(crt, scene, kind):
    """A job of 24 samples: chunks of 4. And one of 9: the last chunk is one sample."""
    fn = FNS[0]
    cam, lens = make(crt, kind, dict(samples_per_pixel=24))
    bad = [(dict(first=2, count=4), "first_sample 2 is not a multiple of the chunk length"),
           (dict(first=0, count=0), "num_samples is 0"),
           (dict(first=20, count=8), "first_sample \\+ num_samples = 28 exceeds samples_per_pixel = 24"),
           (dict(first=0xFFFFFFFC, count=8), "exceeds samples_per_pixel"),
           (dict(first=4, count=6), "the pass ends at sample 10, neither a multiple of the chunk length nor samples_per_pixel"),
           (dict(first=0, count=4, d_sum=0), "d_sum is null")]
    for kw, word in bad:
        for blocks in (0, 4 * FAKE):
            rc, msg = call(crt, scene, fn, cam, lens, blocks=blocks, **kw)
            assert rc == -1 and re.search(fn + ": .*" + word, msg), (kw, rc, msg)
    cam9, _ = make(crt, kind, dict(samples_per_pixel=9))
    rc, msg = call(crt, scene, fn, cam9, lens, first=8, count=2)
    assert rc == -1 and "exceeds samples_per_pixel = 9" in msg
    for cam_ok, kw in ((cam, dict(first=0, count=24)), (cam, dict(first=8, count=12)), (cam, dict(first=20, count=4)),
                       (cam9, dict(first=8, count=1)), (cam9, dict(first=0, count=9)), (cam9, dict(first=4, count=4))):
        rc, msg = call(crt, scene, fn, cam_ok, lens, **kw)
        assert rc in (-3, -4), (kw, rc, msg)  # past the rules: no device, or the scene is not uploaded


def test_frame_size(crt, scene):
    cam, lens = make(crt, 2, dict(image_w=1 << 16, image_h=1 << 15))  # 2^31 pixels
    for fn in FNS:
        rc, msg = call(crt, scene, fn, cam, lens)
        assert rc == -1 and fn + ": frame has more than 2^31-1 pixels" in msg, (rc, msg)


def test_driver_rules(crt, scene):
    from cpp_raytracer_amd import _capi
    fn = FNS[3]
    cam, lens = make(crt, 3, dict(samples_per_pixel=24))
    ok_ad = lambda **kw: _capi.AdaptiveParams(**{**dict(threshold=0.05, min_samples=0, samples_per_pass=8, flags=0, reserved=0), **kw})
    ok_dn = lambda **kw: _capi.DenoiseParams(**{**dict(iterations=3, normal_squarings=7, sigma_l=1.0, sigma_p=0.05, flags=0, reserved=0), **kw})
    rc, msg = call(crt, scene, fn, cam, lens, h_noisy=5 * FAKE)
    assert rc == -1 and fn + ": h_noisy must be null without denoise" in msg, (rc, msg)
    for ad, word in ((ok_ad(reserved=1), "adaptive reserved must be 0"), (ok_ad(flags=1), "unknown adaptive flags"),
                     (ok_ad(flags=4), "unknown adaptive flags"), (ok_ad(threshold=-1.0), "threshold must be finite and >= 0"),
                     (ok_ad(threshold=math.nan), "threshold must be finite and >= 0"),
                     (ok_ad(threshold=math.inf), "threshold must be finite and >= 0")):
        rc, msg = call(crt, scene, fn, cam, lens, adaptive=ad)
        assert rc == -1 and fn + ": " + word in msg, (rc, msg)
    for dn, word in ((ok_dn(iterations=0), "iterations = 0 is outside 1..8"), (ok_dn(iterations=9), "iterations = 9 is outside 1..8"),
                     (ok_dn(normal_squarings=11), "normal_squarings = 11 is outside 0..10"),
                     (ok_dn(sigma_l=0.0), "sigma_l must be finite and > 0"), (ok_dn(sigma_p=math.inf), "sigma_p must be finite and > 0"),
                     (ok_dn(flags=1), "denoise flags must be 0"), (ok_dn(reserved=2), "denoise reserved must be 0")):
        rc, msg = call(crt, scene, fn, cam, lens, denoise=dn, h_noisy=5 * FAKE)
        assert rc == -1 and fn + ": " + word in msg, (rc, msg)
    # nothing was written through the fake pointers, and *samples_rendered is zeroed by a refused call
    done = C.c_uint64(77)
    rc = crt.lib().crt_render_lens_passes(scene.handle, 0, C.byref(cam), C.byref(lens), C.byref(ok_ad(reserved=1)), None,
                                          _capi.DENOISED_FN(), None, None, C.c_void_p(FAKE), None, C.byref(done))
    assert rc == -1 and done.value == 0


def test_python_wrappers_refuse_before_the_library(crt, scene):
    cam, lens = make(crt, 3, dict(samples_per_pixel=24))
    with pytest.raises(crt.CrtError, match="preview needs an adaptive render"):
        scene.render_lens_passes(cam, lens, preview=True)
    with pytest.raises(crt.CrtError, match="noisy=True needs denoise"):
        scene.render_lens_passes(cam, lens, noisy=True)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*first_sample 2 is not a multiple"):
        scene.render_lens_pass(0, cam, lens, 2, 4, FAKE)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*unknown kind"):
        scene.lens_features(0, *make(crt, over=dict(kind=9)), FAKE)
