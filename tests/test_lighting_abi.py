"""CPU-side checks of the lit entries (crt_lighting; crt_radiance_lit_async, crt_probes_lit_async,
crt_render_lens_lit_async, crt_render_lens_pass_lit_async, crt_render_lens_lit and
crt_render_lens_passes_lit): the header, the exports and the ctypes mirror agree; every rule of the
lighting is refused with CRT_E_INVALID and a message naming it before any device work, after the call's
own rules; the Python front end's ValueErrors hold, the one env= with lights= raised before included. No
kernel runs here (tests/test_gpu_lighting.py runs them); "a sampler of another scene or device" needs a
sampler, which needs a resident scene, so those rules are checked there."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = ROOT / "include" / "crt_render.h"
FAKE = 1 << 20  # device pointers that are never dereferenced
ENTRIES = {"crt_radiance_lit_async": 9, "crt_probes_lit_async": 9, "crt_render_lens_lit_async": 7,
           "crt_render_lens_pass_lit_async": 13, "crt_render_lens_lit": 8, "crt_render_lens_passes_lit": 15}
ASYNC = ["crt_radiance_lit_async", "crt_probes_lit_async", "crt_render_lens_lit_async", "crt_render_lens_pass_lit_async"]
BLOCKING = ["crt_render_lens_lit", "crt_render_lens_passes_lit"]
FIELDS = ["env", "sampler", "lights", "reserved"]


def test_header_exports_and_struct_agree(crt):
    from cpp_raytracer_amd import _capi
    text = HEADER.read_text()
    for fn, nargs in ENTRIES.items():
        proto = re.search(rf"int {fn}\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.EXPORTS[fn][1]) == nargs, fn
        assert hasattr(crt.lib(), fn)
    body = re.search(r"typedef struct crt_lighting \{(.*?)\} crt_lighting;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\*?\s*(\w+)\s*$", decl.strip())[0] for decl in body.split(";") if decl.strip()]
    assert names == [f for f, _ in _capi.LightingView._fields_] == FIELDS
    assert C.sizeof(_capi.LightingView) == 32
    assert [getattr(_capi.LightingView, f).offset for f in names] == [0, 8, 16, 24]
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays
    for name in ["Lighting", "LightingView"]:
        assert name in crt.__all__, name
    # the header no longer says the combination is not offered, and says why each sample meets pb alone
    assert "are not offered" not in text and "disjoint emitters" in text


@pytest.fixture(scope="module")
def scene(crt):
    return crt.GpuScene(crt.SceneData.named("cornell"))


def lens_and_cam(over=None):
    from cpp_raytracer_amd import _capi
    D3 = _capi.D3
    lens = _capi.Lens(4, 0, D3(1.0, 2.0, 3.0), D3(1.0, 0.0, 0.0), D3(0.0, 1.0, 0.0), D3(0.0, 0.0, -1.0), 0.0, 0.0, 0)
    cam = _capi.Camera()
    cam.image_w, cam.image_h, cam.samples_per_pixel, cam.max_depth = 4, 24, 4, 50
    cam.background = D3(0.1, 0.2, 0.3)
    cam.t_min = 1e-5
    for k, v in (over or {}).items():
        setattr(cam, k, v)
    return lens, cam


def env_view(texels=FAKE, face_size=4, filt=1, right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, -1.0)):
    from cpp_raytracer_amd import _capi
    D3 = _capi.D3
    return _capi.EnvView(texels, face_size, filt, D3(*right), D3(*up), D3(*forward))


def lit_call(crt, scene, fn, lighting, over=None):
    """One call of an async lit entry with pointers that are never read: (rc, message)."""
    from cpp_raytracer_amd import _capi
    lib, D3, vp = crt.lib(), _capi.D3, C.c_void_p
    ref = C.byref(lighting) if lighting is not None else None
    if fn == "crt_radiance_lit_async":
        p = _capi.RadianceParams(50, 0, D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in (over or {}).items():
            setattr(p, k, v)
        rc = lib.crt_radiance_lit_async(scene.handle, 0, vp(FAKE), 8, None, C.byref(p), ref, vp(2 * FAKE), None)
    elif fn == "crt_probes_lit_async":
        p = _capi.ProbeParams(16, 50, 0, 0, D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in (over or {}).items():
            setattr(p, k, v)
        rc = lib.crt_probes_lit_async(scene.handle, 0, vp(FAKE), None, 8, C.byref(p), ref, vp(2 * FAKE), None)
    elif fn == "crt_render_lens_lit_async":
        lens, cam = lens_and_cam(over)
        rc = lib.crt_render_lens_lit_async(scene.handle, 0, C.byref(cam), C.byref(lens), ref, vp(2 * FAKE), None)
    else:
        lens, cam = lens_and_cam(over)
        rc = lib.crt_render_lens_pass_lit_async(scene.handle, 0, C.byref(cam), C.byref(lens), ref, 0, 4, vp(2 * FAKE),
                                                None, None, None, 0, None)
    return rc, lib.crt_last_error().decode()


def lighting(env=None, sampler=None, lights=None, reserved=0):
    from cpp_raytracer_amd import _capi
    v = _capi.LightingView()
    if env is not None:
        v.env = C.pointer(env)
    v.sampler, v.lights, v.reserved = sampler, lights, reserved
    return v


@pytest.mark.parametrize("fn", ASYNC)
def test_the_lightings_rules_come_after_the_calls_own_and_before_any_device_work(crt, scene, fn):
    rc, msg = lit_call(crt, scene, fn, None)
    assert rc == -1 and re.search(fn + ": lighting is null", msg), (rc, msg)
    rc, msg = lit_call(crt, scene, fn, None, dict(t_min=-1.0))  # the call's own rules first
    assert rc == -1 and re.search(fn + ": t_min must be finite", msg), (rc, msg)
    if fn != "crt_render_lens_pass_lit_async":  # depth 0 is answered after the rules
        rc, msg = lit_call(crt, scene, fn, None, dict(max_depth=0))
        assert rc == -1 and re.search(fn + ": lighting is null", msg), (rc, msg)
    rc, msg = lit_call(crt, scene, fn, lighting(env=env_view(), sampler=FAKE))
    assert rc == -1 and re.search(fn + ": lighting->env and lighting->sampler are both set", msg), (rc, msg)
    rc, msg = lit_call(crt, scene, fn, lighting(reserved=1))
    assert rc == -1 and re.search(fn + ": lighting->reserved must be 0", msg), (rc, msg)
    rc, msg = lit_call(crt, scene, fn, lighting(env=env_view(), lights=FAKE, reserved=1 << 40))
    assert rc == -1 and re.search(fn + ": lighting->reserved must be 0", msg), (rc, msg)
    # crt_env's rules for the env member, lights or not (the light sampler is looked at after them)
    for bad, rule in ((env_view(texels=None), "env->texels is null"), (env_view(face_size=0), r"env->face_size must be in 1 \.\. 16384"),
                      (env_view(face_size=16385), r"env->face_size must be in 1 \.\. 16384"), (env_view(filt=2), "unknown env->filter"),
                      (env_view(up=(0.0, math.nan, 0.0)), "the env basis .* must be finite"),
                      (env_view(forward=(math.inf, 0.0, 0.0)), "the env basis .* must be finite")):
        for lights in (None, FAKE):
            rc, msg = lit_call(crt, scene, fn, lighting(env=bad, lights=lights))
            assert rc == -1 and re.search(fn + ": " + rule, msg), (rc, msg, rule)


def test_the_pass_entry_keeps_the_pass_rules(crt, scene):
    from cpp_raytracer_amd import _capi
    lib, vp = crt.lib(), C.c_void_p
    lens, cam = lens_and_cam()
    lit = lighting()
    for first, count, sum_ptr, rule in ((0, 0, 2 * FAKE, "crt_render_lens_pass_lit_async"), (0, 4, None, "crt_render_lens_pass_lit_async"),
                                        (3, 4, 2 * FAKE, "crt_render_lens_pass_lit_async")):
        rc = lib.crt_render_lens_pass_lit_async(scene.handle, 0, C.byref(cam), C.byref(lens), C.byref(lit), first, count,
                                                vp(sum_ptr), None, None, None, 0, None)
        unlit = lib.crt_last_error().decode()
        assert rc == -1 and rule in unlit, (rc, unlit)
        # the same rule, worded as the unlit entry words it
        rc2 = lib.crt_render_lens_pass_async(scene.handle, 0, C.byref(cam), C.byref(lens), first, count, vp(sum_ptr), None, None,
                                             None, 0, None)
        assert rc2 == -1 and lib.crt_last_error().decode().replace("crt_render_lens_pass_async", "crt_render_lens_pass_lit_async") == unlit
    assert _capi.EXPORTS["crt_render_lens_pass_lit_async"][1][5:] == _capi.EXPORTS["crt_render_lens_pass_async"][1][4:]


def blocking(crt, scene, fn, env, importance, lights, over=None, out=2 * FAKE):
    lib = crt.lib()
    lens, cam = lens_and_cam(over)
    ref = C.byref(env) if env is not None else None
    if fn == "crt_render_lens_lit":
        rc = lib.crt_render_lens_lit(scene.handle, 0, C.byref(cam), C.byref(lens), ref, importance, lights, C.c_void_p(out))
    else:
        from cpp_raytracer_amd import _capi
        rc = lib.crt_render_lens_passes_lit(scene.handle, 0, C.byref(cam), C.byref(lens), ref, importance, lights, None, None,
                                            _capi.DENOISED_FN(), None, None, C.c_void_p(out), None, None)
    return rc, lib.crt_last_error().decode()


@pytest.mark.parametrize("fn", BLOCKING)
def test_the_blocking_entries_rules(crt, scene, fn):
    host = np.ones((24, 4, 3))
    ok = env_view(texels=host.ctypes.data)
    rc, msg = blocking(crt, scene, fn, None, 1, 0)
    assert rc == -1 and re.search(fn + ": importance needs env", msg), (rc, msg)
    rc, msg = blocking(crt, scene, fn, None, 1, 1, dict(t_min=-1.0))
    assert rc == -1 and re.search(fn + ": t_min must be finite", msg), (rc, msg)
    for imp, lights, rule in ((2, 0, "importance must be 0 or 1"), (-1, 1, "importance must be 0 or 1"), (0, 2, "lights must be 0 or 1")):
        rc, msg = blocking(crt, scene, fn, ok, imp, lights)
        assert rc == -1 and re.search(fn + ": " + rule, msg), (rc, msg)
    for imp in (0, 1):  # crt_env's rules either way
        rc, msg = blocking(crt, scene, fn, env_view(texels=None), imp, 1)
        assert rc == -1 and re.search(fn + ": env->texels is null", msg), (rc, msg)
    # crt_env_sampler_create's rules with importance only
    skew = env_view(texels=host.ctypes.data, up=(0.0, 1.0, 1e-3))
    big = env_view(texels=host.ctypes.data, face_size=2049)
    for bad, rule in ((skew, "the env basis must be orthonormal"), (big, "env->face_size must be at most 2048 for a sampler")):
        rc, msg = blocking(crt, scene, fn, bad, 1, 0)
        assert rc == -1 and re.search(fn + ": " + rule, msg), (rc, msg)
    rc, msg = blocking(crt, scene, fn, ok, 0, 1, out=None)
    assert rc == -1 and re.search(fn + r": h?_?rgb is null", msg), (rc, msg)
    if crt.device_count() == 0:  # no rule broken: the call reaches the device layer
        for env, imp, lights in ((None, 0, 0), (ok, 1, 1), (skew, 0, 1)):
            rc, msg = blocking(crt, scene, fn, env, imp, lights)
            assert rc == -3 and "no HIP device" in msg, (rc, msg)


def test_python_argument_errors(crt, scene):
    import torch

    class FakeRays:  # enough of a tensor to reach the lighting= rules, which come before any GPU call
        is_cuda, dtype, shape = True, torch.float64, (4, 6)
        device = torch.device("cuda", 0)

        def dim(self):
            return 2

        def contiguous(self):
            return self

    class FakePoints(FakeRays):
        shape = (4, 3)

    other = crt.GpuScene(crt.SceneData.named("cornell"))
    smp = crt.LightSampler(other, 0, None)  # no handle: nothing to free
    mine = crt.LightSampler(scene, 0, None)
    env = crt.Env(None, None)
    lens, cam = lens_and_cam()
    with pytest.raises(crt.CrtError, match="Lighting: env must be an Env"):
        crt.Lighting(env=object())
    with pytest.raises(crt.CrtError, match="Lighting: lights must be a LightSampler"):
        crt.Lighting(lights=object())
    lit = crt.Lighting(lights=mine)
    assert lit.env is None and lit.lights is mine and crt.Lighting().env is None and crt.Lighting().lights is None
    calls = {
        "radiance": lambda **kw: scene.radiance(FakeRays(), **kw),
        "probes": lambda **kw: scene.probes(FakePoints(), **kw),
        "render_lens": lambda **kw: scene.render_lens(cam, lens, **kw),
    }
    for who, call in calls.items():
        for kw in (dict(env=env), dict(lights=mine), dict(env=env, lights=mine)):
            with pytest.raises(ValueError, match=who + ": lighting= cannot be combined with env= or lights="):
                call(lighting=lit, **kw)
        with pytest.raises(crt.CrtError, match=who + ": lighting must be a Lighting"):
            call(lighting=object())
        with pytest.raises(crt.CrtError, match=who + ": the LightSampler belongs to another scene or device"):
            call(lighting=crt.Lighting(lights=smp))
        with pytest.raises(crt.CrtError, match=who + ": env's texels must be"):
            call(lighting=crt.Lighting(env=env))
        # what env= with lights= raised before, it raises still
        with pytest.raises(ValueError, match=who + ": lights= and env= cannot be combined"):
            call(lights=mine, env=env)
    from cpp_raytracer_amd import _capi
    view = _capi.LightingView()
    for call in (lambda **kw: scene.radiance_async(0, FAKE, 4, 2 * FAKE, max_depth=5, background=(0, 0, 0), **kw),
                 lambda **kw: scene.probes_async(0, FAKE, 0, 4, 2 * FAKE, samples=4, max_depth=5, background=(0, 0, 0), **kw),
                 lambda **kw: scene.render_lens_async(0, cam, lens, 2 * FAKE, **kw)):
        for kw in (dict(env=env_view()), dict(sampler=FAKE), dict(lights=FAKE)):
            with pytest.raises(ValueError, match="lighting= cannot be combined with env=, sampler= or lights="):
                call(lighting=view, **kw)
    with pytest.raises(crt.CrtError, match="render_lens_pass: the LightSampler belongs to another scene or device"):
        scene.render_lens_pass(0, cam, lens, 0, 4, 2 * FAKE, lighting=crt.Lighting(lights=smp))
    with pytest.raises(crt.CrtError, match="render_lens_passes: lighting must be a Lighting"):
        scene.render_lens_passes(cam, lens, lighting=object())
    with pytest.raises(crt.CrtError, match="render_lens_passes: the LightSampler belongs to another scene or device"):
        scene.render_lens_passes(cam, lens, lighting=crt.Lighting(lights=smp))
    from cpp_raytracer_amd.lens_passes import LensRender
    import inspect
    assert "lighting" in inspect.signature(LensRender.__init__).parameters
    assert "lighting" in inspect.signature(LensRender.resume).parameters
