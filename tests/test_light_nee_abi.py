"""CPU-side checks of the light-sampling entries (crt_light_sampler_create / _free / _view,
crt_radiance_lights_async, crt_probes_lights_async, crt_render_lens_lights_async and
crt_render_lens_lights): the header, the exports and the ctypes mirror agree; every new rule and null
pointer is refused with CRT_E_INVALID and a message naming it before any device work; the Python front end
refuses wrong arguments before any GPU call. No kernel runs here (tests/test_gpu_light_nee.py runs them);
"a sampler of another scene or device", "no light" and "no usable total" need a resident scene, so those
rules are checked there."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = ROOT / "include" / "crt_render.h"
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
FAKE = 1 << 20  # device pointers that are never dereferenced
ENTRIES = {"crt_light_sampler_create": 3, "crt_light_sampler_free": 1, "crt_light_sampler_view": 2,
           "crt_radiance_lights_async": 9, "crt_probes_lights_async": 9, "crt_render_lens_lights_async": 7,
           "crt_render_lens_lights": 5}
SAMPLED = ["crt_radiance_lights_async", "crt_probes_lights_async", "crt_render_lens_lights_async"]
FIELDS = ["num_lights", "device", "prim", "ref", "sorted_ref", "w", "cdf", "sorted_w", "W"]


def test_header_exports_and_struct_agree(crt):
    from cpp_raytracer_amd import _capi
    text = HEADER.read_text()
    for fn, nargs in ENTRIES.items():
        proto = re.search(rf"int {fn}\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.EXPORTS[fn][1]) == nargs, fn
        assert hasattr(crt.lib(), fn)
    body = re.search(r"struct crt_light_sampler_view \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"\*?(\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f for f, _ in _capi.LightSamplerView._fields_] == FIELDS
    assert C.sizeof(_capi.LightSamplerView) == 64
    assert [getattr(_capi.LightSamplerView, f).offset for f in names] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays
    for name in ["LightSampler", "LightTables", "LightSamplerView"]:
        assert name in crt.__all__, name


@pytest.fixture(scope="module")
def scene(crt):
    return crt.GpuScene(crt.SceneData.named("cornell"))


def create(crt, scene_handle, device=0, out=True):
    h = C.c_void_p(0xDEAD)
    rc = crt.lib().crt_light_sampler_create(scene_handle, device, C.byref(h) if out else None)
    return rc, crt.lib().crt_last_error().decode(), h.value


def test_create_rules_and_null_pointers(crt, scene):
    lib = crt.lib()
    rc, msg, _ = create(crt, scene.handle, out=False)
    assert rc == -1 and "crt_light_sampler_create: out is null" in msg
    rc, msg, h = create(crt, None)
    assert rc == -1 and "crt_light_sampler_create: scene is null" in msg and h is None  # *out is cleared
    # a scene that was never uploaded is resident nowhere; no device is looked for
    for device in (0, 3, -1, 16, 1 << 20):
        rc, msg, h = create(crt, scene.handle, device)
        assert rc == -1 and f"crt_light_sampler_create: the scene is not resident on device {device}" in msg and h is None
    assert lib.crt_light_sampler_free(None) == 0
    from cpp_raytracer_amd import _capi
    v = _capi.LightSamplerView()
    assert lib.crt_light_sampler_view(None, C.byref(v)) == -1
    assert "crt_light_sampler_view: lights is null" in lib.crt_last_error().decode()
    assert lib.crt_light_sampler_view(C.c_void_p(FAKE), None) == -1  # the sampler is not read before the check
    assert "crt_light_sampler_view: out is null" in lib.crt_last_error().decode()


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


def sampled(crt, scene, fn, lights, over=None):
    from cpp_raytracer_amd import _capi
    lib, D3, vp = crt.lib(), _capi.D3, C.c_void_p
    if fn == "crt_radiance_lights_async":
        p = _capi.RadianceParams(50, 0, D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in (over or {}).items():
            setattr(p, k, v)
        rc = lib.crt_radiance_lights_async(scene.handle, 0, vp(FAKE), 8, None, C.byref(p), lights, vp(2 * FAKE), None)
    elif fn == "crt_probes_lights_async":
        p = _capi.ProbeParams(16, 50, 0, 0, D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in (over or {}).items():
            setattr(p, k, v)
        rc = lib.crt_probes_lights_async(scene.handle, 0, vp(FAKE), None, 8, C.byref(p), lights, vp(2 * FAKE), None)
    else:
        lens, cam = lens_and_cam(over)
        rc = lib.crt_render_lens_lights_async(scene.handle, 0, C.byref(cam), C.byref(lens), lights, vp(2 * FAKE), None)
    return rc, lib.crt_last_error().decode()


@pytest.mark.parametrize("fn", SAMPLED)
def test_a_null_sampler_is_refused_after_the_calls_own_rules(crt, scene, fn):
    rc, msg = sampled(crt, scene, fn, None)
    assert rc == -1 and re.search(fn + ": lights is null", msg), (rc, msg)
    rc, msg = sampled(crt, scene, fn, None, dict(t_min=-1.0))
    assert rc == -1 and re.search(fn + ": t_min must be finite", msg), (rc, msg)
    rc, msg = sampled(crt, scene, fn, None, dict(max_depth=0))  # depth 0 is answered after the rules
    assert rc == -1 and re.search(fn + ": lights is null", msg), (rc, msg)


def test_the_blocking_entrys_rules(crt, scene):
    lib = crt.lib()
    lens, cam = lens_and_cam(dict(t_min=-1.0))
    rc = lib.crt_render_lens_lights(scene.handle, 0, C.byref(cam), C.byref(lens), C.c_void_p(2 * FAKE))
    assert rc == -1 and "crt_render_lens_lights: t_min must be finite" in lib.crt_last_error().decode()
    lens, cam = lens_and_cam()
    rc = lib.crt_render_lens_lights(scene.handle, 0, C.byref(cam), C.byref(lens), None)
    assert rc == -1 and "crt_render_lens_lights: rgb is null" in lib.crt_last_error().decode()
    rc = lib.crt_render_lens_lights(None, 0, C.byref(cam), C.byref(lens), C.c_void_p(2 * FAKE))
    assert rc == -1 and "crt_render_lens_lights: " in lib.crt_last_error().decode()
    if crt.device_count() == 0:  # no rule broken: the call reaches the device layer
        rc = lib.crt_render_lens_lights(scene.handle, 0, C.byref(cam), C.byref(lens), C.c_void_p(2 * FAKE))
        assert rc == -3 and "no HIP device" in lib.crt_last_error().decode()


def test_python_argument_errors(crt, scene):
    import torch

    class FakeRays:  # enough of a tensor to reach the lights= rules, which come before any GPU call
        is_cuda, dtype, shape = True, torch.float64, (4, 6)
        device = torch.device("cuda", 0)

        def dim(self):
            return 2

        def contiguous(self):
            return self

    other = crt.GpuScene(crt.SceneData.named("cornell"))
    smp = crt.LightSampler(other, 0, None)  # no handle: nothing to free
    with pytest.raises(crt.CrtError, match="radiance: the LightSampler belongs to another scene or device"):
        scene.radiance(FakeRays(), lights=smp)
    with pytest.raises(crt.CrtError, match="radiance: lights must be a LightSampler"):
        scene.radiance(FakeRays(), lights=object())
    env = crt.Env(None, None)
    for call in (lambda: scene.radiance(FakeRays(), lights=smp, env=env),
                 lambda: scene.render_lens(lens_and_cam()[1], lens_and_cam()[0], lights=smp, env=env)):
        with pytest.raises(ValueError, match="lights= and env= cannot be combined"):
            call()


def test_light_nee_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "light_nee_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "light_nee_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
