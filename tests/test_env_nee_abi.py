"""CPU-side checks of the luminance-sampling entries (crt_env_sampler_create / _free / _view,
crt_radiance_env_sampled_async, crt_probes_env_sampled_async, crt_render_lens_env_sampled_async and
crt_render_lens_env_sampled): the header, the exports and the ctypes mirror agree; every new rule and
null pointer is refused with CRT_E_INVALID and a message naming it before any device work (a call that
got as far as looking for a device fails with CRT_E_NODEVICE, or CRT_E_NOT_UPLOADED on a machine with
a GPU); the Python front end refuses wrong arguments before any GPU call. No kernel runs here
(tests/test_gpu_env_nee.py runs them); a sampler "built on another device" needs a sampler, so that
rule is checked there."""
import ctypes as C
import math
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = ROOT / "include" / "crt_render.h"
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
FAKE = 1 << 20  # device pointers that are never dereferenced
NAN, INF = math.nan, math.inf
ENTRIES = {"crt_env_sampler_create": 3, "crt_env_sampler_free": 1, "crt_env_sampler_view": 2,
           "crt_radiance_env_sampled_async": 9, "crt_probes_env_sampled_async": 9,
           "crt_render_lens_env_sampled_async": 7, "crt_render_lens_env_sampled": 6}
SAMPLED = ["crt_radiance_env_sampled_async", "crt_probes_env_sampled_async", "crt_render_lens_env_sampled_async"]


def test_header_exports_and_struct_agree(crt):
    from cpp_raytracer_amd import _capi
    text = HEADER.read_text()
    for fn, nargs in ENTRIES.items():
        proto = re.search(rf"int {fn}\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.EXPORTS[fn][1]) == nargs, fn
        assert hasattr(crt.lib(), fn)
    body = re.search(r"struct crt_env_sampler_view \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"\*?(\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f for f, _ in _capi.EnvSamplerView._fields_] == ["env", "w", "c", "m", "W"]
    assert C.sizeof(_capi.EnvSamplerView) == 120
    assert [getattr(_capi.EnvSamplerView, f).offset for f in names] == [0, 88, 96, 104, 112]
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays
    for name in ["Env", "EnvTables", "EnvSamplerView", "make_env"]:
        assert name in crt.__all__, name


@pytest.fixture(scope="module")
def scene(crt):
    return crt.GpuScene(crt.SceneData.named("cornell"))


def env_view(**over):
    from cpp_raytracer_amd import _capi
    D3 = _capi.D3
    e = _capi.EnvView(FAKE, 4, 1, D3(1.0, 0.0, 0.0), D3(0.0, 1.0, 0.0), D3(0.0, 0.0, -1.0))
    for k, v in over.items():
        setattr(e, k, D3(*v) if k in ("right", "up", "forward") else v)
    return e


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


def create(crt, env, out=True):
    h = C.c_void_p(0xDEAD)
    rc = crt.lib().crt_env_sampler_create(0, C.byref(env) if env is not None else None, C.byref(h) if out else None)
    return rc, crt.lib().crt_last_error().decode(), h.value


def lens_host(crt, scene, env, over=None):
    lens, cam = lens_and_cam(over)
    rc = crt.lib().crt_render_lens_env_sampled(scene.handle, 0, C.byref(cam), C.byref(lens),
                                               C.byref(env) if env is not None else None, C.c_void_p(2 * FAKE))
    return rc, crt.lib().crt_last_error().decode()


S2 = math.sqrt(0.5)
RULES = [
    (None, "env is null"),
    (dict(texels=None), "env->texels is null"),
    (dict(face_size=0), "face_size must be in 1 .. 16384"), (dict(face_size=16385), "face_size must be in 1 .. 16384"),
    (dict(face_size=2049), "face_size must be at most 2048 for a sampler"),
    (dict(face_size=16384), "face_size must be at most 2048 for a sampler"),
    (dict(filter=2), "unknown env->filter"),
    (dict(right=(NAN, 0.0, 0.0)), "env basis .* must be finite"), (dict(forward=(0.0, 0.0, -INF)), "env basis .* must be finite"),
    # the Gram matrix: a long vector, a zero one, a skewed pair, one entry 2e-9 off, a huge one (inf - inf)
    (dict(right=(2.0, 0.0, 0.0)), "env basis must be orthonormal"),
    (dict(up=(0.0, 0.0, 0.0)), "env basis must be orthonormal"),
    (dict(right=(S2, S2, 0.0)), "env basis must be orthonormal"),
    (dict(forward=(0.0, 0.0, -(1.0 + 1e-9))), "env basis must be orthonormal"),
    (dict(forward=(1e300, -1e300, 0.0)), "env basis must be orthonormal"),
    # an earlier rule wins: crt_env's own, then the face size, then the Gram matrix
    (dict(face_size=4096, filter=9), "unknown env->filter"), (dict(filter=9, right=(2.0, 0.0, 0.0)), "unknown env->filter"),
    (dict(face_size=4096, right=(2.0, 0.0, 0.0)), "face_size must be at most 2048"),
]


@pytest.mark.parametrize("over,word", RULES, ids=[re.sub(r"\W+", "_", w)[:24] + str(i) for i, (_, w) in enumerate(RULES)])
def test_sampler_rules(crt, scene, over, word):
    env = None if over is None else env_view(**over)
    rc, msg, h = create(crt, env)
    assert rc == -1 and re.search("crt_env_sampler_create: .*" + word, msg), (rc, msg)
    assert h is None  # *out is cleared
    rc, msg = lens_host(crt, scene, env)
    assert rc == -1 and re.search("crt_render_lens_env_sampled: .*" + word, msg), (rc, msg)


def test_null_pointers(crt, scene):
    lib = crt.lib()
    rc, msg, _ = create(crt, env_view(), out=False)
    assert rc == -1 and "crt_env_sampler_create: out is null" in msg
    assert lib.crt_env_sampler_free(None) == 0
    from cpp_raytracer_amd import _capi
    v = _capi.EnvSamplerView()
    assert lib.crt_env_sampler_view(None, C.byref(v)) == -1
    assert "crt_env_sampler_view: sampler is null" in lib.crt_last_error().decode()
    assert lib.crt_env_sampler_view(C.c_void_p(FAKE), None) == -1  # the sampler is not read before the check
    assert "crt_env_sampler_view: out is null" in lib.crt_last_error().decode()


def sampled(crt, scene, fn, sampler, over=None):
    from cpp_raytracer_amd import _capi
    lib, D3, vp = crt.lib(), _capi.D3, C.c_void_p
    if fn == "crt_radiance_env_sampled_async":
        p = _capi.RadianceParams(50, 0, D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in (over or {}).items():
            setattr(p, k, v)
        rc = lib.crt_radiance_env_sampled_async(scene.handle, 0, vp(FAKE), 8, None, C.byref(p), sampler, vp(2 * FAKE), None)
    elif fn == "crt_probes_env_sampled_async":
        p = _capi.ProbeParams(16, 50, 0, 0, D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in (over or {}).items():
            setattr(p, k, v)
        rc = lib.crt_probes_env_sampled_async(scene.handle, 0, vp(FAKE), None, 8, C.byref(p), sampler, vp(2 * FAKE), None)
    else:
        lens, cam = lens_and_cam(over)
        rc = lib.crt_render_lens_env_sampled_async(scene.handle, 0, C.byref(cam), C.byref(lens), sampler, vp(2 * FAKE), None)
    return rc, lib.crt_last_error().decode()


@pytest.mark.parametrize("fn", SAMPLED)
def test_a_null_sampler_is_refused_after_the_calls_own_rules(crt, scene, fn):
    rc, msg = sampled(crt, scene, fn, None)
    assert rc == -1 and re.search(fn + ": sampler is null", msg), (rc, msg)
    rc, msg = sampled(crt, scene, fn, None, dict(t_min=-1.0))
    assert rc == -1 and re.search(fn + ": t_min must be finite", msg), (rc, msg)
    rc, msg = sampled(crt, scene, fn, None, dict(max_depth=0))  # depth 0 is answered after the rules
    assert rc == -1 and re.search(fn + ": sampler is null", msg), (rc, msg)


def test_the_host_entrys_own_rules_come_first(crt, scene):
    rc, msg = lens_host(crt, scene, env_view(face_size=0), dict(t_min=-1.0))
    assert rc == -1 and "crt_render_lens_env_sampled: t_min must be finite" in msg
    lens, cam = lens_and_cam()
    rc = crt.lib().crt_render_lens_env_sampled(scene.handle, 0, C.byref(cam), C.byref(lens), C.byref(env_view()), None)
    assert rc == -1 and "crt_render_lens_env_sampled: rgb is null" in crt.lib().crt_last_error().decode()


def test_valid_envs_get_past_the_rules(crt, scene):
    """No rule broken: the call reaches the device layer. The build and the blocking entry would read the
    fake texels on a device, so they are called only where none is visible."""
    if crt.device_count() != 0:
        return  # a sampler of fake texels would be built on the device; tests/test_gpu_env_nee.py builds real ones
    tilt = math.sqrt(1.0 - 0.36)
    for over in (dict(), dict(face_size=1), dict(face_size=2048), dict(filter=0),
                 dict(right=(0.6, tilt, 0.0), up=(-tilt, 0.6, 0.0)), dict(forward=(0.0, 0.0, -(1.0 + 4e-10)))):
        rc, msg, h = create(crt, env_view(**over))
        assert rc == -3 and "no HIP device" in msg and h is None, (over, rc, msg)
        rc, msg = lens_host(crt, scene, env_view(**over))
        assert rc == -3 and "no HIP device" in msg, (over, rc, msg)


def test_python_argument_errors(crt):
    import torch
    ok = torch.zeros((12, 2, 3), dtype=torch.float64)
    with pytest.raises(crt.CrtError, match="make_env: texels must be a contiguous \\(6n, n, 3\\) float64 tensor on a GPU"):
        crt.make_env(ok, importance=True)  # a CPU tensor
    from cpp_raytracer_amd import _capi
    env = crt.Env(ok, _capi.EnvView())
    assert env.sampler is None
    with pytest.raises(crt.CrtError, match="Env.tables: the Env has no sampler"):
        env.tables


def test_env_nee_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "env_nee_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "env_nee_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
