"""CPU-side checks of the environment entries crt_radiance_env_async, crt_probes_env_async,
crt_render_lens_env_async and crt_render_lens_env: the header, the exports and the ctypes mirror
agree; every rule of crt_env is refused with CRT_E_INVALID and a message naming it before any device
work (a call that got as far as looking for a device fails with CRT_E_NODEVICE, or
CRT_E_NOT_UPLOADED on a machine with a GPU); the Python front end refuses wrong arguments before any
GPU call; and csrc/crt_env.h's lookup, compiled for the host, is tests/env_model.py's bit for bit.
No kernel runs here (tests/test_gpu_env.py runs them)."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

import env_model as em
from conftest import ROOT
from test_env_model import ROTATED, integer_map, probe_directions

HEADER = ROOT / "include" / "crt_render.h"
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
FAKE = 1 << 20  # device pointers that are never dereferenced
FIELDS = ["texels", "face_size", "filter", "right", "up", "forward"]
FNS = ["crt_radiance_env_async", "crt_probes_env_async", "crt_render_lens_env_async", "crt_render_lens_env"]
NAN, INF = math.nan, math.inf


def test_header_exports_and_struct_agree(crt):
    from cpp_raytracer_amd import _capi
    text = HEADER.read_text()
    for value, name in enumerate(["CRT_ENV_NEAREST", "CRT_ENV_BILINEAR"]):
        assert re.search(rf"#define\s+{name}\s+{value}u", text), name
        assert getattr(_capi, name) == value == getattr(crt, name)
    body = re.search(r"typedef struct crt_env \{(.*?)\} crt_env;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") if decl.strip()
             for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?=,|$)", decl.strip())]
    assert names == [f for f, _ in _capi.EnvView._fields_] == FIELDS
    assert C.sizeof(_capi.EnvView) == 88
    assert [getattr(_capi.EnvView, f).offset for f in FIELDS] == [0, 8, 12, 16, 40, 64]
    for fn, nargs in zip(FNS, (9, 9, 7, 6)):
        proto = re.search(rf"int {fn}\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.EXPORTS[fn][1]) == nargs, fn
        assert hasattr(crt.lib(), fn)
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays
    for name in ["Env", "make_env", "CRT_ENV_NEAREST", "CRT_ENV_BILINEAR"]:
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


def call(crt, scene, fn, env, prm_over=None):
    """One call of `fn` with valid arguments of its own and `env` (None: a null pointer)."""
    from cpp_raytracer_amd import _capi
    lib, D3 = crt.lib(), _capi.D3
    pe = C.byref(env) if env is not None else None
    vp = C.c_void_p
    if fn == "crt_radiance_env_async":
        p = _capi.RadianceParams(50, 0, D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in (prm_over or {}).items():
            setattr(p, k, v)
        rc = lib.crt_radiance_env_async(scene.handle, 0, vp(FAKE), 8, None, C.byref(p), pe, vp(2 * FAKE), None)
    elif fn == "crt_probes_env_async":
        p = _capi.ProbeParams(16, 50, 0, 0, D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in (prm_over or {}).items():
            setattr(p, k, v)
        rc = lib.crt_probes_env_async(scene.handle, 0, vp(FAKE), None, 8, C.byref(p), pe, vp(2 * FAKE), None)
    else:
        lens = _capi.Lens(4, 0, D3(1.0, 2.0, 3.0), D3(1.0, 0.0, 0.0), D3(0.0, 1.0, 0.0), D3(0.0, 0.0, -1.0), 0.0, 0.0, 0)
        cam = _capi.Camera()
        cam.image_w, cam.image_h, cam.samples_per_pixel, cam.max_depth = 4, 24, 4, 50
        cam.background = D3(0.1, 0.2, 0.3)
        cam.t_min = 1e-5
        for k, v in (prm_over or {}).items():
            setattr(cam, k, v)
        if fn == "crt_render_lens_env_async":
            rc = lib.crt_render_lens_env_async(scene.handle, 0, C.byref(cam), C.byref(lens), pe, vp(2 * FAKE), None)
        else:
            rc = lib.crt_render_lens_env(scene.handle, 0, C.byref(cam), C.byref(lens), pe, vp(2 * FAKE))
    return rc, lib.crt_last_error().decode()


RULES = [
    (None, "env is null"),
    (dict(texels=None), "env->texels is null"),
    (dict(face_size=0), "face_size must be in 1 .. 16384"), (dict(face_size=16385), "face_size must be in 1 .. 16384"),
    (dict(face_size=0xFFFFFFFF), "face_size must be in 1 .. 16384"),
    (dict(filter=2), "unknown env->filter"), (dict(filter=0x80000000), "unknown env->filter"),
    (dict(right=(NAN, 0.0, 0.0)), "env basis .* must be finite"), (dict(up=(0.0, INF, 0.0)), "env basis .* must be finite"),
    (dict(forward=(0.0, 0.0, -INF)), "env basis .* must be finite"),
    # an earlier rule wins
    (dict(texels=None, face_size=0), "env->texels is null"), (dict(face_size=0, filter=9), "face_size must be"),
]


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("over,word", RULES, ids=[re.sub(r"\W+", "_", w)[:24] + str(i) for i, (_, w) in enumerate(RULES)])
def test_env_rules(crt, scene, fn, over, word):
    rc, msg = call(crt, scene, fn, None if over is None else env_view(**over))
    assert rc == -1 and re.search(fn + ": .*" + word, msg), (rc, msg)


@pytest.mark.parametrize("fn", FNS)
def test_the_calls_own_rules_come_first_and_still_hold(crt, scene, fn):
    over = dict(t_min=-1.0)
    rc, msg = call(crt, scene, fn, env_view(face_size=0), over)
    assert rc == -1 and re.search(fn + ": t_min must be finite", msg), (rc, msg)
    rc, msg = call(crt, scene, fn, env_view(), over)
    assert rc == -1 and re.search(fn + ": t_min must be finite", msg), (rc, msg)


def test_valid_envs_get_past_the_rules(crt, scene):
    """No rule broken: the call reaches the device layer (no device here, or the scene not uploaded;
    the blocking entry would upload it and read the fake texels, so it is called only where no device
    is visible). The basis is used as given: zero and unnormalised vectors are legal."""
    nodev = crt.device_count() == 0
    for over in (dict(), dict(face_size=1), dict(face_size=16384), dict(filter=0),
                 dict(right=(2.0, 0.0, 0.0), up=(0.0, 0.0, 0.0)), dict(forward=(1e300, -1e-300, 0.0))):
        for fn in FNS[:3] + (FNS[3:] if nodev else []):
            rc, msg = call(crt, scene, fn, env_view(**over))
            assert rc in (-3, -4), (fn, over, rc, msg)
            assert ("no HIP device" in msg) if rc == -3 else ("not uploaded" in msg)
    # depth 0 is still answered by the device layer (a memset), never by the rules
    rc, _ = call(crt, scene, FNS[0], env_view(), dict(max_depth=0))
    assert rc in (-3, -4)
    with pytest.raises(crt.CrtError, match=r"\((-3|-4)\)"):
        scene.radiance_async(0, FAKE, 4, 2 * FAKE, max_depth=5, background=(0, 0, 0), env=env_view())
    with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_radiance_env_async: unknown env->filter"):
        scene.radiance_async(0, FAKE, 4, 2 * FAKE, max_depth=5, background=(0, 0, 0), env=env_view(filter=7))
    with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_probes_env_async: env->texels is null"):
        scene.probes_async(0, FAKE, 0, 4, 2 * FAKE, samples=4, max_depth=5, background=(0, 0, 0), env=env_view(texels=None))


def test_python_argument_errors(crt, scene):
    import torch
    ok = torch.zeros((12, 2, 3), dtype=torch.float64)
    with pytest.raises(crt.CrtError, match="make_env: texels must be a contiguous \\(6n, n, 3\\) float64 tensor on a GPU"):
        crt.make_env(ok)  # a CPU tensor
    for bad in (torch.zeros((12, 2, 3), dtype=torch.float32), torch.zeros((12, 3, 3), dtype=torch.float64),
                torch.zeros((12, 2, 4), dtype=torch.float64), torch.zeros((72,), dtype=torch.float64),
                np.zeros((12, 2, 3)), None):
        with pytest.raises(crt.CrtError, match="make_env: texels must be"):
            crt.make_env(bad)
    with pytest.raises(crt.CrtError, match="make_env: filter must be one of"):
        crt.make_env(ok, filter="trilinear")
    cam = crt.resolve_camera(crt.SceneData.named("cornell").camera, 0)
    lens = crt.make_lens("equirect")
    with pytest.raises(crt.CrtError, match="render_lens: env must be an Env"):
        scene.render_lens(cam, lens, env=ok)
    with pytest.raises(crt.CrtError, match="radiance: env must be an Env"):
        scene.radiance(torch.zeros((5, 6), dtype=torch.float64), env=env_view())
    with pytest.raises(crt.CrtError, match="probes: env must be an Env"):
        scene.probes(torch.zeros((5, 3), dtype=torch.float64), env="sky")


def test_env_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "env_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "env_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()


# ---- csrc/crt_env.h on the host -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lookup(tmp_path_factory):
    so = tmp_path_factory.mktemp("env_lookup") / "env_lookup_check.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                        f"-I{ROOT / 'cpp_raytracer_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "env_lookup_check.cpp"),
                        "-o", str(so)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(so))
    lib.env_lookup_many.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.env_lookup_many.restype = None
    assert lib.env_sizeof() == 88

    def lookup(env, dirs, bg):
        from cpp_raytracer_amd import _capi
        D3 = _capi.D3
        t = np.ascontiguousarray(env.texels, np.float64)
        view = _capi.EnvView(t.ctypes.data, env.n, env.filter, D3(*env.right), D3(*env.up), D3(*env.forward))
        d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        b = np.array(bg, np.float64)
        out = np.full((len(d), 3), np.nan)
        lib.env_lookup_many(C.addressof(view), d.ctypes.data, len(d), b.ctypes.data, out.ctypes.data)
        return out
    return lookup


@pytest.mark.parametrize("filt", [em.NEAREST, em.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_the_kernels_lookup_is_the_models_on_the_host(host_lookup, n, filt):
    """Random, axis, diagonal, +-0 and 2^+-300 directions, the ones without a major axis, and directions
    a hair either side of every texel and face boundary; a random map in [0, 4) and the integer map."""
    rng = np.random.default_rng(n)
    edges = []
    for k in range(n + 1):  # u = 2 k / n - 1 and its neighbours, on +Z and +X
        u = 2.0 * k / n - 1.0
        for w in (math.nextafter(u, -2.0), u, math.nextafter(u, 2.0)):
            edges += [(w, 0.3, 1.0), (0.3, w, 1.0), (1.0, w, -w), (w, 1.0, 1.0), (1.0, 1.0, w)]
    bad = [(0.0, 0.0, 0.0), (NAN, 1.0, 0.0), (0.0, INF, 0.0), (-INF, INF, 1.0), (1.7e308, 1.7e308, -1.7e308)]
    dirs = np.concatenate([probe_directions(), np.array(edges), np.array(bad)])
    bg = (0.125, 0.25, 0.5)
    for texels in (rng.random((6 * n, n, 3)) * 4.0, integer_map(n)):
        for basis in (dict(), ROTATED):
            env = em.make(texels, filter=filt, **basis)
            want = em.lookup(env, dirs, bg)
            got = host_lookup(env, dirs, bg)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, filt, basis)
