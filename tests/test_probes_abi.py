"""CPU-side checks of the probe entries crt_probes_async, crt_probes, crt_probe_rays_async and
crt_sh_eval_async: the header, the exports and the ctypes mirror agree, and every argument rule is
refused with CRT_E_INVALID and a message naming it before any device work (so they hold on a machine
without a GPU: a call that got as far as looking for a device fails with CRT_E_NODEVICE, or
CRT_E_NOT_UPLOADED on one with a GPU). No kernel runs here (tests/test_gpu_probes.py runs them)."""
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
FIELDS = ["samples", "max_depth", "base_seed", "mode", "background", "t_min", "batch_probes", "flags"]


def test_header_exports_and_struct_agree(crt):
    from cpp_raytracer_amd import _capi
    text = HEADER.read_text()
    for name, value in (("CRT_PROBE_SPHERE", 0), ("CRT_PROBE_HEMISPHERE", 1), ("CRT_SH_RADIANCE", 0),
                        ("CRT_SH_IRRADIANCE", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}u", text), name
        assert getattr(_capi, name) == value == getattr(crt, name)
    body = re.search(r"typedef struct crt_probe_params \{(.*?)\} crt_probe_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in body.split(";") if decl.strip()
             for n in decl.split(None, 1)[1].split(",")]
    assert names == [f for f, _ in _capi.ProbeParams._fields_] == FIELDS
    assert C.sizeof(_capi.ProbeParams) == 56
    assert [getattr(_capi.ProbeParams, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 40, 48, 52]
    for fn, nargs in (("crt_probes_async", 8), ("crt_probes", 7), ("crt_probe_rays_async", 8), ("crt_sh_eval_async", 9)):
        proto = re.search(rf"int {fn}\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.EXPORTS[fn][1]) == nargs, fn
        assert hasattr(crt.lib(), fn)
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays


@pytest.fixture(scope="module")
def scene(crt):
    return crt.GpuScene(crt.SceneData.named("cornell"))


def params(over, hemisphere=False):
    from cpp_raytracer_amd import _capi
    p = _capi.ProbeParams(64, 50, 7, 1 if hemisphere else 0, _capi.D3(0.1, 0.2, 0.3), 1e-5, 0, 0)
    for k, v in over.items():
        setattr(p, k, _capi.D3(*v) if k == "background" else v)
    return p


def call(crt, scene, fn="crt_probes_async", points=FAKE, normals=0, n=8, prm="ok", out=2 * FAKE, out2=3 * FAKE,
         hemisphere=False, **over):
    p = params(over, hemisphere) if prm is not None else None
    pp = C.byref(p) if p is not None else None
    lib = crt.lib()
    if fn == "crt_probes_async":
        rc = lib.crt_probes_async(scene.handle, 0, C.c_void_p(points or None), C.c_void_p(normals or None), n, pp,
                                  C.c_void_p(out or None), None)
    elif fn == "crt_probes":
        rc = lib.crt_probes(scene.handle, 0, C.c_void_p(points or None), C.c_void_p(normals or None), n, pp,
                            C.c_void_p(out or None))
    else:
        rc = lib.crt_probe_rays_async(0, C.c_void_p(points or None), C.c_void_p(normals or None), n, pp,
                                      C.c_void_p(out or None), C.c_void_p(out2 or None), None)
    return rc, lib.crt_last_error().decode()


RULES = [
    (dict(prm=None), "params is null"),
    (dict(samples=0), "samples must be in 1 .. 2\\^20"), (dict(samples=(1 << 20) + 1), "samples must be in 1 .. 2\\^20"),
    (dict(samples=0xFFFFFFFF), "samples must be in 1 .. 2\\^20"),
    (dict(mode=2), "unknown mode"), (dict(mode=0x80000000), "unknown mode"),
    (dict(flags=2), "unknown flags"), (dict(flags=0x80000001), "unknown flags"),
    (dict(t_min=math.nan), "t_min must be finite, >= 0"), (dict(t_min=-1e-300), "t_min must be finite, >= 0"),
    (dict(t_min=math.inf), "t_min must be finite, >= 0"), (dict(t_min=2.0 ** 101), "<= 2\\^100"),
    (dict(background=(0.0, math.nan, 0.0)), "background must be finite"),
    (dict(background=(0.0, 0.0, -math.inf)), "background must be finite"),
    (dict(n=1 << 31), "more than 2\\^31-1 probes"), (dict(n=(1 << 40) + 5), "more than 2\\^31-1 probes"),
    (dict(hemisphere=True), "normals is null \\(CRT_PROBE_HEMISPHERE needs the normals\\)"),
    (dict(normals=4 * FAKE), "normals must be null with CRT_PROBE_SPHERE"),
    (dict(normals=4 * FAKE, n=0), "normals must be null with CRT_PROBE_SPHERE"),
    (dict(points=0), "points is null"), (dict(points=0, hemisphere=True, normals=4 * FAKE), "points is null"),
]


def rule_ids(rules):
    return [re.sub(r"\W+", "_", w)[:28] + str(i) for i, (_, w) in enumerate(rules)]


@pytest.mark.parametrize("fn", ["crt_probes_async", "crt_probes", "crt_probe_rays_async"])
@pytest.mark.parametrize("over,word", RULES, ids=rule_ids(RULES))
def test_argument_rules(crt, scene, fn, over, word):
    rc, msg = call(crt, scene, fn, **over)
    assert rc == -1 and re.search(fn + ": .*" + word, msg), (rc, msg)


def test_missing_outputs_and_the_record_limit(crt, scene):
    for fn, word in (("crt_probes_async", "d_coeff is null"), ("crt_probes", "coeff is null")):
        rc, msg = call(crt, scene, fn, out=0)
        assert rc == -1 and re.search(fn + ": " + word, msg), (rc, msg)
    for over in (dict(out=0), dict(out2=0)):
        rc, msg = call(crt, scene, "crt_probe_rays_async", **over)
        assert rc == -1 and "crt_probe_rays_async: d_rays or d_states is null" in msg, (rc, msg)
    rc, msg = call(crt, scene, "crt_probe_rays_async", n=(1 << 31) // 64, samples=64)  # 2^31 records
    assert rc == -1 and "crt_probe_rays_async: more than 2^31-1 records" in msg, (rc, msg)


def test_null_scene(crt):
    p = params({})
    assert crt.lib().crt_probes_async(None, 0, C.c_void_p(FAKE), None, 1, C.byref(p), C.c_void_p(FAKE), None) == -1
    assert b"crt_probes_async: scene is null" in crt.lib().crt_last_error()
    assert crt.lib().crt_probes(None, 0, C.c_void_p(FAKE), None, 1, C.byref(p), C.c_void_p(FAKE)) == -1
    assert b"crt_probes: scene is null" in crt.lib().crt_last_error()


def sh_eval(crt, coeff=FAKE, num_probes=4, index=2 * FAKE, dirs=3 * FAKE, m=8, what=0, out=4 * FAKE):
    rc = crt.lib().crt_sh_eval_async(0, C.c_void_p(coeff or None), num_probes, C.c_void_p(index or None),
                                     C.c_void_p(dirs or None), m, what, C.c_void_p(out or None), None)
    return rc, crt.lib().crt_last_error().decode()


SH_RULES = [
    (dict(what=2), "what must be CRT_SH_RADIANCE or CRT_SH_IRRADIANCE"), (dict(what=0xFFFFFFFF), "what must be"),
    (dict(m=1 << 31), "more than 2\\^31-1 queries"), (dict(m=(1 << 40) + 1), "more than 2\\^31-1 queries"),
    (dict(coeff=0), "d_coeff is null"), (dict(index=0), "d_index is null"), (dict(dirs=0), "d_dirs is null"),
    (dict(out=0), "d_rgb is null"),
]


@pytest.mark.parametrize("over,word", SH_RULES, ids=rule_ids(SH_RULES))
def test_sh_eval_rules(crt, over, word):
    rc, msg = sh_eval(crt, **over)
    assert rc == -1 and re.search("crt_sh_eval_async: .*" + word, msg), (rc, msg)


def test_valid_calls_get_past_the_rules(crt, scene):
    """A call that breaks no rule reaches the device layer: without a GPU that is the library's
    no-device error; with one, this scene was never uploaded (the two entries that take no scene would
    run on the fake pointers there, so they are called only where no device is visible). Empty calls
    are CRT_OK with no work, whatever the pointers."""
    for over in (dict(), dict(samples=1), dict(samples=1 << 20), dict(flags=1), dict(t_min=0.0), dict(t_min=2.0 ** 100),
                 dict(hemisphere=True, normals=4 * FAKE), dict(batch_probes=3), dict(max_depth=0)):
        rc, msg = call(crt, scene, **over)
        assert rc in (-3, -4), (over, rc, msg)
        assert ("no HIP device" in msg) if rc == -3 else ("not uploaded" in msg)
    assert call(crt, scene, n=0, points=0, out=0)[0] == 0
    assert call(crt, scene, "crt_probes", n=0, points=0, out=0)[0] == 0
    assert call(crt, scene, "crt_probe_rays_async", n=0, points=0, out=0, out2=0)[0] == 0
    assert sh_eval(crt, coeff=0, index=0, dirs=0, out=0, m=0)[0] == 0
    if crt.device_count() == 0:
        assert call(crt, scene, "crt_probe_rays_async")[0] == -3
        assert sh_eval(crt, what=1)[0] == -3
    with pytest.raises(crt.CrtError, match=r"\((-3|-4)\)"):
        scene.probes_async(0, FAKE, 0, 4, 2 * FAKE, samples=16, max_depth=5, background=(0, 0, 0))
    with pytest.raises(crt.CrtError, match=r"\(-1\).*unknown mode"):
        scene.probes_async(0, FAKE, 0, 4, 2 * FAKE, samples=16, mode=5, max_depth=5, background=(0, 0, 0))


def test_probes_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "probes_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "probes_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
