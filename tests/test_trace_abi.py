"""CPU-side checks of the ray-query entry crt_trace_async: the header, the export and the ctypes
mirror agree, and every argument rule is refused with CRT_E_INVALID and a message naming it before
any device work (so they hold on a machine without a GPU: a call that got as far as looking for a
device fails with CRT_E_NODEVICE, or CRT_E_NOT_UPLOADED on one with a GPU). No kernel runs here
(tests/test_gpu_trace.py runs them)."""
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


def test_header_export_and_struct_agree(crt):
    from cpp_raytracer_amd import _capi
    text = HEADER.read_text()
    assert re.search(r"#define\s+CRT_TRACE_ANY\s+1u", text) and re.search(r"#define\s+CRT_TRACE_PLAIN\s+2u", text)
    assert (_capi.CRT_TRACE_ANY, _capi.CRT_TRACE_PLAIN) == (1, 2) == (crt.CRT_TRACE_ANY, crt.CRT_TRACE_PLAIN)
    body = re.search(r"typedef struct crt_trace_params \{(.*?)\} crt_trace_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f for f, _ in _capi.TraceParams._fields_] == ["t_min", "t_max", "flags", "reserved"]
    assert C.sizeof(_capi.TraceParams) == 24
    assert [getattr(_capi.TraceParams, f).offset for f in names] == [0, 8, 16, 20]
    proto = re.search(r"int crt_trace_async\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_capi.EXPORTS["crt_trace_async"][1]) == 9
    assert hasattr(crt.lib(), "crt_trace_async")
    assert C.sizeof(_capi.Hit) == crt.HIT_DTYPE.itemsize == 72
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays


@pytest.fixture(scope="module")
def scene(crt):
    return crt.GpuScene(crt.SceneData.named("cornell"))


def call(crt, scene, rays=FAKE, n=8, tmax=0, prm="ok", hits=2 * FAKE, occ=0, **over):
    from cpp_raytracer_amd import _capi
    p = None
    if prm is not None:
        p = _capi.TraceParams(1e-5, math.inf, 0, 0)
        for k, v in over.items():
            setattr(p, k, v)
    rc = crt.lib().crt_trace_async(scene.handle, 0, C.c_void_p(rays or None), n, C.c_void_p(tmax or None),
                                   C.byref(p) if p is not None else None, C.c_void_p(hits or None),
                                   C.c_void_p(occ or None), None)
    return rc, crt.lib().crt_last_error().decode()


RULES = [
    (dict(prm=None), "params is null"),
    (dict(flags=4), "unknown flags"), (dict(flags=0x80000001, hits=0, occ=FAKE), "unknown flags"),
    (dict(reserved=1), "reserved must be 0"),
    (dict(t_min=math.nan), "t_min must be finite"), (dict(t_min=math.inf), "t_min must be finite"),
    (dict(t_min=-math.inf), "t_min must be finite"), (dict(t_max=math.nan), "t_max must not be NaN"),
    (dict(n=1 << 31), "more than 2\\^31-1 rays"), (dict(n=(1 << 40) + 5), "more than 2\\^31-1 rays"),
    (dict(rays=0), "d_rays is null"),
    (dict(hits=0), "d_hits is null"), (dict(occ=3 * FAKE), "d_occluded must be null without CRT_TRACE_ANY"),
    (dict(flags=1), "d_hits must be null with CRT_TRACE_ANY"), (dict(flags=1, hits=0), "d_occluded is null"),
    (dict(flags=3), "d_hits must be null with CRT_TRACE_ANY"),
    (dict(flags=2, hits=0, occ=3 * FAKE), "d_occluded must be null without CRT_TRACE_ANY"),
]


@pytest.mark.parametrize("over,word", RULES, ids=[re.sub(r"\W+", "_", w)[:28] + str(i) for i, (_, w) in enumerate(RULES)])
def test_argument_rules(crt, scene, over, word):
    rc, msg = call(crt, scene, **over)
    assert rc == -1 and re.search("crt_trace_async: .*" + word, msg), (rc, msg)


def test_null_scene(crt):
    from cpp_raytracer_amd import _capi
    p = _capi.TraceParams(1e-5, math.inf, 0, 0)
    assert crt.lib().crt_trace_async(None, 0, C.c_void_p(FAKE), 1, None, C.byref(p), C.c_void_p(FAKE), None, None) == -1
    assert b"scene is null" in crt.lib().crt_last_error()


def test_valid_call_gets_past_the_rules(crt, scene):
    """A call that breaks no rule reaches the device layer: without a GPU that is the library's
    no-device error; with one, this scene was never uploaded. The same for t_max = +-inf, a
    negative t_min and both flags, which are all legal."""
    for over in (dict(), dict(t_max=-math.inf), dict(t_min=-1.0, t_max=5.0), dict(flags=3, hits=0, occ=FAKE),
                 dict(flags=2), dict(tmax=3 * FAKE)):
        rc, msg = call(crt, scene, **over)
        assert rc in (-3, -4), (over, rc, msg)
        assert ("no HIP device" in msg) if rc == -3 else ("not uploaded" in msg)
    with pytest.raises(crt.CrtError, match=r"\((-3|-4)\)"):
        scene.trace_async(0, FAKE, 4, hits_ptr=2 * FAKE)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*unknown flags"):
        scene.trace_async(0, FAKE, 4, hits_ptr=2 * FAKE, flags=8)


def test_trace_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "trace_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "trace_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
