"""CPU-side checks of the radiance-query entries (crt_radiance_async, crt_radiance,
crt_camera_rays_async). No kernel runs here (tests/test_gpu_radiance.py runs them).

  - tests/radiance_model.py's camera rays are the reference's: at max_depth = 1 a sample's radiance is
    fixed by its primary ray alone (background on a miss, intensity * colour on a light, 0 otherwise),
    so the oracle's closest hits on the model's rays predict the oracle's per-sample radiance exactly.
  - the header, the exports and the ctypes mirror agree, and every argument rule is refused with
    CRT_E_INVALID and a message naming it before any device work.
  - GpuScene.radiance / camera_rays refuse wrong tensors and arguments with CrtError before any GPU
    call.
"""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

import radiance_model as rm
import ray_sets as rs
from conftest import ROOT
from oracle import crt_oracle_py as orc

HEADER = ROOT / "include" / "crt_render.h"
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
FAKE = 1 << 20  # device pointers that are never dereferenced


# ---- the model's primary rays against the oracle ----------------------------------------------------
@pytest.mark.parametrize("name,both", [("rtow_final", "miss and hit"), ("cornell", "light and non-light")])
def test_primary_rays_predict_the_oracles_depth_one_samples(crt, name, both):
    from cpp_raytracer_amd import CRT_DIFFUSE_LIGHT, camera_with
    d = rs.scene_data(crt, name)
    d.camera = camera_with(d.camera, image_w=24, image_h=16, samples_per_pixel=4, max_depth=1)
    if name == "rtow_final":
        assert d.camera.defocus_angle > 0  # the rejection loop runs
    seed = 31
    cam = crt.resolve_camera(d.camera, seed)
    rays, _ = rm.camera_rays(crt, cam)
    h = orc.hits(d, rays, cam.t_min)
    hit = h["prim"] >= 0
    mats = d.materials[h["material"]]
    light = hit & (mats["kind"] == CRT_DIFFUSE_LIGHT)
    want = np.zeros((len(rays), 3))
    want[~hit] = np.array(list(cam.background))
    want[light] = mats["color"][light] * mats["param"][light, None]
    if both == "miss and hit":
        assert (~hit).any() and hit.any()
    else:
        assert light.any() and (hit & ~light).any()
    _, smp = orc.render(d, seed, samples=True)
    assert np.array_equal(want.reshape(16, 24, 4, 3).view(np.uint64), smp.view(np.uint64))


def test_model_record_order_and_tiling(crt):
    """Records are pixel-major, samples inside; a tiling's records are the whole frame's for its
    owned rows; a sample window is a slice of the job's samples."""
    from cpp_raytracer_amd import Tiling, camera_with
    d = rs.scene_data(crt, "rtow_final")
    d.camera = camera_with(d.camera, image_w=6, image_h=10, samples_per_pixel=5)
    cam = crt.resolve_camera(d.camera, 3)
    rays, st = rm.camera_rays(crt, cam)
    assert rays.shape == (6 * 10 * 5, 6) and st.shape == (300,) and st.dtype == np.uint32
    t = Tiling(4, 3, 1, 0)
    tr, ts = rm.camera_rays(crt, cam, tiling=t)
    rows = rm.owned_rows(cam, t)
    assert rows == [4, 5, 6, 7]
    whole = rays.reshape(10, 6, 5, 6)
    assert np.array_equal(tr.view(np.uint64), whole[rows].reshape(-1, 6).view(np.uint64))
    assert np.array_equal(ts, st.reshape(10, 6, 5)[rows].reshape(-1))
    wr, ws = rm.camera_rays(crt, cam, 2, 2)
    assert np.array_equal(wr.view(np.uint64), whole[:, :, 2:4].reshape(-1, 6).view(np.uint64))
    assert np.array_equal(ws, st.reshape(10, 6, 5)[:, :, 2:4].reshape(-1))


# ---- header, exports, ctypes ------------------------------------------------------------------------
def test_header_export_and_struct_agree(crt):
    from cpp_raytracer_amd import _capi
    text = HEADER.read_text()
    assert re.search(r"#define\s+CRT_RADIANCE_PLAIN\s+1u", text)
    assert _capi.CRT_RADIANCE_PLAIN == 1 == crt.CRT_RADIANCE_PLAIN
    body = re.search(r"typedef struct crt_radiance_params \{(.*?)\} crt_radiance_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip() for decl in body.split(";") if decl.strip()
             for n in decl.split(None, 1)[1].split(",")]
    assert names == [f for f, _ in _capi.RadianceParams._fields_] == \
        ["max_depth", "base_seed", "background", "t_min", "flags", "reserved"]
    assert C.sizeof(_capi.RadianceParams) == 48
    assert [getattr(_capi.RadianceParams, f).offset for f in names] == [0, 4, 8, 32, 40, 44]
    for fn, nargs in (("crt_radiance_async", 8), ("crt_radiance", 7), ("crt_camera_rays_async", 8)):
        proto = re.search(r"int " + fn + r"\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.EXPORTS[fn][1]) == nargs, fn
        assert hasattr(crt.lib(), fn)
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays


@pytest.fixture(scope="module")
def scene(crt):
    return crt.GpuScene(crt.SceneData.named("cornell"))


def call(crt, scene, fn="crt_radiance_async", rays=FAKE, n=8, states=0, prm="ok", rgb=2 * FAKE, **over):
    from cpp_raytracer_amd import _capi
    p = None
    if prm is not None:
        p = _capi.RadianceParams(50, 0, _capi.D3(0.7, 0.8, 1.0), 1e-5, 0, 0)
        for k, v in over.items():
            setattr(p, k, _capi.D3(*v) if k == "background" else v)
    args = [scene.handle if scene is not None else None, 0, C.c_void_p(rays or None), n, C.c_void_p(states or None),
            C.byref(p) if p is not None else None, C.c_void_p(rgb or None)]
    if fn == "crt_radiance_async":
        args.append(None)
    rc = getattr(crt.lib(), fn)(*args)
    return rc, crt.lib().crt_last_error().decode()


# in the order the entry checks them (crt_trace_async's: scene, params, flags, interval, count, output, rays)
RULES = [
    (dict(prm=None), "params is null"),
    (dict(flags=2), "unknown flags"), (dict(flags=0x80000001), "unknown flags"),
    (dict(reserved=1), "reserved must be 0"),
    (dict(t_min=math.nan), "t_min must be finite, >= 0"), (dict(t_min=math.inf), "t_min must be finite, >= 0"),
    (dict(t_min=-1e-300), "t_min must be finite, >= 0"), (dict(t_min=2.0 ** 101), "t_min must be finite, >= 0"),
    (dict(background=(0.0, math.nan, 0.0)), "background must be finite"),
    (dict(background=(math.inf, 0.0, 0.0)), "background must be finite"),
    (dict(background=(0.0, 0.0, -math.inf)), "background must be finite"),
    (dict(n=1 << 31), "more than 2\\^31-1 rays"), (dict(n=(1 << 40) + 5), "more than 2\\^31-1 rays"),
    (dict(rgb=0), "d_rgb is null"), (dict(rays=0), "d_rays is null"),
    # an earlier rule wins
    (dict(flags=4, reserved=1, rays=0), "unknown flags"), (dict(t_min=-1.0, n=1 << 31), "t_min must be finite"),
]


@pytest.mark.parametrize("over,word", RULES, ids=[re.sub(r"\W+", "_", w)[:24] + str(i) for i, (_, w) in enumerate(RULES)])
def test_argument_rules(crt, scene, over, word):
    rc, msg = call(crt, scene, **over)
    assert rc == -1 and re.search("crt_radiance_async: .*" + word, msg), (rc, msg)
    if "rgb" not in over and "rays" not in over:  # the blocking entry names its own arguments
        rc, msg = call(crt, scene, fn="crt_radiance", **over)
        assert rc == -1 and re.search("crt_radiance: .*" + word, msg), (rc, msg)


def test_null_scene_and_no_work(crt, scene):
    rc, msg = call(crt, None)
    assert rc == -1 and "scene is null" in msg
    assert call(crt, scene, n=0, rays=0, rgb=0)[0] == 0  # n == 0: CRT_OK, nothing is looked at
    assert call(crt, scene, fn="crt_radiance", n=0, rays=0, rgb=0)[0] == 0


def test_valid_calls_get_past_the_rules(crt, scene):
    """A call that breaks no rule reaches the device layer: without a GPU that is the library's
    no-device error; with one, this scene was never uploaded. Depth 0, t_min = 0 and 2^100, states
    and the plain route are all legal."""
    for over in (dict(), dict(max_depth=0), dict(t_min=0.0), dict(t_min=2.0 ** 100), dict(flags=1), dict(states=3 * FAKE),
                 dict(base_seed=0xFFFFFFFF), dict(background=(-1.0, 0.0, 1e300))):
        rc, msg = call(crt, scene, **over)
        assert rc in (-3, -4), (over, rc, msg)
        assert ("no HIP device" in msg) if rc == -3 else ("not uploaded" in msg)
    with pytest.raises(crt.CrtError, match=r"\((-3|-4)\)"):
        scene.radiance_async(0, FAKE, 4, 2 * FAKE, max_depth=5, background=(0, 0, 0))
    with pytest.raises(crt.CrtError, match=r"\(-1\).*unknown flags"):
        scene.radiance_async(0, FAKE, 4, 2 * FAKE, max_depth=5, background=(0, 0, 0), flags=8)


def test_camera_rays_argument_rules(crt):
    from cpp_raytracer_amd import Tiling
    cam = crt.resolve_camera(crt.SceneData.named("cornell").camera, 0)
    f = crt.lib().crt_camera_rays_async

    def go(cam_ref=C.byref(cam), tiling=None, first=0, num=1, rays=FAKE, states=2 * FAKE):
        rc = f(0, cam_ref, tiling, first, num, C.c_void_p(rays or None), C.c_void_p(states or None), None)
        return rc, crt.lib().crt_last_error().decode()

    for kw, word in ((dict(cam_ref=None), "cam is null"), (dict(rays=0), "d_rays or d_states is null"),
                     (dict(states=0), "d_rays or d_states is null"),
                     (dict(first=0xFFFFFFFF, num=1), "first_sample \\+ num_samples exceeds")):
        rc, msg = go(**kw)
        assert rc == -1 and re.search("crt_camera_rays_async: " + word, msg), (kw, rc, msg)
    for t in (Tiling(0, 1, 0, 0), Tiling(4, 2, 2, 0), Tiling(4, 2, 0, 2)):
        rc, msg = go(tiling=C.byref(t))
        assert rc in (-1, -3) and (rc == -3 or "tiling" in msg), (rc, msg)  # after the device check


# ---- the torch front end refuses wrong tensors before any GPU call ----------------------------------
def test_python_argument_errors(crt, scene):
    import torch
    from cpp_raytracer_amd import Tiling
    ok = torch.zeros((5, 6), dtype=torch.float64)
    with pytest.raises(crt.CrtError, match="radiance: rays must be an \\(n, 6\\) float64 tensor on a GPU"):
        scene.radiance(ok)  # a CPU tensor
    for bad in (torch.zeros((5, 6), dtype=torch.float32), torch.zeros((5, 7), dtype=torch.float64),
                torch.zeros((30,), dtype=torch.float64), torch.zeros((5, 6), dtype=torch.int64)):
        with pytest.raises(crt.CrtError, match="radiance: rays must be"):
            scene.radiance(bad)
    cam = crt.resolve_camera(crt.SceneData.named("cornell").camera, 0)
    with pytest.raises(crt.CrtError, match="camera_rays: cam must be"):
        scene.camera_rays(crt.SceneData.named("cornell").camera)  # settings, not a resolved camera
    with pytest.raises(crt.CrtError, match="camera_rays: first_sample and num_samples"):
        scene.camera_rays(cam, first_sample=-1)
    with pytest.raises(crt.CrtError, match="camera_rays: first_sample and num_samples"):
        scene.camera_rays(cam, first_sample=cam.samples_per_pixel + 1)  # a negative default count
    with pytest.raises(crt.CrtError, match="camera_rays: first_sample \\+ num_samples"):
        scene.camera_rays(cam, first_sample=0xFFFFFFFF, num_samples=1)
    for t in (Tiling(0, 1, 0, 0), Tiling(4, 2, 2, 0), "whole"):
        with pytest.raises(crt.CrtError, match="camera_rays: bad tiling"):
            scene.camera_rays(cam, tiling=t)


def test_radiance_cpp_program_compiles_and_links(tmp_path):
    exe = tmp_path / "radiance_e2e"
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "radiance_e2e.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
