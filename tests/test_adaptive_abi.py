"""CPU-side checks of the adaptive-sampling entry points: the exports and the Python binding, the
argument rules (refused before any device work, so they hold on a machine without a GPU), the
block count, the checkpoint guard of AdaptiveRender.resume, and the C++ drop-in's render_adaptive
compiling and linking. No kernel runs here (tests/test_gpu_adaptive.py runs them)."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
NEW = ("crt_block_count", "crt_render_pass_masked_async", "crt_adaptive_update", "crt_render_adaptive")
FAKE = 4096  # a device pointer that is never dereferenced: every call given it is refused first


def test_exports_contain_adaptive_entry_points(crt):
    from cpp_raytracer_amd import _capi
    for name in NEW:
        assert name in _capi.EXPORTS
        assert hasattr(crt.lib(), name)
    assert _capi.EXPORTS["crt_render_adaptive"][1][4] is _capi.ADAPTIVE_FN
    assert (_capi.CRT_BLOCK_W, _capi.CRT_BLOCK_H, _capi.CRT_BLOCK_STOPPED) == (16, 4, 0x80000000)
    assert crt.CRT_BLOCK_STOPPED == 0x80000000
    assert crt.lib().crt_abi_version() == 2  # additive: the ABI version stays


@pytest.mark.parametrize("w,rows,want", [(50, 30, 32), (16, 4, 1), (17, 5, 4), (1200, 800, 75 * 200), (16, 0, 0)])
def test_block_count(crt, w, rows, want):
    assert crt.block_count(w, rows) == want
    assert crt.lib().crt_block_count(w, rows) == want


@pytest.fixture
def job(crt):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named("config1")
    d.camera = camera_with(d.camera, image_w=50, image_h=30, samples_per_pixel=22)
    return crt.GpuScene(d), crt.resolve_camera(d.camera, 5)


def test_masked_pass_rules_are_checked_before_any_device_work(crt, job):
    """crt_render_pass_masked_async has crt_render_pass_async's rules and names the broken one."""
    from cpp_raytracer_amd import Tiling
    scene, cam = job
    for first, count, ptr, blocks, tiling, word in [
            (2, 4, FAKE, FAKE, None, "multiple of the chunk length"), (0, 0, FAKE, FAKE, None, "num_samples is 0"),
            (20, 4, FAKE, FAKE, None, "exceeds samples_per_pixel"), (0, 6, FAKE, FAKE, None, "neither a multiple"),
            (0, 8, 0, FAKE, None, "d_sum is null"), (0, 8, FAKE, 0, None, "d_blocks is null"),
            (0, 8, FAKE, FAKE, Tiling(2, 2, 0, 0), "row_block a multiple of 4"),
            (0, 8, FAKE, FAKE, Tiling(6, 3, 1, 1), "row_block a multiple of 4")]:
        with pytest.raises(crt.CrtError, match=word):
            scene.render_pass_masked(0, cam, first, count, ptr, FAKE, 0, blocks, 0, 0, tiling)


def test_update_rules_are_checked_before_any_device_work(crt, job):
    from cpp_raytracer_amd import Tiling
    _, cam = job
    for threshold in (-0.5, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(crt.CrtError, match="threshold must be finite"):
            crt.adaptive_update(0, cam, FAKE, FAKE, 8, threshold)
    with pytest.raises(crt.CrtError, match="row_block a multiple of 4"):
        crt.adaptive_update(0, cam, FAKE, FAKE, 8, 0.1, tiling=Tiling(2, 2, 0, 0))
    with pytest.raises(crt.CrtError, match="null argument"):
        crt.adaptive_update(0, cam, FAKE, 0, 8, 0.1)
    with pytest.raises(crt.CrtError, match="exceeds samples_per_pixel"):
        crt.adaptive_update(0, cam, FAKE, FAKE, 24, 0.1)
    with pytest.raises(crt.CrtError, match="not a pass boundary"):
        crt.adaptive_update(0, cam, FAKE, FAKE, 10, 0.1)  # 22 spp: chunks of 4


def test_blocking_api_rules(crt, job):
    scene, cam = job
    for threshold in (-1.0, float("nan"), float("inf")):
        with pytest.raises(crt.CrtError, match="threshold must be finite"):
            scene.render_adaptive(cam, threshold)
    import ctypes as C
    from cpp_raytracer_amd import _capi
    out = np.zeros((30, 50, 3))
    prm = _capi.AdaptiveParams(0.1, 8, 8, 0, 1)  # reserved != 0
    assert crt.lib().crt_render_adaptive(scene.handle, C.byref(cam), 1, C.byref(prm), _capi.ADAPTIVE_FN(), None,
                                         out.ctypes.data, None, None) == -1
    assert b"reserved must be 0" in crt.lib().crt_last_error()


def test_adaptive_render_rejects_a_degenerate_tiling(crt, job):
    from cpp_raytracer_amd import Tiling
    from cpp_raytracer_amd.adaptive import AdaptiveRender
    scene, cam = job
    for t in (Tiling(0, 1, 0, 0), Tiling(4, 0, 0, 0), Tiling(4, 2, 2, 0), Tiling(2, 2, 0, 0)):
        with pytest.raises(crt.CrtError, match="tiling"):
            AdaptiveRender(scene, cam, 0.1, 8, tiling=t)


def _state(cam, **over):
    words = np.full(32, 8, np.uint32)
    words[:5] |= np.uint32(0x80000000)
    s = {"sum": np.zeros((cam.image_h, cam.image_w, 3)), "noise": np.zeros((cam.image_h, cam.image_w, 2)),
         "samples_done": 8, "spp": int(cam.samples_per_pixel), "base_seed": int(cam.base_seed),
         "width": int(cam.image_w), "height": int(cam.image_h), "tiling": np.array([1, 1, 0, 0], np.uint32),
         "blocks": words, "threshold": 0.1, "min_samples": 8}
    s.update(over)
    return {k: v for k, v in s.items() if v is not None}


@pytest.mark.parametrize("over", [dict(spp=24), dict(base_seed=6), dict(width=51), dict(height=31),
                                  dict(samples_done=7), dict(samples_done=23), dict(sum=np.zeros((30, 49, 3))),
                                  dict(blocks=np.full(31, 8, np.uint32)), dict(blocks=np.full(32, 12, np.uint32)),
                                  dict(blocks=np.full(32, 4, np.uint32)), dict(blocks=None), dict(threshold=None),
                                  dict(noise=None), dict(tiling=np.array([2, 2, 0, 0], np.uint32))],
                         ids=["spp", "seed", "width", "height", "done_off_chunk", "done_past_end", "sum_shape",
                              "block_count", "blocks_ahead", "active_blocks_behind", "no_blocks", "no_threshold",
                              "no_noise", "tiling"])
def test_resume_rejects_a_state_of_another_job(crt, job, over):
    """A checkpoint continues only the job it was taken from, and only with block words that fit
    it; refused before anything touches a device."""
    from cpp_raytracer_amd.adaptive import AdaptiveRender
    scene, cam = job
    with pytest.raises(crt.CrtError, match="resume|tiling"):
        AdaptiveRender.resume(scene, cam, _state(cam, **over))


@pytest.mark.parametrize("name,inc", [("adaptive_e2e", INC), ("passes_e2e", ROOT / "include")])
def test_adaptive_cpp_program_compiles_and_links(tmp_path, name, inc):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++20", "-O2", f"-I{inc}", str(ROOT / "tests" / "cpp" / f"{name}.cpp"),
                        "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
