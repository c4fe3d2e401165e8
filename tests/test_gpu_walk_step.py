"""The hand-scheduled speculative link step (crt_device.hip link_spec_steps) at the shapes
tests/test_gpu_walk_masks.py's full 64-lane bands do not reach. Inside the block exec is the mask of
the lanes still in the wave's loop, so what matters is who is in exec when:
  partial waves    frames of 1 x 1, 5 x 3 and 16 x 1 pixels: lanes that never hold a unit are outside
                   the call's exec from the first step
  several waves    a 40 x 12 frame (partial tiles right and below): waves that drain apart
  f64 hand-back    the block leaves with the loop's exec, C++ decides the undecided lanes, and the
                   block is entered again: the pinned band with 8 such node tests, and a scene whose
                   rays lie on both sides of the f32 node test's range (tests/guard_cases.py, F =
                   2^-36), so that lanes are undecided in steps in which others decide and park
  flat instance    the parallelogram-only kernel (prim_mode 2) keeps the C++ loop (it leaves for the
                   f64 test too often for the block to pay); its link walk runs the same partial waves
  masked pass      the MASK instance: one adaptive pass with two of four blocks stopped
Every case runs the link walk and the stack walk (CRT_NO_LINK_WALK=1) of the same build: frames
bit-identical, the frame the oracle's at tests/test_gpu_parity.py's tolerance, the instrumented
pass's counters (plain and speculative, CRT_COUNT_SPEC=1: the loop under test) equal, Schlick
guard 0."""
import numpy as np
import pytest

import guard_cases as gc
import plan_worlds as pw
from oracle import crt_oracle_py as orc
from test_gpu_link_walk import TOL, balanced_row
from test_gpu_walk_masks import COUNTERS, PARENT_SPEC, ROW, SCENES, both_walks

pytestmark = pytest.mark.gpu


def framed(d, w, h, spp):
    from cpp_raytracer_amd import camera_with
    d.camera = camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp)
    return d


# What a frame of several tiles leaves to chance: its waves take their tiles from a shared queue, so
# which rays share a wave, and with it the wave's trip counts and the speculative walk's extra node
# visits, differ from run to run of one and the same walk (profiles/r08_masks/README.md). Such
# frames compare the counts that belong to the rays alone.
PER_WAVE = {"plain": ("wave_iters_walk",), "spec": ("wave_iters_walk", "nodes_visited", "slow_node_tests")}


def check(links, stack, d, seed, shape, one_wave=True):
    assert np.isfinite(links[0]).all() and links[0].shape[:2] == shape
    assert np.array_equal(links[0].view(np.uint64), stack[0].view(np.uint64))
    for i, name in ((1, "plain"), (2, "spec")):
        skip = () if one_wave else PER_WAVE[name]
        a, b = ({k: v for k, v in w[i].items() if k not in skip} for w in (links, stack))
        assert a == b, name + " pass"
    plain, spec = links[1], links[2]
    for k in ("rays", "sphere_tests", "candidate_tests"):  # the speculative walk adds node visits alone
        assert spec[k] == plain[k], k
    assert spec["nodes_visited"] >= plain["nodes_visited"] >= plain["rays"] and spec["wave_iters_walk"] > 0
    want = orc.render(d, seed, threads=16)
    err = np.abs(links[0] - want)
    print(f"plain {plain} speculative {spec}; max |gpu - oracle| = {err.max():.3g}")
    assert err.max() <= TOL and err.max() <= 1e-12 * max(1.0, np.abs(want).max())
    return plain, spec


@pytest.mark.parametrize("spp", [2, 5])
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (16, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene", ["leaf_root", "two_leaves", "row"])
def test_partial_waves(crt, monkeypatch, scene, size, spp):
    d, kw = SCENES[scene](crt)
    d = framed(d, size[0], size[1], spp)
    links, stack = both_walks(crt, monkeypatch, d, kw, 51 + spp)
    plain, _ = check(links, stack, d, 51 + spp, (size[1], size[0]))
    assert plain["rays"] >= size[0] * size[1] * spp
    assert size[0] * size[1] < 64  # fewer pixels than lanes: part of the wave never holds a unit


@pytest.mark.parametrize("scene", ["sparse", "row"])
def test_several_waves_draining_apart(crt, monkeypatch, scene):
    d, kw = SCENES[scene](crt)
    d = framed(d, 40, 12, 3)  # 3 x 3 tiles of 16 x 4, the right and the bottom ones partial
    links, stack = both_walks(crt, monkeypatch, d, kw, 61)
    plain, spec = check(links, stack, d, 61, (12, 40), one_wave=False)
    assert plain["rays"] >= 40 * 12 * 3 and spec["nodes_visited"] > plain["nodes_visited"]


def test_hand_back_in_the_pinned_band(crt, monkeypatch):
    """test_gpu_walk_masks' row band at 2 spp: 8 node tests go to f64 while other lanes park."""
    d, kw = balanced_row(crt, ROW)
    d = framed(d, 16, 4, 2)
    links, stack = both_walks(crt, monkeypatch, d, kw, 33)
    _, spec = check(links, stack, d, 33, (4, 16))
    assert spec == PARENT_SPEC["row", 2] and spec["slow_node_tests"] == 8


def test_hand_back_with_lanes_on_both_sides_of_the_f32_range(crt, monkeypatch):
    """F = 2^-36: the jittered samples near the centre columns and rows are outside the f32 node
    test's range (marg = inf: undecided at every node), their neighbours inside it."""
    d = gc.scene(crt, "spheres", 0, -36, "origin")
    links, stack = both_walks(crt, monkeypatch, d, {}, gc.BASE_SEED)
    _, spec = check(links, stack, d, gc.BASE_SEED, (gc.H, gc.W), one_wave=False)
    # some node tests in f64 and not all (test_gpu_range_guards' bound for this case)
    assert 0 < spec["slow_node_tests"] < spec["nodes_visited"]


def test_hand_back_on_both_sides_of_the_f32_range_in_one_wave(crt, monkeypatch):
    """The same scene in one tile of 16 x 4 pixels (a pixel is 2^-38.5 wide here, so the samples of
    the two centre columns and rows still fall on both sides of 2^-39): one wave does all the work, and
    every counter of the speculative pass, the f64 node tests among them, is compared between the walks."""
    d = framed(gc.scene(crt, "spheres", 0, -36, "origin"), 16, 4, gc.SPP)
    links, stack = both_walks(crt, monkeypatch, d, {}, gc.BASE_SEED)
    _, spec = check(links, stack, d, gc.BASE_SEED, (4, 16))
    assert 0 < spec["slow_node_tests"] < spec["nodes_visited"]


def flat_walks(crt, env, d, seed):
    """both_walks for the flat-parallelogram instance (its plan differs: prim_mode 2)."""
    counters = COUNTERS + ("parallelogram_tests",)
    out = {}
    s = crt.GpuScene(d)
    try:
        p = s.launch_plan("render")
        assert p.five_waves == 1 and p.prim_mode == 2 and p.klass == pw.LDS_SCENE
        cam = crt.resolve_camera(d.camera, seed)
        for walk in ("links", "stack"):
            if walk == "stack":
                env.setenv("CRT_NO_LINK_WALK", "1")
            frame, _ = s.render(cam, 1)
            assert s.last_walk(0) == walk
            counts = []
            for spec in (False, True):
                if spec:
                    env.setenv("CRT_COUNT_SPEC", "1")
                st = s.render_count(0, cam)
                assert s.last_walk(0) == walk
                counts.append({k: int(getattr(st, k)) for k in counters})
            env.delenv("CRT_COUNT_SPEC")
            out[walk] = (frame, counts[0], counts[1])
        env.delenv("CRT_NO_LINK_WALK")
        assert s.guard(0) == 0
    finally:
        s.close()
    return out["links"], out["stack"]


@pytest.mark.parametrize("size", [(16, 4), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_flat_parallelogram_instance(crt, monkeypatch, size):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named("cornell", None)
    d.camera = camera_with(d.camera, image_w=size[0], image_h=size[1], samples_per_pixel=4, max_depth=12)
    links, stack = flat_walks(crt, monkeypatch, d, 71)
    plain, spec = check(links, stack, d, 71, (size[1], size[0]))
    assert spec["parallelogram_tests"] == plain["parallelogram_tests"] > 0
    assert spec["slow_node_tests"] > 0  # Cornell's faces lie on node bounds: ties for f64


def test_masked_pass(crt, monkeypatch):
    """One pass over all 8 samples of a 32 x 8 frame (2 x 2 blocks) with blocks 1 and 2 stopped."""
    import torch
    from cpp_raytracer_amd import camera_with
    w, h, spp, stopped = 32, 8, 8, 0x80000000
    d = crt.SceneData.named("rtow_final", 42)
    d.camera = camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp, max_depth=50)
    on = np.array([True, False, False, True])
    inside = torch.from_numpy(np.repeat(np.repeat(on.reshape(2, 2), 4, axis=0), 16, axis=1)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    s = crt.GpuScene(d)
    got = {}
    try:
        p = s.launch_plan("render")
        assert p.five_waves == 1 and p.prim_mode == 0 and crt.block_count(w, h) == 4
        s.upload(0)
        cam = crt.resolve_camera(d.camera, 81)
        for walk in ("links", "stack"):
            if walk == "stack":
                monkeypatch.setenv("CRT_NO_LINK_WALK", "1")
            total, nz, out = (torch.full((h, w, k), float("nan"), dtype=torch.float64, device="cuda") for k in (3, 2, 3))
            blocks = torch.from_numpy(np.where(on, 0, stopped).astype(np.uint32).view(np.int32).copy()).cuda()
            s.render_pass_masked(0, cam, 0, spp, total.data_ptr(), nz.data_ptr(), out.data_ptr(), blocks.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            assert s.last_walk(0) == walk
            words = blocks.cpu().numpy().view(np.uint32)
            assert (words[on] == spp).all() and (words[~on] == stopped).all()
            assert all((t[~inside] == 0).all() for t in (total, nz, out))
            counts = []
            for spec in (False, True):
                if spec:
                    monkeypatch.setenv("CRT_COUNT_SPEC", "1")
                st = s.render_count(0, cam)
                counts.append({k: int(getattr(st, k)) for k in COUNTERS})
            monkeypatch.delenv("CRT_COUNT_SPEC")
            got[walk] = ([t.cpu().numpy() for t in (total, nz, out)], counts)
        monkeypatch.delenv("CRT_NO_LINK_WALK")
        assert s.guard(0) == 0
    finally:
        s.close()
    for a, b in zip(got["links"][0], got["stack"][0]):
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for i, name in ((0, "plain"), (1, "spec")):  # four tiles: the per-ray counts (check())
        a, b = ({k: v for k, v in got[w][1][i].items() if k not in PER_WAVE[name]} for w in ("links", "stack"))
        assert a == b and a["rays"] >= w * h * spp, name
    want = orc.render(d, 81, threads=16)
    m = inside.cpu().numpy()
    err = np.abs(got["links"][0][2] - want)[m]
    print(f"masked pass: max |gpu - oracle| in the active blocks = {err.max():.3g}")
    assert err.max() <= TOL and err.max() <= 1e-12 * max(1.0, np.abs(want).max())
