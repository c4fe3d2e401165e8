"""The speculative walk's state in lane masks (crt_device.hip walk(), SPEC): a parking
lane stays on its node instead of popping and undoing the pop, and "no leaf recorded yet" is a lane
mask updated at the first leaf instead of a compare of the recorded node every step. Every outcome a
lane can have in the wave's loop, in one wave: a one-tile band of 16 x 4 pixels (64 lanes) at 2 and at
5 samples a pixel (the second crosses a chunk boundary), on
  leaf_root   a root that is a leaf: every lane records it in its first step and parks on the sentinel
  two_leaves  one interior node: lanes record a leaf and park on the other, or on the sentinel
  row         test_gpu_link_walk's balanced row at the link side of its capacity edge (191 spheres,
              one a leaf, depth 9): long walks, lanes parking early beside lanes still descending
  sparse      six spheres in a frame four times as wide as their cluster: most rays enter no leaf and reach
              the sentinel with nothing recorded while their neighbours park on a second leaf
each through the link walk and through the stack walk (CRT_NO_LINK_WALK=1). The two walks' frames are
bit-identical and the frame is the oracle's at tests/test_gpu_parity.py's tolerance. The instrumented
pass is run twice per walk: with its plain walk, and under CRT_COUNT_SPEC=1, where it walks
speculatively like the timed kernel, the loop under test. Both sets of counters are equal between
the two walks, the speculative pass differs from the plain one in node visits alone, and its counters
are those the build before this change gave (PARENT_SPEC)."""
import numpy as np
import pytest

import plan_worlds as pw
from oracle import crt_oracle_py as orc
from test_gpu_link_walk import TOL, balanced_row, region

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "nodes_visited", "sphere_tests", "candidate_tests", "wave_iters_walk", "slow_node_tests")
ROW = 191  # test_gpu_link_walk's capacity_edge()[0]; checked against the plan below


def band(d, spp):
    from cpp_raytracer_amd import camera_with
    d.camera = camera_with(d.camera, image_w=16, image_h=4, samples_per_pixel=spp)
    return d


def sparse(crt):
    from cpp_raytracer_amd import camera_with
    d, _ = pw.world(crt, "cloud", 6)
    objs = d.objects.copy()
    objs["v"][:, 3] = 2.5
    d.objects = objs
    # 16 x 4 pixels over 64 x 16 units at the cluster's distance; the cluster spans 16
    d.camera = camera_with(d.camera, fov=float(2 * np.arctan(8 / 44)))
    return d, dict(max_prims_in_node=1)


def near(crt, n, **kw):
    """plan_worlds' first n cloud spheres at radius 3 in a frame of 32 x 8 units at their distance:
    about half the 64 pixels see one."""
    from cpp_raytracer_amd import camera_with
    d, _ = pw.world(crt, "cloud", n)
    objs = d.objects.copy()
    objs["v"][:, 3] = 3.0
    d.objects = objs
    d.camera = camera_with(d.camera, fov=float(2 * np.arctan(4 / 44)))
    return d, kw


SCENES = {
    "leaf_root": lambda crt: near(crt, 1),
    "two_leaves": lambda crt: near(crt, 2, max_prims_in_node=1),
    "row": lambda crt: balanced_row(crt, ROW),
    "sparse": sparse,
}


def both_walks(crt, env, d, kw, base_seed):
    """{walk: (frame, the instrumented pass's counters with its plain walk, the same with the
    speculative walk)} for the link and the stack walk. render_count walks speculatively, as the
    timed kernel does, only under CRT_COUNT_SPEC=1 (read at the call): that is the pass that runs
    the loop under test; the plain pass counts the reference's own visits. `env` is a
    pytest.MonkeyPatch."""
    out = {}
    s = crt.GpuScene(d, **kw)
    try:
        p = s.launch_plan("render")
        assert p.five_waves == 1 and p.prim_mode == 0 and 16 * p.num_nodes <= region(p)
        cam = crt.resolve_camera(d.camera, base_seed)
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
                counts.append({k: int(getattr(st, k)) for k in COUNTERS})
            env.delenv("CRT_COUNT_SPEC")
            out[walk] = (frame, counts[0], counts[1])
        env.delenv("CRT_NO_LINK_WALK")
        assert s.guard(0) == 0
    finally:
        s.close()
    return out["links"], out["stack"]


# The speculative pass's counters of the parent of the commit that moved the walk's state into lane masks,
# measured with that build through this module's both_walks (link and stack walk alike, the same in
# repeated runs: a band of one tile is one wave's work at a time). The node sequence is the same as
# before, not merely the same between the two walks.
PARENT_SPEC = {
    ("leaf_root", 2): dict(rays=139, nodes_visited=139, sphere_tests=24, candidate_tests=22, wave_iters_walk=6, slow_node_tests=0),
    ("leaf_root", 5): dict(rays=349, nodes_visited=349, sphere_tests=64, candidate_tests=58, wave_iters_walk=17, slow_node_tests=0),
    ("row", 2): dict(rays=143, nodes_visited=1306, sphere_tests=403, candidate_tests=214, wave_iters_walk=201, slow_node_tests=8),
    ("row", 5): dict(rays=345, nodes_visited=2910, sphere_tests=862, candidate_tests=482, wave_iters_walk=525, slow_node_tests=0),
    ("sparse", 2): dict(rays=144, nodes_visited=445, sphere_tests=45, candidate_tests=33, wave_iters_walk=73, slow_node_tests=0),
    ("sparse", 5): dict(rays=363, nodes_visited=1086, sphere_tests=120, candidate_tests=89, wave_iters_walk=217, slow_node_tests=0),
    ("two_leaves", 2): dict(rays=140, nodes_visited=242, sphere_tests=27, candidate_tests=24, wave_iters_walk=14, slow_node_tests=0),
    ("two_leaves", 5): dict(rays=350, nodes_visited=604, sphere_tests=72, candidate_tests=60, wave_iters_walk=37, slow_node_tests=0),
}


@pytest.mark.parametrize("spp", [2, 5])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_walks_agree_and_match_the_oracle(crt, monkeypatch, scene, spp):
    d, kw = SCENES[scene](crt)
    d = band(d, spp)
    links, stack = both_walks(crt, monkeypatch, d, kw, 31 + spp)
    assert np.isfinite(links[0]).all() and links[0].shape[:2] == (4, 16)
    assert np.array_equal(links[0].view(np.uint64), stack[0].view(np.uint64))
    assert links[1] == stack[1], "plain pass"
    assert links[2] == stack[2], "speculative pass"
    plain, spec = links[1], links[2]
    print(f"{scene} {spp} spp: plain {plain} speculative {spec}")
    # the speculative walk adds node visits and nothing else (walk(), SPEC)
    for k in ("rays", "sphere_tests", "candidate_tests"):
        assert spec[k] == plain[k], k
    assert spec["nodes_visited"] >= plain["nodes_visited"] and spec["wave_iters_walk"] > 0
    assert plain["rays"] >= 64 * spp
    assert plain["nodes_visited"] >= plain["rays"]  # every ray tests the root
    if scene != "leaf_root":
        assert plain["nodes_visited"] > plain["rays"]
    if scene in ("row", "sparse"):
        assert spec["nodes_visited"] > plain["nodes_visited"]  # lanes did walk on past their first leaf
    assert spec == PARENT_SPEC[scene, spp]
    want = orc.render(d, 31 + spp, threads=16)
    err = np.abs(links[0] - want)
    print(f"{scene} {spp} spp: max |gpu - oracle| = {err.max():.3g}")
    assert err.max() <= TOL and err.max() <= 1e-12 * max(1.0, np.abs(want).max())
    if scene == "sparse":
        _, counts = np.unique(want.reshape(-1, 3), axis=0, return_counts=True)
        assert 0.5 < counts.max() / 64 < 1  # most pixels see the background alone, not all
