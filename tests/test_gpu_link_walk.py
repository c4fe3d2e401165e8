"""The stackless walk of the five-wave LDS-scene render instances (crt_device.hip walk(), LINK; DESIGN
§4) against the stack walk in the same build: CRT_NO_LINK_WALK=1, read at each launch, keeps a launch
on the stack instance, and crt_last_walk says which one a launch took. The two walks visit the same
nodes in the same order (tests/test_link_walk_model.py), so frames must be bit-identical and the
instrumented pass's counters exactly equal; one scene also goes against the oracle at
tests/test_gpu_parity.py's tolerance. Scenes: the five-wave sphere instance (rtow_final), the flat
parallelogram instance (cornell), a root that is a leaf, one interior node, the EXACT walk forced for
every ray (CRT_EXACT_SLAB=1), and both sides of the capacity edge 16 * nodes <= guard levels + stack
inside the five-wave class (balanced_row: 191 | 192 spheres), the far side observed on the stack
instance."""
import numpy as np
import pytest

import plan_worlds as pw
from oracle import crt_oracle_py as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_parity.py
COUNTERS = ("rays", "nodes_visited", "sphere_tests", "parallelogram_tests", "slow_node_tests", "candidate_tests")


def named(crt, name, seed, **cam):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named(name, seed)
    d.camera = camera_with(d.camera, **cam)
    return d, {}


def cloud(crt, n, **kw):
    from cpp_raytracer_amd import camera_with
    d, _ = pw.world(crt, "cloud", n)
    d.camera = camera_with(d.camera, image_w=16, image_h=8, samples_per_pixel=2)
    return d, kw


CASES = {
    "rtow_final": lambda crt: named(crt, "rtow_final", 42, image_w=64, image_h=32, samples_per_pixel=8, max_depth=50),
    "cornell": lambda crt: named(crt, "cornell", None, image_w=32, image_h=32, samples_per_pixel=8),
    "one_sphere": lambda crt: cloud(crt, 1),
    "two_spheres": lambda crt: cloud(crt, 2, max_prims_in_node=1),
}


def both_walks(crt, monkeypatch, d, kw, base_seed, want_default="links"):
    """(frame, counters) of the default launch and of the stack walk, with the walk each one took checked."""
    out = {}
    s = crt.GpuScene(d, **kw)
    try:
        cam = crt.resolve_camera(d.camera, base_seed)
        assert s.last_walk(0) == "none"
        for forced in (False, True):  # the launch's own choice first, then the stack walk by the switch
            if forced:
                monkeypatch.setenv("CRT_NO_LINK_WALK", "1")
            walk = "stack" if forced else want_default
            frame, _ = s.render(cam, 1)
            assert s.last_walk(0) == walk
            st = s.render_count(0, cam)
            assert s.last_walk(0) == walk
            out[forced] = (frame, {k: int(getattr(st, k)) for k in COUNTERS})
        monkeypatch.delenv("CRT_NO_LINK_WALK")
        assert s.guard(0) == 0
    finally:
        s.close()
    return out[False], out[True]


def assert_same(a, b):
    assert np.isfinite(a[0]).all()
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert a[1] == b[1]
    assert a[1]["rays"] > 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_walks_agree(crt, monkeypatch, case):
    d, kw = CASES[case](crt)
    s = crt.GpuScene(d, **kw)
    p = s.launch_plan("render")
    s.close()
    assert p.five_waves == 1 and p.prim_mode == (2 if case == "cornell" else 0)
    links, stack = both_walks(crt, monkeypatch, d, kw, 11)
    assert_same(links, stack)
    if case == "two_spheres":
        assert links[1]["nodes_visited"] > links[1]["rays"]  # the root is interior


@pytest.mark.parametrize("case", ["rtow_final", "cornell"])
def test_walks_agree_with_the_exact_walk_forced(crt, monkeypatch, case):
    d, kw = CASES[case](crt)
    monkeypatch.setenv("CRT_EXACT_SLAB", "1")
    exact = both_walks(crt, monkeypatch, d, kw, 12)
    assert_same(*exact)
    monkeypatch.delenv("CRT_EXACT_SLAB")
    fast, _ = both_walks(crt, monkeypatch, d, kw, 12)
    assert np.array_equal(exact[0][0].view(np.uint64), fast[0].view(np.uint64))
    # the f32 walk decides almost every node itself; the EXACT walk has no f32 test to fall back from
    assert exact[0][1]["slow_node_tests"] == 0 and exact[0][1]["nodes_visited"] == fast[1]["nodes_visited"]


def test_link_walk_matches_the_oracle(crt, monkeypatch):
    d, kw = CASES["rtow_final"](crt)
    links, _ = both_walks(crt, monkeypatch, d, kw, 13)
    want = orc.render(d, 13, threads=16)
    err = np.abs(links[0] - want)
    assert err.max() <= TOL
    assert err.max() <= 1e-12 * max(1.0, np.abs(want).max())


def region(p):
    return 2 * p.level + p.stack_bytes


def balanced_row(crt, n):
    """A sphere-only world made to reach the table's capacity inside the five-wave class: the first n of
    192 spheres of radius 0.3 on the x axis at hierarchically spaced places (x = sum of b_k 3^k over
    the 8 bits of i, without the i whose low two bits are both set, scaled to [-8, 8]), one sphere a leaf.
    The gaps grow threefold a level, so the SAH build splits where the bits do: 192 leaves in 10 levels
    (BVH depth 9), the shallowest tree a five-wave block's 32 KB can hold so many nodes of. A node
    costs the table 16 bytes and the stack region grows by 512 a level, so only a tree this shallow
    outgrows the region before the scene leaves the five-wave class; tests/plan_worlds.py's own
    families (SAH on random clouds, depth 11 and more at these sizes) leave the class first, so the
    world is built here, on plan_worlds' materials and camera."""
    from cpp_raytracer_amd import camera_with
    x = np.array([sum(((i >> k) & 1) * 3 ** k for k in range(8)) for i in range(256) if (i & 3) != 3], float)
    assert 1 <= n <= len(x)
    d, _ = pw.world(crt, "cloud", n)
    objs = d.objects.copy()
    objs["v"][:, :3] = 0
    objs["v"][:, 0] = (x[:n] - x.max() / 2) * (16.0 / x.max())
    objs["v"][:, 3] = 0.3
    d.objects = objs
    # a 32 x 4 frame 17.6 x 2.2 units at the row's distance (44): the row fills about one pixel row of four
    d.camera = camera_with(d.camera, image_w=32, image_h=4, samples_per_pixel=2, fov=float(2 * np.arctan(1.1 / 44)))
    return d, dict(max_prims_in_node=1)


@pytest.fixture(scope="module")
def capacity_edge(crt):
    """(n - 1, n): the largest balanced_row whose table fits the bytes the plan keeps for the guard
    levels and the stack, and the smallest whose table does not, both five-wave sphere-only LDS
    scenes; found from the plans alone (191 | 192 spheres, 383 | 385 nodes, 6128 | 6160 of 6144 bytes)."""
    prev = None
    for n in range(2, 193):
        d, kw = balanced_row(crt, n)
        s = crt.GpuScene(d, **kw)
        p = s.launch_plan("render")
        s.close()
        assert p.klass == pw.LDS_SCENE and p.five_waves == 1 and p.prim_mode == 0 and p.entry_bytes == 2, n
        if 16 * p.num_nodes > region(p):
            assert prev == n - 1
            return n - 1, n
        prev = n
    raise LookupError("no balanced_row outgrows the stack region inside the five-wave class")


@pytest.mark.parametrize("side", ["fits", "beyond"])
def test_capacity_edge(crt, monkeypatch, capacity_edge, side):
    """Both sides equal the stack walk and the oracle; the far side is observed to have taken the
    stack instance by its own choice (no switch set), with its table in hand."""
    n = capacity_edge[0 if side == "fits" else 1]
    d, kw = balanced_row(crt, n)
    s = crt.GpuScene(d, **kw)
    p = s.launch_plan("render")
    assert s.walk_links() is not None and len(s.walk_links()) == p.num_nodes  # the table exists on both sides
    s.close()
    assert (16 * p.num_nodes <= region(p)) == (side == "fits")
    own, stack = both_walks(crt, monkeypatch, d, kw, 14, "links" if side == "fits" else "stack")
    assert_same(own, stack)
    assert own[1]["nodes_visited"] > own[1]["rays"]  # some rays descend below the root
    want = orc.render(d, 14, threads=16)
    err = np.abs(own[0] - want)
    assert err.max() <= TOL and err.max() <= 1e-12 * max(1.0, np.abs(want).max())
