"""Ray and radiance queries on the GPU at the decision edges of every node and leaf test:
tests/edge_rays.py's world (59 primitives, four deliberate coincidences) under the default BVH
parameters and as a deep tree, and its families T (sphere tangents), R (sphere roots at t_min),
Q (parallelogram edges and corners), P (rays at the 1e-9 parallel cutoff), C (coincident primitives,
bit-equal hit times), N (node-box planes, edges and corners: NaN slab values, -0.0 components) and
`all` (the six, permuted: NaN-slab rays, tangents and ordinary rays in one wave). The f32 leaf filters
run only in scenes of one kind of primitive, so the world's spheres, its parallelograms and Boxes, and
its axis-aligned ones alone (er.WORLDS) take the same rays: the packed sphere filter, the generic
parallelogram filter and the flat-box filter each see the families made for them, and `all`.
tests/test_edge_rays.py shows, without a GPU, that each family is on both sides of its decision and
that the oracle's records of it are the reference's own (tests/golden/hits_edge_rays.npz).

crt_trace_async's fast route and plain route, crt_closest_hits and every run-time switch must give
the oracle's records, bit for bit, and those are the committed reference records; crt_radiance_async
takes the same rays as first segments and must give the oracle's ray_color bits (the world's colours,
light and background are multiples of 1/8, so at depth 6 every product and sum of ray_color is exact
however it is associated: nothing but the paths themselves can differ). The harness is
tests/test_gpu_trace.py's and tests/test_gpu_radiance.py's: NaN rays past n, 0xFF-prefilled outputs,
a sentinel tail, and every scene's parity guard at 0 after every test."""
import math

import numpy as np
import pytest

import denoise_model as dm
import edge_rays as er
import ray_sets as rs
import test_edge_rays as ter
from oracle import crt_oracle_py as orc
from test_gpu_radiance import PLAIN as RADIANCE_PLAIN
from test_gpu_radiance import bits
from test_gpu_radiance import run as radiance
from test_gpu_trace import ANY, PLAIN, fast_instances, run, same  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
WORLD_KEYS = ter.WORLD_KEYS
PARTS = list(er.WORLDS)
SWITCHES = [
    {"CRT_NO_LDS_SCENE": "1"}, {"CRT_NO_LDS_SCENE": "1", "CRT_NO_PAIR_WALK": "1"},
    {"CRT_NO_LDS_SCENE": "1", "CRT_FORCE_GSTACK": "1"}, {"CRT_F64_NODES": "1"}, {"CRT_EXACT_SLAB": "1"},
    {"CRT_F64_SPHERES": "1"}, {"CRT_F64_QUADS": "1"}, {"CRT_GENERIC_QUADS": "1"},
]
_SCENES = {}


def resident(crt, tree, part="full"):
    """A world of er.WORLDS as the tree of er.TREES on device 0, built under the default switches and kept."""
    if (tree, part) not in _SCENES:
        s = crt.GpuScene(er.world(crt).data[part], **er.TREES[tree])
        s.upload(0)
        _SCENES[tree, part] = s
    return _SCENES[tree, part]


def keys(part):
    return list(er.WORLDS[part]) + ["all"]


@pytest.fixture(autouse=True)
def guard_stays_zero():
    yield
    for which, s in _SCENES.items():
        assert s.guard(0) == 0, which


def check(crt, tree, scene, key, part="full", routes=(0, PLAIN)):
    """One family through `scene`: closest records with the oracle's bits, any-hit flags equal to
    "the oracle found something", on each route. Returns the first route's records."""
    call, want = er.call(crt, key), er.want(crt, tree, key, part)
    first = None
    for route in routes:
        got = run(scene, call, route)
        same(got, want, f"{part} {key} {tree} route {route}")
        assert np.array_equal(run(scene, call, route | ANY), want["prim"] >= 0), f"{part} {key} {tree} any, route {route}"
        first = got if first is None else first
    return first


# ---- ray queries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("part,key", WORLD_KEYS, ids=[f"{p}-{k}" for p, k in WORLD_KEYS])
@pytest.mark.parametrize("tree", list(er.TREES))
def test_both_routes_give_the_references_records(crt, tree, part, key):
    s = resident(crt, tree, part)
    got = check(crt, tree, s, key, part)
    ter.same_as_reference(got, ter.reference_records(crt, tree, key, part), f"{part} {key} {tree} against the reference")
    host = s.closest_hits(er.world(crt).rays[key], er.T_MIN)
    assert host.tobytes() == got.tobytes(), "crt_closest_hits on host arrays"


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("tree", list(er.TREES))
@pytest.mark.parametrize("env", SWITCHES, ids=["+".join(k[4:] for k in e) for e in SWITCHES])
def test_every_switch_gives_the_same_bytes(crt, monkeypatch, env, tree, part):
    """The scene is built and uploaded under the switch (the filter switches are read then). HBM
    kernels with the pair walk, without it and with the global stack; f64 nodes, the exact slab
    test for every ray, the f64 leaf tests in place of the filters (spheres; quads and flat), the
    generic parallelogram filter in place of the flat-box one (flat)."""
    default = {key: run(resident(crt, tree, part), er.call(crt, key)) for key in keys(part)}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = crt.GpuScene(er.world(crt).data[part], **er.TREES[tree])
    s.upload(0)
    for key in keys(part):
        got = check(crt, tree, s, key, part)
        assert got.tobytes() == default[key].tobytes(), key
    s.close()


def edge_oracle(crt, tree, part, rays, t):
    """The oracle's record of every ray i over (t_min, t[i]) through the tree, one oracle run a ray."""
    from cpp_raytracer_amd import HIT_DTYPE
    kw = er.TREES[tree]
    out = np.zeros(len(rays), HIT_DTYPE)
    for i in range(len(rays)):
        out[i] = orc.hits(er.world(crt).data[part], rays[i:i + 1], er.T_MIN, float(t[i]), kw.get("num_buckets", 32),
                          kw.get("max_prims_in_node", 12))[0]
    return out


@pytest.mark.parametrize("part,least", [("full", 128), ("spheres", 32), ("quads", 96), ("flat", 96)])
@pytest.mark.parametrize("tree", list(er.TREES))
def test_upper_bounds_at_a_tied_hit_time(crt, tree, part, least):
    """Family C's rays whose closest hit is the tie, with per-ray upper bounds: t_max = the tied time
    excludes both primitives (a miss, or whatever lies behind), t_max = nextafter(t, inf) returns the
    winner of the unbounded query. The oracle is shown to change its answer across the edge first."""
    w = er.world(crt)
    c, full = er.targeted(crt)["C"], er.want(crt, tree, "C", part)
    idx = np.flatnonzero(c["tie"] & (full["prim"] >= 0) & (dm.bits(full["t"]) == dm.bits(c["t"])))
    assert len(idx) >= least
    rays, hit = w.rays["C"][idx], full[idx]
    at = rs.Call(rays, t_min=er.T_MIN, tmax=hit["t"].copy())
    above = rs.Call(rays, t_min=er.T_MIN, tmax=np.nextafter(hit["t"], math.inf))
    o_at, o_above = edge_oracle(crt, tree, part, rays, at.tmax), edge_oracle(crt, tree, part, rays, above.tmax)
    assert not ((o_at["prim"] >= 0) & (dm.bits(o_at["t"]) == dm.bits(hit["t"]))).any()
    same(o_above, hit, "oracle above the edge")
    s = resident(crt, tree, part)
    for route in (0, PLAIN):
        same(run(s, at, route), o_at, f"{tree} t_max = t, route {route}")
        same(run(s, above, route), hit, f"{tree} t_max = nextafter(t), route {route}")
        assert np.array_equal(run(s, at, route | ANY), o_at["prim"] >= 0)
        assert run(s, above, route | ANY).all()


def test_one_block_takes_the_mixed_wave(crt, monkeypatch):
    """`all` on a grid of one block: every wave refills with rays of every family."""
    monkeypatch.setenv("CRT_GRID_BLOCKS", "1")
    for part in PARTS:
        for tree in er.TREES:
            check(crt, tree, resident(crt, tree, part), "all", part, routes=(0,))


# ---- radiance queries -------------------------------------------------------------------------------
@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("tree", list(er.TREES))
@pytest.mark.parametrize("env", [{}, {"CRT_NO_LDS_SCENE": "1"}], ids=["default", "NO_LDS_SCENE"])
def test_radiance_of_edge_rays_as_first_segments(crt, monkeypatch, env, tree, part):
    """States crt_sample_seed(base, i, 0) (the call passes none), depth 6, a background that no
    material has: both routes give the oracle's bits. A grazing first hit sends the scattered ray
    off a point on a node plane, which is how renders reach these cases."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = crt.GpuScene(er.world(crt).data[part], **er.TREES[tree]) if env else resident(crt, tree, part)
    s.upload(0)
    for key in keys(part):
        want = er.want_radiance(crt, tree, key, part)
        rays = er.world(crt).rays[key]
        fast = radiance(s, rays, None, er.RADIANCE_DEPTH, er.BG, er.T_MIN, 0, base_seed=er.RADIANCE_BASE)
        plain = radiance(s, rays, None, er.RADIANCE_DEPTH, er.BG, er.T_MIN, RADIANCE_PLAIN, base_seed=er.RADIANCE_BASE)
        diff = (bits(fast) != bits(want)).any(1)
        print(f"{part} {key} {tree}: {int(diff.sum())} of {len(rays)} paths differ from the oracle, max |gpu - oracle| = "
              f"{float(np.abs(fast - want).max()):.3g}")
        assert not diff.any(), (part, key, tree, np.flatnonzero(diff)[:8])
        assert np.array_equal(bits(plain), bits(fast)), (part, key, tree)
        explicit = radiance(s, rays, er.states(er.RADIANCE_BASE, len(rays)), er.RADIANCE_DEPTH, er.BG, er.T_MIN, 0)
        assert np.array_equal(bits(explicit), bits(fast)), (part, key, tree)
        assert len(np.unique(bits(want), axis=0)) > 4  # paths of several kinds
    if env:
        assert s.guard(0) == 0
        s.close()
