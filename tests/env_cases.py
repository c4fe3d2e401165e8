"""The radiance kernels' environment instances, one row each: which seeded world of tests/plan_worlds.py
under which route reaches `radiance_kernel<SE, GSTACK, LSCENE, PM, true>` for every reachable
(class, entry width, primitive mode), the ray set that makes its paths bounce before they leave, and
the model's answer (tests/env_model.py). tests/test_env_instances.py checks the table without a GPU;
tests/test_gpu_env_instances.py runs every row. Not a test module.

A row states the (klass, entry_bytes, prim_mode) it expects and `plan_of` asserts it from
GpuScene.launch_plan("radiance") under the row's route before anything runs: the sizes were read off
one build and may drift, the assertion keeps a row on its instance.

The worlds' own camera rays are almost all first-segment misses at these sizes, so `ray_set` aims
1536 seeded rays from the camera's centre at the centres of randomly drawn objects, each target moved
by N(0, 0.15) a coordinate: about half of the paths bounce and then escape.
"""
from collections import namedtuple

import numpy as np

import env_model as em
import plan_worlds as pw
import probe_sets as ps

N_RAYS = 1536
JITTER = 0.15
BG = (0.35, 0.6, 1.25)  # three distinct channels, none of them a world's own
T_MIN = 1e-5

Row = namedtuple("Row", "label family n route plan")  # plan: (klass, entry_bytes, prim_mode)
L, S, G = pw.LDS_SCENE, pw.LDS_STACK, pw.HBM_STACK
ROWS = [
    Row("lds-u16-pm0", "cloud", 300, "default", (L, 2, 0)),
    Row("lds-u16-pm1", "mixed", 278, "default", (L, 2, 1)),
    Row("lds-u16-pm1-flat", "flat", 40, "default", (L, 2, 1)),  # the flat-box filter
    Row("lstack-u16-pm0", "cloud", 300, "hbm", (S, 2, 0)),
    Row("lstack-u16-pm1", "mixed", 300, "default", (S, 2, 1)),
    Row("gstack-u16-pm0", "cloud", 300, "gstack", (G, 2, 0)),
    Row("gstack-u16-pm0-deep", "chain", 78, "default", (G, 2, 0)),  # the depth alone forces the HBM stack
    Row("gstack-u16-pm1", "mixed", 300, "gstack", (G, 2, 1)),
    Row("gstack-u16-pm1-notop", "mixed", 300, "notop", (G, 2, 1)),  # no treelet: another walk entry
    Row("lstack-u32-pm0", "cloud", 2400, "default", (S, 4, 0)),
    Row("lstack-u32-pm1", "mixed", 2950, "default", (S, 4, 1)),
    Row("gstack-u32-pm0", "cloud", 2400, "gstack", (G, 4, 0)),
    Row("gstack-u32-pm0-deep", "chain32", 45, "default", (G, 4, 0)),
    Row("gstack-u32-pm1", "mixed", 2950, "gstack", (G, 4, 1)),
]
BY_LABEL = {r.label: r for r in ROWS}
# every instance a scene can reach: an LDS scene never has u32 entries
REACHABLE = {(L, 2, 0), (L, 2, 1)} | {(k, e, p) for k in (S, G) for e in (2, 4) for p in (0, 1)}
# the bars a row's ray set meets on the model (test_env_instances)
MIN_ESCAPE_SHARE = 0.20

_PATHS = {}


def bvh_of(family):
    """oracle.hits' keywords for the family's tree (GpuScene's max_prims_in_node is its max_prims)."""
    kw = pw.BVH.get(family, {})
    return dict(num_buckets=kw.get("num_buckets", 32), max_prims=kw.get("max_prims_in_node", 12))


def plan_of(scene, row):
    """The scene's radiance plan under the row's route, asserted to be the row's instance."""
    with pw.route(row.route):
        p = pw.plan_dict(scene.launch_plan("radiance"))
    got = (p["klass"], p["entry_bytes"], p["prim_mode"])
    assert got == row.plan, f"{row.label}: {row.family} {row.n} under {row.route} plans {got}, the row says {row.plan}"
    return got


def ray_set(crt, family, n):
    """(rays (N_RAYS, 6), states (N_RAYS,) uint32) of a world: from its camera's centre towards the
    centre of a randomly drawn object, the target moved by N(0, JITTER) a coordinate."""
    d, _ = pw.world(crt, family, n)
    rng = np.random.default_rng(9000 + 7 * (pw.FAMILIES + pw.DEPTH_FAMILIES).index(family) + n)
    objs = d.objects
    pick = rng.integers(0, len(objs), N_RAYS)
    v = np.array(objs["v"][pick], np.float64)
    centre = v[:, :3].copy()
    quad = objs["kind"][pick] == 2
    centre[quad] += 0.5 * (v[quad, 3:6] + v[quad, 6:9])
    box = objs["kind"][pick] == 3
    centre[box] = 0.5 * (v[box, :3] + v[box, 3:6])
    o = np.array(list(d.camera.center), np.float64)
    target = centre + rng.normal(0.0, JITTER, (N_RAYS, 3))
    rays = np.concatenate([np.broadcast_to(o, (N_RAYS, 3)), target - o], 1)
    assert em.traceable(rays).all()
    return np.ascontiguousarray(rays), ps.states(N_RAYS, 9100 + n)


Paths = namedtuple("Paths", "d bvh rays states ended last T flat first_miss twice")


def model_paths(crt, orc, d, rays, states, depth, bvh):
    """The model's paths of rays in a scene at a depth, left unchanged afterwards: how each ended, its
    last direction, its throughput, its value under the constant background BG, whether its first
    segment missed and whether it bounced twice or more. bvh: oracle.hits' keywords, None for the
    defaults."""
    bvh = dict(bvh or {})
    flat, ended, last, T = em.ray_color(orc, d, rays, states, depth, BG, T_MIN, crt=crt, bvh=bvh)
    # a path still going when a depth of 2 runs out has bounced twice
    twice = em.ray_color(orc, d, rays, states, 2, BG, T_MIN, crt=crt, bvh=bvh)[1] == em.DEPTH
    first_miss = orc.hits(d, rays, T_MIN, **bvh)["prim"] < 0
    for a in (rays, states, flat, ended, last, T, first_miss, twice):
        a.setflags(write=False)
    return Paths(d, bvh, rays, states, ended, last, T, flat, first_miss, twice)


def paths(crt, family, n, orc):
    """model_paths of a world's ray set at plan_worlds.DEPTH through the world's own tree, computed
    once a process."""
    k = (family, n)
    if k not in _PATHS:
        d, _ = pw.world(crt, family, n)
        rays, states = ray_set(crt, family, n)
        _PATHS[k] = model_paths(crt, orc, d, rays, states, pw.DEPTH, bvh_of(family))
    return _PATHS[k]


def shares(p):
    """(share of paths that end in a miss after one or more bounces, paths that end on a light, paths
    that end in a miss after two or more bounces) of a Paths."""
    after = (p.ended == em.MISS) & ~p.first_miss
    return float(after.mean()), int((p.ended == em.LIGHT).sum()), int((after & p.twice).sum())


def lit_by(menv, p, bg=BG):
    """The model's output under `menv` from its paths: 0 + T * E(last direction) where a path ended in
    a miss, its constant-background value (which no background enters) elsewhere."""
    want = np.array(p.flat)
    miss = p.ended == em.MISS
    with np.errstate(all="ignore"):
        want[miss] = 0.0 + p.T[miss] * em.lookup(menv, p.last[miss], bg)
    return want


# ---- one axis-aligned mirror: the lookup's edges after a bounce ---------------------------------------
def mirror_world(crt, axis):
    """One Metal parallelogram with fuzz 0, 2000 wide, through the origin with its normal along `axis`
    (0: x, 1: y)."""
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE
    mats = np.zeros(1, MATERIAL_DTYPE)
    mats["kind"], mats["color"], mats["param"] = em.METAL, [[0.5, 0.75, 0.25]], 0.0
    objs = np.zeros(1, OBJECT_DTYPE)
    objs["kind"] = 2
    a, b = [k for k in range(3) if k != axis]
    q, u, v = np.zeros(3), np.zeros(3), np.zeros(3)
    q[a] = q[b] = -1000.0
    u[a] = v[b] = 2000.0
    objs["v"][0] = np.concatenate([q, u, v])
    d = crt.SceneData.named("config1")
    d.materials, d.objects = mats, objs
    return d


def mirror_rays(directions, axis):
    """The finite directions with a component along `axis`, that component made negative, each ray
    started five units back along its direction: it meets the mirror at the origin at t = 5."""
    d = np.array(directions, np.float64)
    d = d[np.isfinite(d).all(1) & (d[:, axis] != 0)]
    d[:, axis] = -np.abs(d[:, axis])
    return np.ascontiguousarray(np.concatenate([-5.0 * d, d], 1))


def ties(dirs):
    """Which directions have two components of exactly equal magnitude, neither zero."""
    a = np.abs(np.asarray(dirs, np.float64))
    out = np.zeros(len(a), bool)
    for i, j in ((0, 1), (1, 2), (0, 2)):
        out |= (a[:, i] == a[:, j]) & (a[:, i] > 0)
    return out


# ---- texels the lookup must not inspect ---------------------------------------------------------------
def odd_map(n=4):
    """A random map with -0.0, negative values, f64 subnormals, +-1e300, +inf and NaN among its texels."""
    rng = np.random.default_rng(77)
    t = rng.random((6 * n, n, 3)) * 4.0
    odd = np.array([-0.0, -1.5, -1e-3, 5e-324, -2.5e-310, 1e300, -1e300, np.inf, np.nan, 0.0])
    flat = t.reshape(-1)
    where = rng.permutation(flat.size)[:flat.size // 2]
    flat[where] = odd[np.arange(len(where)) % len(odd)]
    return t
