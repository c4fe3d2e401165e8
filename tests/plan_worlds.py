"""Seeded worlds with a size parameter for the launch-plan tests: the host picks a kernel instance from
the scene's size alone (crt_device.hip scene_layout, u16_entries), and these worlds
walk each family across every one of those decisions one object at a time. tests/test_launch_plan.py
checks the plans on the way, without a GPU; tests/test_gpu_plan_edges.py runs both sides of every
edge found. Not a test module.

world(crt, family, n) is the first n objects of one fixed seeded sequence (so n and n + 1 differ by one
object), materials i % 5 of guard_cases.unit_world's five kinds, in a [-8, 8]^3 cluster that a camera
at (0, 0, 44) sees whole; every record is far inside the f32 ranges (crt_internal.h kF32BoundMax,
kF32SphereMax). Families:

  cloud    spheres only (every 9th hollow)
  flat     axis-aligned parallelograms, every 4th object a Box
  rotated  general parallelograms
  mixed    spheres, general and axis-aligned parallelograms in turn

Depth families, built with BVH(world, 2 buckets, 1 primitive a leaf) so that the depth follows the
centroids: `chain` is sphere i at (2^(i - 48), 0, 0) with radius 1 - i / 128, bvh_pathological's
geometric positions with a ratio the f32 range survives (2^26 at 75 spheres; its radii do not grow,
so the boxes of all levels share the core at the origin and a ray towards it descends every level).
With two buckets the split peels one octave of centroids a level: depth ~ n, and depth + 1 passes 64
(the u16 edge of the LDS stack budget) near n = 75. `chain32` puts a fixed cloud of CLOUD32 small
spheres (more than 2048 nodes: u32 entries) beside the first n chain spheres; its stack leaves LDS
where it no longer fits an HBM scene's block beside the treelet's levels (depth + 1 = 29 | 30 for render
and radiance, 30 | 31 for trace, near n = 27; 32 | 33, the 32 KB themselves, lies behind that), also inside
the f32 range. Their camera looks at the core and the chain's
spheres up to x = 16; the ones further out are beyond the frame.
"""
import contextlib
import os

import numpy as np

FAMILIES = ("cloud", "flat", "rotated", "mixed")
DEPTH_FAMILIES = ("chain", "chain32")
KERNELS = ("render", "trace", "radiance")
W, H, SPP, DEPTH = 24, 16, 4, 8
FOV = float(np.deg2rad(40.0))
BACKGROUND = (0.55, 0.7, 0.95)
BASE_SEED = 7300
CLOUD32 = 1100
# scan ranges: edge() looks at every n of [1, N_MAX[family]]; an edge not found inside is an error
N_MAX = {"cloud": 2400, "flat": 1150, "rotated": 3100, "mixed": 2950, "chain": 78, "chain32": 45}
BVH = {f: dict(max_prims_in_node=4) for f in FAMILIES}
BVH.update(chain=dict(num_buckets=2, max_prims_in_node=1), chain32=dict(num_buckets=2, max_prims_in_node=1))

# routes: the switches set on top of one another, and the treelet off beside an LDS stack
ROUTES = {
    "default": (),
    "hbm": ("CRT_NO_LDS_SCENE",),
    "gstack": ("CRT_NO_LDS_SCENE", "CRT_FORCE_GSTACK"),
    "notop": ("CRT_NO_LDS_SCENE", "CRT_FORCE_GSTACK", "CRT_NO_LDS_TOP"),
    "hbm_notop": ("CRT_NO_LDS_SCENE", "CRT_NO_LDS_TOP"),
}
_SWITCHES = ("CRT_NO_LDS_SCENE", "CRT_FORCE_GSTACK", "CRT_NO_LDS_TOP", "CRT_FOUR_WAVES", "CRT_F64_NODES",
             "CRT_F64_SPHERES", "CRT_F64_QUADS", "CRT_GENERIC_QUADS", "CRT_EXACT_SLAB")
LDS_SCENE, LDS_STACK, HBM_STACK = 0, 1, 2
ABSENT = 0xFFFFFFFF


@contextlib.contextmanager
def route(name):
    """The process environment with exactly the route's switches set (and CRT_TRACE_FAST, so a trace
    plan is the fast instance's)."""
    keep = {k: os.environ.get(k) for k in _SWITCHES + ("CRT_TRACE_FAST",)}
    for k in _SWITCHES:
        os.environ.pop(k, None)
    for k in ROUTES[name] + ("CRT_TRACE_FAST",):
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def materials():
    from cpp_raytracer_amd import MATERIAL_DTYPE
    mats = np.zeros(5, MATERIAL_DTYPE)
    mats["kind"] = [1, 2, 2, 3, 4]  # Lambertian, mirror Metal, fuzzed Metal, Dielectric, light
    mats["color"] = [[0.8, 0.3, 0.2], [0.9, 0.9, 0.7], [0.6, 0.7, 0.9], [0.0, 0.0, 0.0], [1.0, 0.9, 0.8]]
    mats["param"] = [0.0, 0.0, 0.4, 1.5, 3.0]
    return mats


_SEQ = {}


def sequence(family):
    """The family's whole object sequence (N_MAX of them), generated once."""
    if family in _SEQ:
        return _SEQ[family]
    from cpp_raytracer_amd import OBJECT_DTYPE
    n = N_MAX[family]
    objs = np.zeros(n, OBJECT_DTYPE)
    objs["material"] = np.arange(n) % 5
    i = np.arange(n)
    if family in DEPTH_FAMILIES:
        objs["kind"] = 1
        objs["material"] = (i + 3) % 5  # the outermost of the core is glass
        objs["v"][:, 0] = 2.0 ** (i - 48)
        objs["v"][:, 3] = 1.0 - i / 128.0
        assert objs["v"][:, 3].min() > 0.25 and objs["v"][:, 0].max() <= 2.0 ** 29
    else:
        rng = np.random.default_rng(40 + FAMILIES.index(family))
        # per object one row of draws, whatever its kind: the sequence does not depend on n
        u = rng.random((n, 12))
        pos = u[:, :3] * 16 - 8
        sphere = {"cloud": np.ones(n, bool), "mixed": i % 3 == 0}.get(family, np.zeros(n, bool))
        general = {"rotated": np.ones(n, bool), "mixed": i % 3 == 1}.get(family, np.zeros(n, bool))
        box = (i % 4 == 3) if family == "flat" else np.zeros(n, bool)
        aligned = ~sphere & ~general & ~box
        objs["kind"] = np.where(sphere, 1, np.where(box, 3, 2))
        v = objs["v"]
        v[:, :3] = pos
        v[sphere, 3] = (0.15 + 0.3 * u[sphere, 3]) * np.where(i[sphere] % 9 == 8, -1, 1)
        v[general, 3:9] = u[general, 3:9] * 2.4 - 1.2
        for k in np.flatnonzero(aligned):
            ax = np.argsort(u[k, 9:12])
            v[k, 3 + ax[0]] = (0.5 + 1.5 * u[k, 3]) * (1 if u[k, 5] < 0.5 else -1)
            v[k, 6 + ax[1]] = (0.5 + 1.5 * u[k, 4]) * (1 if u[k, 6] < 0.5 else -1)
        v[box, 3:6] = pos[box] + 0.4 + 0.8 * u[box, 3:6]
    _SEQ[family] = objs
    return objs


def cloud32():
    """chain32's fixed cloud: CLOUD32 small spheres right of the core."""
    from cpp_raytracer_amd import OBJECT_DTYPE
    rng = np.random.default_rng(46)
    objs = np.zeros(CLOUD32, OBJECT_DTYPE)
    objs["kind"] = 1
    objs["material"] = np.arange(CLOUD32) % 5
    objs["v"][:, :3] = rng.uniform([6, -4, -4], [14, 4, 4], (CLOUD32, 3))
    objs["v"][:, 3] = rng.uniform(0.1, 0.2, CLOUD32)
    return objs


def world(crt, family, n):
    """(SceneData, GpuScene keywords) of the family's first n objects."""
    from cpp_raytracer_amd import camera_with
    from cpp_raytracer_amd._capi import D3
    assert 1 <= n <= N_MAX[family], (family, n)
    objs = sequence(family)[:n].copy()
    if family == "chain32":
        objs = np.concatenate([cloud32(), objs])
    d = crt.SceneData.named("config1")
    d.materials, d.objects = materials(), objs
    centre, look = ((5.0, 3.0, 34.0), (5.0, 0.0, 0.0)) if family in DEPTH_FAMILIES else ((0.0, 0.0, 44.0), (0.0, 0.0, 0.0))
    d.camera = camera_with(d.camera, image_w=W, image_h=H, samples_per_pixel=SPP, max_depth=DEPTH, center=D3(*centre),
                           lookat=D3(*look), has_lookat=1, up=D3(0.0, 1.0, 0.0), fov=FOV, fov_is_vertical=1,
                           defocus_angle=0.0, focus_dist=1.0, has_focus_dist=1, background=D3(*BACKGROUND))
    return d, dict(BVH.get(family, {}))


def gpu_scene(crt, family, n):
    d, kw = world(crt, family, n)
    return d, crt.GpuScene(d, **kw)


def plan_dict(p):
    return {name: getattr(p, name) for name, _ in p._fields_ if name != "reserved"}


def plans(scene, routes=ROUTES, kernels=KERNELS):
    """{(kernel, route): plan dict} of a GpuScene."""
    out = {}
    for r in routes:
        with route(r):
            for k in kernels:
                out[k, r] = plan_dict(scene.launch_plan(k))
    return out


# ---- the edges -------------------------------------------------------------------------------------
def treelet(p):
    """An HBM-scene plan's treelet: the whole node array, a cut of it, or none."""
    if p["klass"] == LDS_SCENE:
        return "n/a"
    return "whole" if p["ntop"] == p["all_nodes"] else "cut"


# edge -> (what it reads off a plan, the value below, the value above)
EDGES = {
    "E1": (lambda p: p["entry_bytes"], 2, 4),
    "E2": (lambda p: p["klass"] == LDS_SCENE, True, False),
    "E3": (lambda p: (p["klass"] == LDS_SCENE, p["five_waves"]), (True, 1), (True, 0)),
    "E4": (lambda p: (p["klass"] == LDS_SCENE, p["bytes_sph64"] > 0), (True, True), (True, False)),
    "E5": (treelet, "whole", "cut"),
    "E6": (lambda p: p["klass"] == HBM_STACK, False, True),
}


def applies(edge, kernel, family):
    if family in DEPTH_FAMILIES:
        return edge == "E6"
    if edge == "E3":
        return kernel == "render" and family in ("cloud", "flat")
    if edge == "E4":
        return kernel == "render" and family == "cloud"
    return edge in ("E1", "E2", "E5")


def rows():
    """Every (edge, kernel, family) that must be found."""
    return [(e, k, f) for e in EDGES for f in FAMILIES + DEPTH_FAMILIES for k in KERNELS if applies(e, k, f)]


_TABLE = {}


def scan(crt, family, visit=None, routes=("default",)):
    """Every n of the family's scan range in turn: visit(n, info, plans) if given, and the family's
    edges {(edge, kernel): (n_below, n_above, nodes below, nodes above, depth below, depth above)}, the
    first place each is crossed on the default route. A missing edge raises."""
    found, prev = {}, None
    want = [(e, k) for e, k, f in rows() if f == family]
    for n in range(1, N_MAX[family] + 1):
        _, s = gpu_scene(crt, family, n)
        pl = plans(s, routes)
        info = s.info()
        s.close()
        if visit:
            visit(n, info, pl)
        if prev is not None:
            for e, k in want:
                read, below, above = EDGES[e]
                a, b = prev[1][k, "default"], pl[k, "default"]
                if (e, k) not in found and read(a) == below and read(b) == above:
                    found[e, k] = (n - 1, n, a["num_nodes"], b["num_nodes"], a["depth"], b["depth"])
        prev = (n, pl)
    missing = [x for x in want if x not in found]
    if missing:
        raise LookupError(f"{family}: edges {missing} not found for n in [1, {N_MAX[family]}]")
    return found


def table(crt, family):
    """scan()'s edges of a family, computed once a process."""
    if family not in _TABLE:
        _TABLE[family] = scan(crt, family)
    return _TABLE[family]


def edge(crt, family, kernel, field):
    """(n - 1, n): the first neighbouring sizes between which the plan's `field` (E1..E6) changes."""
    return table(crt, family)[field, kernel][:2]


def format_table(tables):
    lines = ["edge kernel   family   n_below n_above nodes_below nodes_above depth_below depth_above"]
    for e, k, f in rows():
        r = tables[f][e, k]
        lines.append(f"{e:4} {k:8} {f:8} {r[0]:7} {r[1]:7} {r[2]:11} {r[3]:11} {r[4]:11} {r[5]:11}")
    return "\n".join(lines)
