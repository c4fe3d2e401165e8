"""Seeded ray sets for the ray-query tests (crt_trace_async): what tests/test_gpu_trace.py sends
through both routes of the GPU entry and what tests/test_ray_sets.py checks, without a GPU, to be
worth sending (the oracle reports both hits and misses in every set). Not a test module.

A query is a Call: rays (n, 6), the call's t_min and t_max, and per-ray upper bounds (or None).
The oracle (oracle/crt_oracle_py.py hits) takes one interval a call, so oracle() runs it once per
distinct upper bound.

  A  centre rays of a 96 x 64 camera of the scene (denoise_model.centre_rays)
  B  the reflected secondaries of A's hits: origin = hit point, d - 2 (d . n) n
  C  shadow rays from A's hit points to seeded points of the hit points' bounding box, per-ray
     upper bounds: 1 (the target), and 0.5, 2 and +inf for every 4th, 7th and 11th ray
  D  tests/test_gpu_vs_oracle.py's many-rays generator at 20,000 rays: origins over and beyond the
     scene box, normal directions, 5 % with a zero component
  E  the first 4096 rays of D with directions times 2^k and t_min times 2^-k, k of
     guard_cases.HIT_SCALES (the fast paths' range fallbacks): one Call per k
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import denoise_model as dm
import guard_cases as gc
from oracle import crt_oracle_py as orc

W, H = 96, 64
SEED = 11
INF = float("inf")


@dataclass
class Call:
    rays: np.ndarray
    t_min: float = 1e-5
    t_max: float = INF
    tmax: Optional[np.ndarray] = None

    def bounds(self):
        return self.tmax if self.tmax is not None else np.full(len(self.rays), self.t_max)


def oracle(d, call):
    """The oracle's records of a Call, one oracle run per distinct upper bound."""
    from cpp_raytracer_amd import HIT_DTYPE
    if call.tmax is None:
        return orc.hits(d, call.rays, call.t_min, call.t_max)
    out = np.zeros(len(call.rays), HIT_DTYPE)
    for v in np.unique(call.tmax):
        sel = call.tmax == v
        out[sel] = orc.hits(d, call.rays[sel], call.t_min, float(v))
    return out


def camera(crt, d):
    from cpp_raytracer_amd import camera_with
    return crt.resolve_camera(camera_with(d.camera, image_w=W, image_h=H), 0)


def set_a(crt, d):
    return Call(dm.centre_rays(camera(crt, d)).reshape(-1, 6))


def set_b(a, hits_a):
    hit = hits_a["prim"] >= 0
    dd, n = a.rays[hit, 3:], hits_a["normal"][hit]
    dn = (dd[:, 0] * n[:, 0] + dd[:, 1] * n[:, 1]) + dd[:, 2] * n[:, 2]
    return Call(np.concatenate([hits_a["point"][hit], dd - 2 * dn[:, None] * n], 1))


def set_c(hits_a):
    p = hits_a["point"][hits_a["prim"] >= 0]
    rng = np.random.default_rng(SEED)
    target = p.min(0) + rng.random(p.shape) * (p.max(0) - p.min(0))
    tmax = np.ones(len(p))
    i = np.arange(len(p))
    tmax[i % 4 == 3] = 0.5
    tmax[i % 7 == 6] = 2.0
    tmax[i % 11 == 10] = INF
    return Call(np.concatenate([p, target - p], 1), tmax=tmax)


def root_box(crt, d, **kw):
    nodes, _ = crt.GpuScene(d, **kw).export_bvh()
    b = nodes[0]["bounds"]
    if not np.all(np.isfinite(b)):  # a linear scene's one leaf is unbounded: the objects' reach
        v = np.abs(np.asarray(d.objects["v"], np.float64)).max()
        return np.full(3, -v), np.full(3, v)
    return np.array([b[0], b[2], b[4]]), np.array([b[1], b[3], b[5]])


def set_d(crt, d, n=20_000, **kw):
    lo, hi = root_box(crt, d, **kw)
    rng = np.random.default_rng(7)
    lo, hi = np.maximum(lo, -1e3), np.minimum(hi, 1e3)
    span = hi - lo
    o = lo - 0.25 * span + rng.random((n, 3)) * 1.5 * span
    dirs = rng.normal(size=(n, 3))
    dirs[: n // 20, rng.integers(0, 3)] = 0.0
    return Call(np.concatenate([o, dirs], axis=1))


def set_e(dcall):
    out = []
    for k in gc.HIT_SCALES:
        r = dcall.rays[:4096].copy()
        r[:, 3:] *= 2.0 ** k
        out.append(Call(r, t_min=1e-5 * 2.0 ** -k))
    return out


def all_sets(crt, d, **kw):
    """{"A": [Call], ..., "E": [Call, ...]} and the oracle's records of every call, in step."""
    a = set_a(crt, d)
    ha = oracle(d, a)
    dd = set_d(crt, d, **kw)
    sets = {"A": [a], "B": [set_b(a, ha)], "C": [set_c(ha)], "D": [dd], "E": set_e(dd)}
    want = {k: [ha] if k == "A" else [oracle(d, c) for c in v] for k, v in sets.items()}
    return sets, want


def hit_share(wants):
    prim = np.concatenate([w["prim"] for w in wants])
    return float((prim >= 0).mean())


# ---- rays outside the contract: (name, six numbers, per-ray upper bound) ---------------------------
NAN = float("nan")
_OK = [0.5, 0.25, 3.0, 0.1, -0.2, -1.0]


def invalid_rays():
    out = []
    for k in range(6):
        r = list(_OK)
        r[k] = NAN
        out.append((f"nan[{k}]", r, INF))
    for k in (0, 2, 3, 5):
        for v in (INF, -INF):
            r = list(_OK)
            r[k] = v
            out.append((f"{'+' if v > 0 else '-'}inf[{k}]", r, INF))
    out.append(("zero-dir", _OK[:3] + [0.0, 0.0, 0.0], INF))
    out.append(("negzero-dir", _OK[:3] + [-0.0, 0.0, -0.0], INF))
    out.append(("nan-tmax", list(_OK), NAN))
    return out


# ---- the scenes of the GPU tests -------------------------------------------------------------------
def big_world(crt, n=20_000, quads=0):
    """A seeded world of n small spheres (and `quads` parallelograms) in a [-100, 100]^3 cube: more
    than 65536 bytes of f32 nodes, so the stacks hold u32 entries and the scene stays in HBM."""
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE, camera_with
    from cpp_raytracer_amd._capi import D3
    rng = np.random.default_rng(2024)
    mats = np.zeros(4, MATERIAL_DTYPE)
    mats["kind"] = [1, 2, 3, 1]
    mats["color"] = [[0.7, 0.3, 0.3], [0.8, 0.8, 0.8], [0, 0, 0], [0.2, 0.6, 0.3]]
    mats["param"] = [0, 0.1, 1.5, 0]
    objs = np.zeros(n + quads, OBJECT_DTYPE)
    objs["kind"][:n] = 1
    objs["material"] = rng.integers(0, 4, n + quads)
    objs["v"][:n, :3] = rng.uniform(-100, 100, (n, 3))
    objs["v"][:n, 3] = rng.uniform(0.3, 1.6, n)
    if quads:
        objs["kind"][n:] = 2
        objs["v"][n:, :3] = rng.uniform(-100, 96, (quads, 3))
        objs["v"][n:, 3:9] = rng.uniform(-4, 4, (quads, 6))
    d = crt.SceneData.named("config1")
    d.materials, d.objects = mats, objs
    d.camera = camera_with(d.camera, center=D3(0.0, 0.0, 230.0), lookat=D3(0.0, 0.0, 0.0), has_lookat=1,
                           up=D3(0.0, 1.0, 0.0), fov=float(np.deg2rad(50.0)), fov_is_vertical=1, defocus_angle=0.0)
    return d


def scene_data(crt, name):
    if name == "rtow_final":
        return crt.SceneData.named("rtow_final", 42)
    if name in ("cornell", "christmas_tree", "bvh_pathological"):
        return crt.SceneData.named(name)
    if name in ("rotated", "mixed", "flat", "spheres"):
        return gc.scene(crt, name)
    if name == "big":
        return big_world(crt)
    if name == "big_mixed":
        return big_world(crt, 12_000, 600)
    raise KeyError(name)


# scene -> the sets its GPU tests use (tests/test_ray_sets.py holds each pair to 5 % of hits and of
# misses). Every ray of sets A, B, D and E hits bvh_pathological's enclosing sphere, so that scene
# takes the shadow rays only. The linear scenes (one always-entered leaf) are the seeded worlds of
# guard_cases: 25 of cornell's centre rays hit an edge shared by two parallelograms, and which of the
# two a tie reports depends on the order of the tests, which a linear scene and the oracle's tree do
# not share.
SCENE_SETS = {"rtow_final": "ABCDE", "cornell": "ABCDE", "rotated": "ABCDE", "mixed": "ABCDE",
              "christmas_tree": "ABCDE", "big": "ABCDE", "big_mixed": "AD", "bvh_pathological": "C",
              "rotated_linear": "ABCDE", "mixed_linear": "ABCDE"}
_WORLDS = {}


def world(crt, name):
    """(SceneData, GpuScene keywords, sets, the oracle's records) of a test scene, computed once."""
    if name not in _WORLDS:
        kw = {"linear": True} if name.endswith("_linear") else {}
        d = scene_data(crt, name.removesuffix("_linear"))
        sets, want = all_sets(crt, d, **kw)
        keep = SCENE_SETS[name]
        _WORLDS[name] = (d, kw, {k: v for k, v in sets.items() if k in keep}, {k: v for k, v in want.items() if k in keep})
    return _WORLDS[name]
