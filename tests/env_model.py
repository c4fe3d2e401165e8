"""A numpy and Python-float restatement of cube-map environment lighting (include/crt_render.h,
crt_env): what the device must write, computed without a GPU. Not a test module.

  lookup     E(d) of the header, step by step, over arrays of directions.
  ray_color  a path model of crt_radiance_async with or without an environment: one bounce at a time
             over all live paths. The closest hits come from the oracle (oracle.hits: the point, the
             normal facing the ray and front_face), the four materials are shade()'s own operations in
             shade()'s order on Python floats (the forward throughput T, the draws through the
             package's rand_double, IEEE sqrt and division, nothing fused).

Python floats and numpy float64 arrays are IEEE doubles, so the lookup's values are the kernel's bits;
the paths are the reference's wherever the oracle's ray_color is (tests/test_env_model.py holds the
model to it). pow5 (csrc/crt_schlick.h) is x^5 rounded once; here it is the exact rational rounded.
"""
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

NEAREST, BILINEAR = 0, 1
MISS, LIGHT, ABSORBED, DEPTH = range(4)  # how a path ended
LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT = 1, 2, 3, 4  # crt_material kinds (asserted in the tests)


@dataclass
class Env:
    texels: np.ndarray  # (6n, n, 3) float64
    filter: int
    right: tuple
    up: tuple
    forward: tuple

    @property
    def n(self):
        return self.texels.shape[1]


def basis(forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)):
    """make_lens's and make_env's basis (right, up, forward), the same numpy lines."""
    f = np.asarray(forward, np.float64).reshape(3)
    u = np.asarray(up, np.float64).reshape(3)
    f = f / np.sqrt(f.dot(f))
    r = np.cross(f, u)
    r = r / np.sqrt(r.dot(r))
    u = np.cross(r, f)
    return tuple(r.tolist()), tuple(u.tolist()), tuple(f.tolist())


def make(texels, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), filter=BILINEAR):
    t = np.ascontiguousarray(texels, np.float64)
    assert t.ndim == 3 and t.shape[2] == 3 and t.shape[0] == 6 * t.shape[1] and t.shape[1] >= 1
    r, u, f = basis(forward, up)
    return Env(t, filter, r, u, f)


def lookup(env, dirs, background=(0.0, 0.0, 0.0)):
    """E(d) for dirs (m, 3): (m, 3) float64. `background` is the call's constant, the value where d
    has no major axis."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    R, U, F = env.right, env.up, env.forward
    n = env.n
    with np.errstate(all="ignore"):
        x = (d[:, 0] * R[0] + d[:, 1] * R[1]) + d[:, 2] * R[2]
        y = (d[:, 0] * U[0] + d[:, 1] * U[1]) + d[:, 2] * U[2]
        z = (d[:, 0] * F[0] + d[:, 1] * F[1]) + d[:, 2] * F[2]
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        m = np.maximum(np.maximum(ax, ay), az)  # NaN if any is NaN
        ok = (m > 0) & (m < np.inf)
    out = np.empty((len(d), 3))
    out[~ok] = np.array([float(v) for v in background])
    x, y, z, ax, ay, az, m = (a[ok] for a in (x, y, z, ax, ay, az, m))
    fx_ = ax >= ay
    fx_ &= ax >= az
    fy_ = ~fx_ & (ay >= az)
    fz_ = ~fx_ & ~fy_
    face = np.where(fx_, np.where(x > 0, 0, 1), np.where(fy_, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
    un = np.select([face == 0, face == 1, face == 5], [-z, z, -x], x)   # u's numerator
    vn = np.select([face == 2, face == 3], [z, -z], -y)                 # v's numerator
    u, v = un / m, vn / m
    h = 0.5 * float(n)
    fx, fy = (u + 1.0) * h, (v + 1.0) * h
    row0 = face * n
    t = env.texels
    if env.filter == NEAREST:
        col = np.clip(np.floor(fx).astype(np.int64), 0, n - 1)
        row = np.clip(np.floor(fy).astype(np.int64), 0, n - 1)
        out[ok] = t[row0 + row, col]
        return out
    gx, gy = fx - 0.5, fy - 0.5
    x0f, y0f = np.floor(gx), np.floor(gy)
    wx, wy = (gx - x0f)[:, None], (gy - y0f)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    ca, cb = np.clip(x0, 0, n - 1), np.clip(x0 + 1, 0, n - 1)
    ra, rb = row0 + np.clip(y0, 0, n - 1), row0 + np.clip(y0 + 1, 0, n - 1)
    c00, c10, c01, c11 = t[ra, ca], t[ra, cb], t[rb, ca], t[rb, cb]
    with np.errstate(all="ignore"):
        a = c00 + wx * (c10 - c00)
        b = c01 + wx * (c11 - c01)
        out[ok] = a + wy * (b - a)
    return out


def traceable(rays):
    """csrc/crt_ray_class.h's ray_traceable with t_max = +inf: six finite numbers, a direction not all zero."""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    return np.isfinite(rays).all(1) & (rays[:, 3:] != 0).any(1)


def pow5(x):
    return float(Fraction(x) ** 5)


def _unit_vector(crt, rng):
    """random_unit_vector: (state, x, y, z)."""
    while True:
        rng, x = crt.rand_double(rng, -1.0, 1.0)
        rng, y = crt.rand_double(rng, -1.0, 1.0)
        rng, z = crt.rand_double(rng, -1.0, 1.0)
        if x * x + y * y + z * z < 1:
            break
    inv = 1 / math.sqrt(x * x + y * y + z * z)
    return rng, x * inv, y * inv, z * inv


def scatter(crt, kind, color, param, d, n, front, rng):
    """shade()'s scatter of one hit on a Lambertian, Metal or Dielectric: (new direction or None when
    a Metal absorbs, the state after the draws). d, n: lists of 3 floats, n facing the ray."""
    lam, met, die = kind == LAMBERTIAN, kind == METAL, kind == DIELECTRIC
    ux = uy = uz = 0.0
    if met or die:
        il = 1 / math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        ux, uy, uz = d[0] * il, d[1] * il, d[2] * il
    reflect = met
    cosv = ratio = 0.0
    if die:
        ri = param
        ratio = (1. / ri) if front else ri
        cosv = min((-ux) * n[0] + (-uy) * n[1] + (-uz) * n[2], 1.)
        sinv = math.sqrt(1 - cosv * cosv)
        if ratio * sinv > 1:
            reflect = True
        else:
            r = ((1 - 1. / ri) / (1 + 1. / ri)) if front else ((1 - ri / 1.) / (1 + ri / 1.))
            r0 = r * r
            pw = pow5(1 - cosv)
            rng, u = crt.rand_double(rng, 0.0, 1.0)
            reflect = u < r0 + (1 - r0) * pw
    rx = ry = rz = 0.0
    if lam or met:
        rng, rx, ry, rz = _unit_vector(crt, rng)
    if reflect:
        k2 = 2 * (ux * n[0] + uy * n[1] + uz * n[2])
        nd = [ux - n[0] * k2, uy - n[1] * k2, uz - n[2] * k2]
        if met:
            nd = [nd[0] + rx * param, nd[1] + ry * param, nd[2] + rz * param]
            if n[0] * nd[0] + n[1] * nd[1] + n[2] * nd[2] < 0:
                return None, rng
    elif die:
        px, py, pz = (ux + n[0] * cosv) * ratio, (uy + n[1] * cosv) * ratio, (uz + n[2] * cosv) * ratio
        sq = -math.sqrt(abs(1 - (px * px + py * py + pz * pz)))
        nd = [px + n[0] * sq, py + n[1] * sq, pz + n[2] * sq]
    else:
        nd = [n[0] + rx, n[1] + ry, n[2] + rz]
        if abs(nd[0]) < 1e-8 and abs(nd[1]) < 1e-8 and abs(nd[2]) < 1e-8:
            nd = list(n)
    return nd, rng


def ray_color(orc, scene, rays, states, max_depth, background, t_min=1e-5, env=None, crt=None, bvh=None):
    """crt_radiance_async's (or, with env, crt_radiance_env_async's) output for rays (n, 6) and LCG
    states (n,) uint32: (rgb (n, 3), how each path ended (n,) of MISS / LIGHT / ABSORBED / DEPTH, its
    last direction (n, 3), its throughput at the end (n, 3)). A ray outside the query contract is a
    first-segment miss, never traced. max_depth == 0: zeros, every path ends as DEPTH. bvh: the
    scene's BVH parameters for oracle.hits (num_buckets, max_prims) where they are not the defaults."""
    if crt is None:
        import cpp_raytracer_amd as crt
    rays = np.array(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    T = np.ones((n, 3))
    rng = [int(s) for s in np.asarray(states, np.uint32).reshape(-1)]
    rgb = np.zeros((n, 3))
    ended = np.full(n, DEPTH, np.int64)
    bg = [float(v) for v in background]
    if max_depth == 0:
        return rgb, ended, d, T
    ok = traceable(rays)
    live = np.flatnonzero(ok)
    missed = [np.flatnonzero(~ok)]
    mat = scene.materials
    for depth_left in range(max_depth, 0, -1):
        if len(live) == 0:
            break
        h = orc.hits(scene, np.concatenate([o[live], d[live]], 1), t_min, **(bvh or {}))
        hit = h["prim"] >= 0
        missed.append(live[~hit])
        nxt = []
        for j in np.flatnonzero(hit):
            i = int(live[j])
            m = mat[int(h["material"][j])]
            kind = int(m["kind"])
            color, param = [float(c) for c in m["color"]], float(m["param"])
            if kind == DIFFUSE_LIGHT:
                rgb[i] = [0.0 + T[i, k] * (color[k] * param) for k in range(3)]
                ended[i] = LIGHT
                continue
            nd, rng[i] = scatter(crt, kind, color, param, d[i].tolist(), [float(v) for v in h["normal"][j]],
                                 bool(h["front_face"][j]), rng[i])
            if nd is None:
                ended[i] = ABSORBED
                continue
            if kind != DIELECTRIC:
                T[i] = [T[i, k] * color[k] for k in range(3)]
            o[i] = h["point"][j]
            d[i] = nd
            if depth_left > 1:
                nxt.append(i)  # else: no bounce left, the path returns zero (DEPTH)
        live = np.array(nxt, np.int64)
    missed = np.concatenate(missed)
    ended[missed] = MISS
    if len(missed):
        e = lookup(env, d[missed], bg) if env is not None else np.array([bg] * len(missed))
        with np.errstate(all="ignore"):
            rgb[missed] = 0.0 + T[missed] * e
    return rgb, ended, d, T
