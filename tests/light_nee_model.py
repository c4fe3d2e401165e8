"""A numpy and Python-float restatement of the sampling of a scene's own lights (include/crt_render.h,
crt_light_sampler): what the device must build and write, computed without a GPU. Not a test module.

  flatten    the scene's flattened primitives (csrc/crt_prims.h: a Box gives six parallelograms).
  tables     the lights in pick order with prim, w, cdf and W, the sums sequential.
  pick       light_pick over arrays of numbers.
  point      light_point of one light from an LCG state (Python floats).
  pdf        light_pdf of hits on a light, over arrays.
  ray_color  the estimator: env_model.ray_color's loop (the hits from the oracle, env_model.scatter) with
             next-event estimation of the lights at every Lambertian bounce and the balance heuristic.
             Besides the output it returns a Trace of every event, for the tests' counts and statistics.

numpy float64 and Python floats are IEEE doubles and never fused, np.sqrt and math.sqrt are correctly
rounded and np.add.accumulate adds in order, so every value here is the kernel's bits.
"""
import math
from dataclasses import dataclass, field

import numpy as np

import env_model as em

PI = 3.141592653589793
SPHERE, QUAD = 1, 2


def _gmin(x, y):  # crt_prims.h's gfmin / gfmax on numbers that are not NaN
    return x if x < y else y


def _gmax(x, y):
    return x if x > y else y


def flatten(scene):
    """[(kind, material, geometry)] in flattened primitive order: a sphere's geometry is (c (3,), r),
    a parallelogram's (v, s1, s2), each a list of floats."""
    out = []
    for o in scene.objects:
        kind, mat = int(o["kind"]), int(o["material"])
        v = [float(x) for x in o["v"]]
        if kind == 1:
            out.append((SPHERE, mat, (v[:3], v[3])))
        elif kind == 2:
            out.append((QUAD, mat, (v[0:3], v[3:6], v[6:9])))
        else:
            mn = [_gmin(v[k], v[3 + k]) for k in range(3)]
            mx = [_gmax(v[k], v[3 + k]) for k in range(3)]
            sx, sy, sz = [mx[0] - mn[0], 0.0, 0.0], [0.0, mx[1] - mn[1], 0.0], [0.0, 0.0, mx[2] - mn[2]]
            nx, ny, nz = [-a for a in sx], [-a for a in sy], [-a for a in sz]
            for q in ((mn, sx, sy), (mn, sx, sz), (mn, sy, sz), (mx, nx, ny), (mx, nx, nz), (mx, ny, nz)):
                out.append((QUAD, mat, q))
    return out


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def area(kind, g):
    if kind == QUAD:
        _, s1, s2 = g
        cr = [s1[1] * s2[2] - s1[2] * s2[1], s1[2] * s2[0] - s1[0] * s2[2], s1[0] * s2[1] - s1[1] * s2[0]]
        return math.sqrt(dot(cr, cr))
    return (4.0 * PI) * (g[1] * g[1])


@dataclass
class Tables:
    prim: np.ndarray   # (L,) uint32, ascending
    w: np.ndarray      # (L,)
    cdf: np.ndarray    # (L,)
    W: float
    kind: list         # per light SPHERE / QUAD
    geom: list         # per light its geometry
    emit: list         # per light [e0, e1, e2]
    area: list
    of_prim: dict      # flattened primitive index -> light index


def tables(scene):
    """The sampler's tables, or None for a scene without a light."""
    prims = flatten(scene)
    mats = scene.materials
    prim, w, kind, geom, emit, ar = [], [], [], [], [], []
    for p, (k, m, g) in enumerate(prims):
        mt = mats[m]
        if int(mt["kind"]) != em.DIFFUSE_LIGHT:
            continue
        param = float(mt["param"])
        with np.errstate(all="ignore"):
            e = [float(np.float64(c) * np.float64(param)) for c in mt["color"]]
            Y = float((np.float64(0.2126) * e[0] + np.float64(0.7152) * e[1]) + np.float64(0.0722) * e[2])
            Y = Y if Y > 0 else 0.0
            A = area(k, g)
            wi = float(np.float64(Y) * np.float64(A))
        prim.append(p), w.append(wi), kind.append(k), geom.append(g), emit.append(e), ar.append(A)
    if not prim:
        return None
    w = np.array(w, np.float64)
    with np.errstate(all="ignore"):
        cdf = np.ascontiguousarray(np.add.accumulate(np.concatenate([[0.0], w]))[1:])
    return Tables(np.array(prim, np.uint32), w, cdf, float(cdf[-1]), kind, geom, emit, ar,
                  {p: i for i, p in enumerate(prim)})


def usable(tb):
    """crt_light_sampler_create's rules: a light, and a positive finite total."""
    return tb is not None and bool(tb.W > 0 and tb.W < np.inf)


def pick(tb, xi1):
    xi1 = np.asarray(xi1, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        return np.minimum((tb.cdf[None, :] <= (xi1 * tb.W)[:, None]).sum(1), len(tb.cdf) - 1)


def point(crt, tb, i, rng):
    """light_point(i, state): (state after the draws, p, u): u is the sphere's unit vector, None for a
    parallelogram."""
    if tb.kind[i] == QUAD:
        v, s1, s2 = tb.geom[i]
        rng, xi2 = crt.rand_double(rng, 0.0, 1.0)
        rng, xi3 = crt.rand_double(rng, 0.0, 1.0)
        return rng, [(v[k] + s1[k] * xi2) + s2[k] * xi3 for k in range(3)], None
    c, r = tb.geom[i]
    rng, x, y, z = em._unit_vector(crt, rng)
    u = [x, y, z]
    return rng, [c[k] + u[k] * abs(r) for k in range(3)], u


def pdf(tb, i, t, n, d, front):
    """light_pdf over arrays: hits at t (k,) with normals n (k, 3), front (k,) of rays with directions
    d (k, 3), all on light i."""
    t = np.asarray(t, np.float64).reshape(-1)
    n = np.asarray(n, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    front = np.asarray(front, bool).reshape(-1)
    outside = np.ones(len(t), bool)
    if tb.kind[i] == SPHERE:
        outside = front == (tb.geom[i][1] > 0)
    w = tb.w[i]
    if not w > 0:
        return np.zeros(len(t))
    with np.errstate(all="ignore"):
        v = d * t[:, None]
        vv = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        nv = (n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1]) + n[:, 2] * v[:, 2]
        pl = ((w / tb.W) / tb.area[i]) * ((vv * np.sqrt(vv)) / np.abs(nv))
    return np.where(outside, pl, 0.0)


@dataclass
class Trace:
    """What ray_color did besides its output: one entry per event, `path` the path's index."""
    kept: list = field(default_factory=list)            # (path, the added (T * e) * f as 3 floats)
    hidden_other: list = field(default_factory=list)    # path: the shadow ray stopped on something that is no light
    hidden_light: list = field(default_factory=list)    # path: it stopped on another light
    dropped: list = field(default_factory=list)         # path: it reached its light with pl not in (0, inf), or missed
    far_side: list = field(default_factory=list)        # path: a sphere's far-side point, no ray
    below: list = field(default_factory=list)           # path: !(c_s > 0), no ray
    hits_weighted: list = field(default_factory=list)   # (path, f): a light hit with pb not none
    hits_plain: list = field(default_factory=list)      # path: a light hit with pb none (f = 1)
    after_specular: list = field(default_factory=list)  # path: a hits_plain after a Metal or Dielectric bounce
    lambertian: set = field(default_factory=set)        # paths that scattered off a Lambertian at least once
    missed: list = field(default_factory=list)          # path: the half of dropped whose shadow ray hit nothing
    unweighable: list = field(default_factory=list)     # path: the other half: its light reached, pl not in (0, inf)
    picks: list = field(default_factory=list)           # (path, light index, xi1) of every sample drawn
    inside_hits: list = field(default_factory=list)     # path: a light hit with pb set on a sphere's inside (pl = 0)


def ray_color(orc, scene, rays, states, max_depth, background, t_min, tb, crt=None, bvh=None):
    """crt_radiance_lights_async's output for rays (n, 6) and LCG states (n,) uint32: (rgb (n, 3), how each
    path ended (env_model's MISS / LIGHT / ABSORBED / DEPTH), a Trace)."""
    if crt is None:
        import cpp_raytracer_amd as crt
    rays = np.array(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    T = np.ones((n, 3))
    rng = [int(s) for s in np.asarray(states, np.uint32).reshape(-1)]
    acc = np.zeros((n, 3))
    pb = [None] * n
    bounced = np.zeros(n, bool)
    ended = np.full(n, em.DEPTH, np.int64)
    tr = Trace()
    bg = [float(v) for v in background]
    if max_depth == 0:
        return acc, ended, tr
    kw = bvh or {}

    def escape(idx):
        for i in idx.tolist():
            acc[i] = [acc[i, k] + T[i, k] * bg[k] for k in range(3)]
        ended[idx] = em.MISS

    ok = em.traceable(rays)
    escape(np.flatnonzero(~ok))
    live = np.flatnonzero(ok)
    mat = scene.materials
    for depth_left in range(max_depth, 0, -1):
        if len(live) == 0:
            break
        h = orc.hits(scene, np.concatenate([o[live], d[live]], 1), t_min, **kw)
        hit = h["prim"] >= 0
        escape(live[~hit])
        nxt, sh = [], []  # sh: (path, light, c_s, d_s)
        for j in np.flatnonzero(hit):
            i = int(live[j])
            mt = mat[int(h["material"][j])]
            kind = int(mt["kind"])
            color, param = [float(c) for c in mt["color"]], float(mt["param"])
            if kind == em.DIFFUSE_LIGHT:
                li = tb.of_prim[int(h["prim"][j])]
                f = 1.0
                if pb[i] is None:
                    tr.hits_plain.append(i)
                    if bounced[i]:
                        tr.after_specular.append(i)
                else:
                    pl = float(pdf(tb, li, h["t"][j], h["normal"][j], d[i], h["front_face"][j] != 0)[0])
                    if tb.kind[li] == SPHERE and (h["front_face"][j] != 0) != (tb.geom[li][1] > 0):
                        tr.inside_hits.append(i)
                    s = pl + pb[i]
                    f = pb[i] / s if s > 0 else 0.0
                    tr.hits_weighted.append((i, f))
                e = tb.emit[li]
                with np.errstate(all="ignore"):
                    acc[i] = [float(np.float64(acc[i, k]) + (np.float64(T[i, k]) * e[k]) * np.float64(f)) for k in range(3)]
                ended[i] = em.LIGHT
                continue
            nrm = [float(v) for v in h["normal"][j]]
            nd, rng[i] = em.scatter(crt, kind, color, param, d[i].tolist(), nrm, bool(h["front_face"][j]), rng[i])
            if nd is None:
                ended[i] = em.ABSORBED
                continue
            if kind != em.DIELECTRIC:
                T[i] = [T[i, k] * color[k] for k in range(3)]
            bounced[i] = True
            if kind == em.LAMBERTIAN:
                tr.lambertian.add(i)
            o[i] = h["point"][j]
            d[i] = nd
            if depth_left == 1:
                continue  # no bounce left: the path ends with what it gathered (DEPTH)
            nxt.append(i)
            if kind != em.LAMBERTIAN:
                pb[i] = None
                continue
            rng[i], xi1 = crt.rand_double(rng[i], 0.0, 1.0)
            li = int(pick(tb, xi1)[0])
            tr.picks.append((i, li, xi1))
            rng[i], p, u = point(crt, tb, li, rng[i])
            oi = o[i].tolist()
            ds = [p[k] - oi[k] for k in range(3)]
            with np.errstate(all="ignore"):
                cs = float(np.float64(dot(nrm, ds)) / np.sqrt(np.float64(dot(ds, ds))))
                pb[i] = float((np.float64(dot(nrm, nd)) / np.sqrt(np.float64(dot(nd, nd)))) / PI)
            if not cs > 0:
                tr.below.append(i)
            elif u is not None and not dot(u, ds) < 0:
                tr.far_side.append(i)
            else:
                sh.append((i, li, cs, ds))
        if sh:
            s_i = np.array([a[0] for a in sh], np.int64)
            s_d = np.array([a[3] for a in sh], np.float64)
            hs = orc.hits(scene, np.concatenate([o[s_i], s_d], 1), t_min, **kw)
            for j, (i, li, cs, ds) in enumerate(sh):
                p = int(hs["prim"][j])
                if p != int(tb.prim[li]):
                    if p < 0:
                        tr.dropped.append(i)
                        tr.missed.append(i)
                    elif p in tb.of_prim:
                        tr.hidden_light.append(i)
                    else:
                        tr.hidden_other.append(i)
                    continue
                pl = float(pdf(tb, li, hs["t"][j], hs["normal"][j], ds, hs["front_face"][j] != 0)[0])
                if not (pl > 0 and pl < math.inf):
                    tr.dropped.append(i)
                    tr.unweighable.append(i)
                    continue
                pbs = cs / PI
                f = pbs / (pl + pbs)
                e = tb.emit[li]
                with np.errstate(all="ignore"):
                    add = [float((np.float64(T[i, k]) * e[k]) * np.float64(f)) for k in range(3)]
                    acc[i] = [float(np.float64(acc[i, k]) + add[k]) for k in range(3)]
                tr.kept.append((i, add))
        live = np.array(nxt, np.int64)
    return acc, ended, tr
