"""A numpy and Python-float restatement of the lit estimator (include/crt_render.h, crt_lighting): an
environment and the scene's own lights under one argument, computed without a GPU. Not a test module.

A lighting is two independent choices: the environment (None: the constant background; an env_model.Env
alone: the plain map; an Env with env_nee_model's Tables: the sampled map) and the lights (None, or
light_nee_model's Tables). The tables, env_sample, env_pdf, light_pick, light_point and light_pdf are
imported from the two models unchanged; the loop is env_model.ray_color's (the hits from the oracle,
env_model.scatter), restated here with both samples a Lambertian bounce:

  all of the map sample's draws, then the light sample's; pb; the map's shadow segment (any hit occludes)
  and its term; then the light's (closest hit, its own slot) and its term; then the scattered ray.

ray_color returns the output, how each path ended and a Trace of every event, for the tests' counts.
numpy float64 and Python floats are IEEE doubles and never fused, np.sqrt and math.sqrt are correctly
rounded, so every value here is the kernel's bits.
"""
import math
from dataclasses import dataclass, field

import numpy as np

import env_model as em
import env_nee_model as enm
import light_nee_model as lm

PI = 3.141592653589793
PATTERNS = ("both", "map_only", "light_only", "none")
EVENTS = ("map_kept", "map_occluded", "map_skipped", "light_kept", "light_hidden_other", "light_hidden_light",
          "light_no_ray", "hits_weighted", "hits_plain", "escapes_weighted", "escapes_plain") + PATTERNS


@dataclass
class Lighting:
    env: object = None   # env_model.Env, or None: the constant background
    etb: object = None   # env_nee_model.Tables: the map is sampled; None: plain
    ltb: object = None   # light_nee_model.Tables: the lights are sampled; None: not


@dataclass
class Trace:
    """What ray_color did besides its output: one entry per event, `path` the path's index."""
    map_kept: list = field(default_factory=list)            # (path, the added (T * E) * f as 3 floats)
    map_occluded: list = field(default_factory=list)        # path: the map's shadow segment hit something
    map_skipped: list = field(default_factory=list)         # path: below the horizon or zero density, no ray
    map_below: list = field(default_factory=list)           # path: of map_skipped, !(c_e > 0)
    map_zero_pdf: list = field(default_factory=list)        # path: of map_skipped, c_e > 0 and !(pe > 0)
    light_kept: list = field(default_factory=list)          # (path, the added (T * emit) * f as 3 floats)
    light_hidden_other: list = field(default_factory=list)  # path: the light's shadow segment ended on a non-light
    light_hidden_light: list = field(default_factory=list)  # path: it ended on another light
    light_dropped: list = field(default_factory=list)       # path: it missed everything, or pl not in (0, inf)
    light_no_ray: list = field(default_factory=list)        # path: a far-side point or !(c_l > 0), no ray
    light_far_side: list = field(default_factory=list)      # path: of light_no_ray, a sphere's far side
    light_below: list = field(default_factory=list)         # path: of light_no_ray, !(c_l > 0) (asked first)
    hits_weighted: list = field(default_factory=list)       # (path, f): a light hit weighted against the sampler
    hits_plain: list = field(default_factory=list)          # path: a light hit with f = 1 (pb none, or no sampler)
    escapes_weighted: list = field(default_factory=list)    # (path, f): an escape weighted against the sampler
    escapes_plain: list = field(default_factory=list)       # path: an escape with f = 1 (pb none, or no sampler)
    lambertian: set = field(default_factory=set)            # paths that scattered off a Lambertian at least once
    both: list = field(default_factory=list)                # path, per bounce: both shadow rays were sent
    map_only: list = field(default_factory=list)            # path, per bounce: the map's alone
    light_only: list = field(default_factory=list)          # path, per bounce: the light's alone
    none: list = field(default_factory=list)                # path, per bounce: neither


def counts(tr):
    return {k: len(getattr(tr, k)) for k in EVENTS}


def _f(x):
    return np.float64(x)


def ray_color(orc, scene, rays, states, max_depth, background, t_min, lit, crt=None, bvh=None):
    """The *_lit entries' output for rays (n, 6) and LCG states (n,) uint32 under the Lighting `lit`: (rgb
    (n, 3), how each path ended (env_model's MISS / LIGHT / ABSORBED / DEPTH), a Trace)."""
    if crt is None:
        import cpp_raytracer_amd as crt
    env, etb, ltb = lit.env, lit.etb, lit.ltb
    assert etb is None or env is not None
    rays = np.array(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    T = np.ones((n, 3))
    rng = [int(s) for s in np.asarray(states, np.uint32).reshape(-1)]
    acc = np.zeros((n, 3))
    pb = [None] * n
    ended = np.full(n, em.DEPTH, np.int64)
    tr = Trace()
    bg = [float(v) for v in background]
    if max_depth == 0:
        return acc, ended, tr
    kw = bvh or {}

    def escape(idx):
        if len(idx) == 0:
            return
        ended[idx] = em.MISS
        if env is None:
            for i in idx.tolist():
                acc[i] = [acc[i, k] + T[i, k] * bg[k] for k in range(3)]
                tr.escapes_plain.append(i)
            return
        e = em.lookup(env, d[idx], bg)
        if etb is None:
            with np.errstate(all="ignore"):
                acc[idx] = acc[idx] + T[idx] * e
            tr.escapes_plain.extend(idx.tolist())
            return
        pe = enm.pdf(env, etb, d[idx])
        for j, i in enumerate(idx.tolist()):
            f = 1.0
            if pb[i] is None:
                tr.escapes_plain.append(i)
            else:
                with np.errstate(all="ignore"):
                    s = float(_f(pe[j]) + _f(pb[i]))
                    f = float(_f(pb[i]) / _f(s)) if s > 0 else 0.0
                tr.escapes_weighted.append((i, f))
            with np.errstate(all="ignore"):
                acc[i] = [float(_f(acc[i, k]) + (_f(T[i, k]) * _f(e[j, k])) * _f(f)) for k in range(3)]

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
        nxt = []
        lam, lam_n = [], []  # the Lambertian bounces of this level with a bounce left, and their normals
        for j in np.flatnonzero(hit):
            i = int(live[j])
            mt = mat[int(h["material"][j])]
            kind = int(mt["kind"])
            color, param = [float(c) for c in mt["color"]], float(mt["param"])
            if kind == em.DIFFUSE_LIGHT:
                ended[i] = em.LIGHT
                if ltb is None:  # shade's own acc + T * emit
                    acc[i] = [acc[i, k] + T[i, k] * (color[k] * param) for k in range(3)]
                    tr.hits_plain.append(i)
                    continue
                li = ltb.of_prim[int(h["prim"][j])]
                f = 1.0
                if pb[i] is None:
                    tr.hits_plain.append(i)
                else:
                    pl = float(lm.pdf(ltb, li, h["t"][j], h["normal"][j], d[i], h["front_face"][j] != 0)[0])
                    with np.errstate(all="ignore"):
                        s = float(_f(pl) + _f(pb[i]))
                        f = float(_f(pb[i]) / _f(s)) if s > 0 else 0.0
                    tr.hits_weighted.append((i, f))
                e = ltb.emit[li]
                with np.errstate(all="ignore"):
                    acc[i] = [float(_f(acc[i, k]) + (_f(T[i, k]) * e[k]) * _f(f)) for k in range(3)]
                continue
            nrm = [float(v) for v in h["normal"][j]]
            nd, rng[i] = em.scatter(crt, kind, color, param, d[i].tolist(), nrm, bool(h["front_face"][j]), rng[i])
            if nd is None:
                ended[i] = em.ABSORBED
                continue
            if kind != em.DIELECTRIC:
                T[i] = [T[i, k] * color[k] for k in range(3)]
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
            lam.append(i)
            lam_n.append(nrm)
        if lam and (etb is not None or ltb is not None):
            k_ = len(lam)
            ray_e, ray_l = [False] * k_, [False] * k_
            d_e, w_e = [None] * k_, [0.0] * k_
            d_l, c_l, l_i = [None] * k_, [0.0] * k_, [0] * k_
            # 1. the map sample: four draws each, always
            if etb is not None:
                xi = []
                for i in lam:
                    row = []
                    for _ in range(4):
                        rng[i], x = crt.rand_double(rng[i], 0.0, 1.0)
                        row.append(x)
                    xi.append(row)
                xi = np.array(xi, np.float64)
                N = np.array(lam_n, np.float64)
                de = enm.sample(env, etb, xi[:, 0], xi[:, 1], xi[:, 2], xi[:, 3])
                with np.errstate(all="ignore"):
                    ce = enm.dot(N, de) / np.sqrt(enm.dot(de, de))
                    pe = enm.pdf(env, etb, de)
                    pbe = ce / PI
                    fe = pbe / (pe + pbe)
                for j, i in enumerate(lam):
                    ray_e[j] = bool(ce[j] > 0 and pe[j] > 0)
                    d_e[j], w_e[j] = de[j], float(fe[j])
                    if not ray_e[j]:
                        tr.map_skipped.append(i)
                        (tr.map_zero_pdf if ce[j] > 0 else tr.map_below).append(i)
            # 2. the light sample: its draws after all of the map's
            if ltb is not None:
                for j, i in enumerate(lam):
                    rng[i], xi1 = crt.rand_double(rng[i], 0.0, 1.0)
                    li = int(lm.pick(ltb, xi1)[0])
                    rng[i], p, u = lm.point(crt, ltb, li, rng[i])
                    oi = o[i].tolist()
                    dl = [p[k] - oi[k] for k in range(3)]
                    with np.errstate(all="ignore"):
                        cl = float(_f(lm.dot(lam_n[j], dl)) / np.sqrt(_f(lm.dot(dl, dl))))
                    d_l[j], c_l[j], l_i[j] = dl, cl, li
                    if not cl > 0:
                        tr.light_no_ray.append(i)
                        tr.light_below.append(i)
                    elif u is not None and not lm.dot(u, dl) < 0:
                        tr.light_no_ray.append(i)
                        tr.light_far_side.append(i)
                    else:
                        ray_l[j] = True
            # 3. pb of the scattered direction
            for j, i in enumerate(lam):
                nd = d[i].tolist()
                with np.errstate(all="ignore"):
                    pb[i] = float((_f(lm.dot(lam_n[j], nd)) / np.sqrt(_f(lm.dot(nd, nd)))) / PI)
                pat = "both" if ray_e[j] and ray_l[j] else "map_only" if ray_e[j] else "light_only" if ray_l[j] else "none"
                getattr(tr, pat).append(i)
            # 4. the map's shadow segments: any hit occludes
            je = [j for j in range(k_) if ray_e[j]]
            if je:
                s_i = np.array([lam[j] for j in je], np.int64)
                s_d = np.array([d_e[j] for j in je], np.float64)
                hs = orc.hits(scene, np.concatenate([o[s_i], s_d], 1), t_min, **kw)
                e = em.lookup(env, s_d, bg)
                for q, j in enumerate(je):
                    i = lam[j]
                    if hs["prim"][q] >= 0:
                        tr.map_occluded.append(i)
                        continue
                    with np.errstate(all="ignore"):
                        add = [float((_f(T[i, k]) * _f(e[q, k])) * _f(w_e[j])) for k in range(3)]
                        acc[i] = [float(_f(acc[i, k]) + add[k]) for k in range(3)]
                    tr.map_kept.append((i, add))
            # 5. the lights' shadow segments: closest hit, the sampled light's own slot
            jl = [j for j in range(k_) if ray_l[j]]
            if jl:
                s_i = np.array([lam[j] for j in jl], np.int64)
                s_d = np.array([d_l[j] for j in jl], np.float64)
                hs = orc.hits(scene, np.concatenate([o[s_i], s_d], 1), t_min, **kw)
                for q, j in enumerate(jl):
                    i, li = lam[j], l_i[j]
                    p = int(hs["prim"][q])
                    if p != int(ltb.prim[li]):
                        if p < 0:
                            tr.light_dropped.append(i)
                        elif p in ltb.of_prim:
                            tr.light_hidden_light.append(i)
                        else:
                            tr.light_hidden_other.append(i)
                        continue
                    pl = float(lm.pdf(ltb, li, hs["t"][q], hs["normal"][q], d_l[j], hs["front_face"][q] != 0)[0])
                    if not (pl > 0 and pl < math.inf):
                        tr.light_dropped.append(i)
                        continue
                    pbl = c_l[j] / PI
                    f = pbl / (pl + pbl)
                    em_ = ltb.emit[li]
                    with np.errstate(all="ignore"):
                        add = [float((_f(T[i, k]) * em_[k]) * _f(f)) for k in range(3)]
                        acc[i] = [float(_f(acc[i, k]) + add[k]) for k in range(3)]
                    tr.light_kept.append((i, add))
        elif lam:  # nothing is sampled: pb is never read
            for i in lam:
                tr.none.append(i)
        live = np.array(nxt, np.int64)
    return acc, ended, tr
