"""A numpy restatement of luminance sampling of cube-map environments (include/crt_render.h,
crt_env_sampler): what the device must build and write, computed without a GPU. Not a test module.

  tables     w, c, m and W of a map, the sums sequential in the header's order.
  project    steps 1 to 5 of E(d) (the face, u, v, fx, fy), restated here because env_model.lookup
             keeps them to itself; test_env_nee_model.py holds it to env_model.lookup.
  pdf        env_pdf(d) over arrays of directions.
  sample     env_sample(xi1..xi4) over arrays of numbers.
  ray_color  the estimator: env_model.ray_color's loop (the hits from the oracle, env_model.scatter,
             env_model.lookup) with next-event estimation at every Lambertian bounce and the balance
             heuristic. Besides the output it returns every contribution it added, for the tests'
             statistics.

numpy float64 arithmetic is IEEE and never fused, np.sqrt is correctly rounded and np.add.accumulate
adds in order, so every value here is the kernel's bits.
"""
from dataclasses import dataclass, field

import numpy as np

import env_model as em

PI = 3.141592653589793


@dataclass
class Tables:
    w: np.ndarray  # (6n, n)
    c: np.ndarray  # (6n, n)
    m: np.ndarray  # (6n,)
    W: float


def tables(env):
    t = env.texels
    n = env.n
    with np.errstate(all="ignore"):
        Y = (0.2126 * t[:, :, 0] + 0.7152 * t[:, :, 1]) + 0.0722 * t[:, :, 2]
        Y = np.where(Y > 0, Y, 0.0)
        g = 2.0 / float(n)
        uc = (np.arange(n, dtype=np.float64) + 0.5) * g - 1.0  # per column, and per row_in_face
        vc = np.tile(uc, 6)
        sc = (1.0 + uc[None, :] * uc[None, :]) + vc[:, None] * vc[:, None]
        w = Y / (sc * np.sqrt(sc))
        c = np.ascontiguousarray(np.add.accumulate(np.concatenate([np.zeros((6 * n, 1)), w], 1), 1)[:, 1:])
        m = np.ascontiguousarray(np.add.accumulate(np.concatenate([[0.0], c[:, n - 1]]))[1:])
    return Tables(np.ascontiguousarray(w), c, m, float(m[-1]))


def usable(tb):
    """crt_env_sampler_create's rule on the total."""
    return bool(tb.W > 0 and tb.W < np.inf)


def project(env, dirs):
    """(ok, face, u, v, h, fx, fy) of dirs (k, 3); where ok is False the rest is meaningless."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    R, U, F = env.right, env.up, env.forward
    with np.errstate(all="ignore"):
        x = (d[:, 0] * R[0] + d[:, 1] * R[1]) + d[:, 2] * R[2]
        y = (d[:, 0] * U[0] + d[:, 1] * U[1]) + d[:, 2] * U[2]
        z = (d[:, 0] * F[0] + d[:, 1] * F[1]) + d[:, 2] * F[2]
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        m = np.maximum(np.maximum(ax, ay), az)  # NaN if any is NaN
        ok = (m > 0) & (m < np.inf)
        fx_ = (ax >= ay) & (ax >= az)
        fy_ = ~fx_ & (ay >= az)
        face = np.where(fx_, np.where(x > 0, 0, 1), np.where(fy_, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
        un = np.select([face == 0, face == 1, face == 5], [-z, z, -x], x)
        vn = np.select([face == 2, face == 3], [z, -z], -y)
        u, v = un / m, vn / m
        h = 0.5 * float(env.n)
        fx, fy = (u + 1.0) * h, (v + 1.0) * h
    return ok, face, u, v, h, fx, fy


def pdf(env, tb, dirs):
    ok, face, u, v, h, fx, fy = project(env, dirs)
    n = env.n
    out = np.zeros(len(ok))
    with np.errstate(all="ignore"):
        col = np.clip(np.floor(np.where(ok, fx, 0.0)).astype(np.int64), 0, n - 1)
        row = np.clip(np.floor(np.where(ok, fy, 0.0)).astype(np.int64), 0, n - 1)
        s = (1.0 + u * u) + v * v
        hh = h * h
        p = ((tb.w[np.where(ok, face, 0) * n + row, col] / tb.W) * hh) * (s * np.sqrt(s))
    out[ok] = p[ok]
    return out


def pick(env, tb, xi1, xi2):
    """(r, k): the row and the column env_sample picks."""
    n = env.n
    xi1, xi2 = np.asarray(xi1, np.float64).reshape(-1), np.asarray(xi2, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        r = np.minimum((tb.m[None, :] <= (xi1 * tb.W)[:, None]).sum(1), 6 * n - 1)
        cr = tb.c[r]
        k = np.minimum((cr <= (xi2 * cr[:, n - 1])[:, None]).sum(1), n - 1)
    return r, k


def sample(env, tb, xi1, xi2, xi3, xi4):
    """env_sample over arrays: (k, 3) directions in world space, unnormalised."""
    n = env.n
    r, k = pick(env, tb, xi1, xi2)
    xi3, xi4 = np.asarray(xi3, np.float64).reshape(-1), np.asarray(xi4, np.float64).reshape(-1)
    face, rf = r // n, r % n
    g = 2.0 / float(n)
    fx, fy = k.astype(np.float64) + xi3, rf.astype(np.float64) + xi4
    u, v = fx * g - 1.0, fy * g - 1.0
    one = np.ones(len(u))
    x = np.select([face == 0, face == 1, face == 5], [one, -one, -u], u)
    y = np.select([face == 2, face == 3], [one, -one], -v)
    z = np.select([face == 0, face == 1, face == 2, face == 3, face == 4], [-u, u, v, -v, one], -one)
    R, U, F = env.right, env.up, env.forward
    return np.stack([(R[j] * x + U[j] * y) + F[j] * z for j in range(3)], 1)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


@dataclass
class Trace:
    """What ray_color did besides its output: one entry per event, `path` the path's index."""
    nee_free: list = field(default_factory=list)       # (path, (T * e) * f as 3 floats)
    nee_occluded: list = field(default_factory=list)   # (path, the material kind of what the shadow ray hit)
    nee_skipped: list = field(default_factory=list)    # path: c_s <= 0 or pe_s <= 0, no shadow ray
    escapes_weighted: list = field(default_factory=list)  # (path, f): an escape with pb not none
    escapes_plain: list = field(default_factory=list)  # path: an escape with pb none (f = 1)
    lambertian: set = field(default_factory=set)       # paths that scattered off a Lambertian at least once
    below: list = field(default_factory=list)          # path: of nee_skipped, c_s <= 0 (asked first)
    zero_pdf: list = field(default_factory=list)       # path: of nee_skipped, c_s > 0 and pe_s <= 0
    picks: list = field(default_factory=list)          # (path, row r, column k, (xi1..xi4), d_s as 3 floats) per sample


def ray_color(orc, scene, rays, states, max_depth, background, t_min, env, tb, crt=None, bvh=None):
    """crt_radiance_env_sampled_async's output for rays (n, 6) and LCG states (n,) uint32: (rgb (n, 3),
    how each path ended (env_model's MISS / LIGHT / ABSORBED / DEPTH), a Trace)."""
    if crt is None:
        import cpp_raytracer_amd as crt
    rays = np.array(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    T = np.ones((n, 3))
    rng = [int(s) for s in np.asarray(states, np.uint32).reshape(-1)]
    acc = np.zeros((n, 3))
    pb = np.zeros(n)
    has_pb = np.zeros(n, bool)
    ended = np.full(n, em.DEPTH, np.int64)
    tr = Trace()
    bg = [float(v) for v in background]
    if max_depth == 0:
        return acc, ended, tr

    def escape(idx):
        if len(idx) == 0:
            return
        e = em.lookup(env, d[idx], bg)
        f = np.ones(len(idx))
        hp = has_pb[idx]
        if hp.any():
            with np.errstate(all="ignore"):
                s = pdf(env, tb, d[idx][hp]) + pb[idx][hp]
                f[hp] = np.where(s > 0, pb[idx][hp] / np.where(s > 0, s, 1.0), 0.0)
        with np.errstate(all="ignore"):
            acc[idx] = acc[idx] + (T[idx] * e) * f[:, None]
        ended[idx] = em.MISS
        for i, w, h_ in zip(idx.tolist(), f.tolist(), hp.tolist()):
            if h_:
                tr.escapes_weighted.append((i, w))
            else:
                tr.escapes_plain.append(i)

    ok = em.traceable(rays)
    escape(np.flatnonzero(~ok))
    live = np.flatnonzero(ok)
    mat = scene.materials
    for depth_left in range(max_depth, 0, -1):
        if len(live) == 0:
            break
        h = orc.hits(scene, np.concatenate([o[live], d[live]], 1), t_min, **(bvh or {}))
        hit = h["prim"] >= 0
        escape(live[~hit])
        nxt, lam, lam_n, xi = [], [], [], []
        for j in np.flatnonzero(hit):
            i = int(live[j])
            mt = mat[int(h["material"][j])]
            kind = int(mt["kind"])
            color, param = [float(c) for c in mt["color"]], float(mt["param"])
            if kind == em.DIFFUSE_LIGHT:
                acc[i] = [acc[i, k] + T[i, k] * (color[k] * param) for k in range(3)]
                ended[i] = em.LIGHT
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
                has_pb[i] = False
                continue
            draws = []
            for _ in range(4):
                rng[i], x = crt.rand_double(rng[i], 0.0, 1.0)
                draws.append(x)
            lam.append(i)
            lam_n.append(nrm)
            xi.append(draws)
        if lam:
            lam = np.array(lam, np.int64)
            N = np.array(lam_n, np.float64)
            xi = np.array(xi, np.float64)
            ds = sample(env, tb, xi[:, 0], xi[:, 1], xi[:, 2], xi[:, 3])
            with np.errstate(all="ignore"):
                cs = dot(N, ds) / np.sqrt(dot(ds, ds))
                pbs = cs / PI
                pes = pdf(env, tb, ds)
                nd = d[lam]
                pb[lam] = (dot(N, nd) / np.sqrt(dot(nd, nd))) / PI
                has_pb[lam] = True
                go = (cs > 0) & (pes > 0)
            tr.nee_skipped.extend(lam[~go].tolist())
            tr.below.extend(lam[~(cs > 0)].tolist())
            tr.zero_pdf.extend(lam[(cs > 0) & ~(pes > 0)].tolist())
            tr.picks.extend(zip(lam.tolist(), *(a.tolist() for a in pick(env, tb, xi[:, 0], xi[:, 1])), map(tuple, xi.tolist()),
                                map(tuple, ds.tolist())))
            if go.any():
                s_i, s_d = lam[go], ds[go]
                with np.errstate(all="ignore"):
                    f = pbs[go] / (pes[go] + pbs[go])
                hs = orc.hits(scene, np.concatenate([o[s_i], s_d], 1), t_min, **(bvh or {}))
                free = hs["prim"] < 0
                kinds = mat["kind"][hs["material"][~free]]
                tr.nee_occluded.extend(zip(s_i[~free].tolist(), [int(k) for k in kinds]))
                if free.any():
                    fi = s_i[free]
                    e = em.lookup(env, s_d[free], bg)
                    with np.errstate(all="ignore"):
                        add = (T[fi] * e) * f[free][:, None]
                        acc[fi] = acc[fi] + add
                    tr.nee_free.extend(zip(fi.tolist(), add.tolist()))
        live = np.array(nxt, np.int64)
    return acc, ended, tr
