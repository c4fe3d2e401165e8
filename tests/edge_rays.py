"""One small world and six seeded ray families that sit ON the geometric decisions of the traversal,
for the ray-query and radiance-query tests (crt_trace_async, crt_radiance_async): what
tests/test_gpu_edge_rays.py sends through every route and switch, and what tests/test_edge_rays.py
checks, without a GPU, to be where it claims to be. Not a test module.

The world: 44 objects (59 primitives) in [-4, 4]^3, every coordinate a multiple of 1/8, all four
material kinds; 22 seeded spheres (3 hollow), 8 rotated and 6 axis-aligned parallelograms, 3 Boxes, and
four deliberate coincidences (world().coincidences): two spheres with one centre and radius, two overlapping
coplanar parallelograms, two Boxes sharing the plane x = -2.5, a parallelogram in a Box's top face.
The members of a coincidence carry different materials. TREES: the default BVH parameters and a deep
tree (num_buckets 8, max_prims_in_node 1: 113 nodes, the members of a coincidence in different
leaves unless their boxes are equal).

The families, 256 rays each, finite components, a non-zero direction, all meant for (1e-5, inf).
Each comes with a numpy restatement, in the reference's operation order, of the decision it targets
(numpy multiplies and adds without contraction, like the reference's build):

  T  sphere tangents: p = c + r n, unit tangent u, origin p - s u + n (r k 2^-52), s in [1, 10],
     direction u f, f in [0.5, 2], k of K_T (0 twice: one of the two with n and u on the axes and
     dyadic s and f, where every operation is exact and discriminant_quarter is 0). The decision:
     discriminant_quarter < 0 (sphere.h).
  R  sphere roots at t_min: the origin 1e-5 f0 before a surface point along a direction that enters
     (outside, the smaller root near t_min: 112 rays) or leaves (inside, the larger root near t_min:
     112 rays); the direction's length is then bisected until the computed root crosses 1e-5 and
     moved a few ulps, to either side. 32 more rays start on / k 2^-52 r off the surface. The
     decision: t_min < root.
  Q  parallelogram edges and corners: aimed at vertex + a side1 + b side2 with a, or b, or both in
     {0, 1} + k 2^-52, k of K, the other in [0.1, 0.9]. The decision: 0 <= alpha, beta <= 1.
  P  near-parallel: d = u + n e, u a unit vector of the plane (for the axis-aligned ones an axis,
     so that dot(n, d) = e exactly), e = +-1e-9 times P_FACTORS. The decision: |dot(n, d)| < 1e-9.
  C  coincidences: 64 rays through each, from both sides, in all eight sign octants; every 9th has
     -0.0 on the split axis of the deep tree's node above the pair. The decision: which of two
     primitives with bit-equal hit times is visited first.
  N  node-box edges, the deep tree's boxes from export_bvh() of the host build: (i) 96 rays with an
     origin component exactly on a node's slab plane and that direction component +0.0 or -0.0, the
     other two aimed at a primitive of the node: 0 * inf, a NaN slab value; (ii) 64 through corners
     and edge points of node boxes exactly; (iii) 48 lying in a face plane; (iv) 48 with -0.0
     components and the origin off every plane. The decision: AABB::is_hit_by_optimized's selects.
  all  every family, concatenated and permuted with a fixed seed.

WORLDS: the whole world, and its spheres / its parallelograms and Boxes / its axis-aligned
parallelograms and Boxes alone, which is where the render kernel's f32 leaf filters run. A part keeps
the objects' order, so its primitives' numbers are its own; a family's rays are the same in every
world, and so is the decision they target (a primitive's own test), while what else they hit differs.

MEASURED holds the shares found when the families were chosen; tests/test_edge_rays.py recomputes
them, holds them to the floors and to MEASURED within 0.01."""
import numpy as np

import ray_sets as rs
from oracle import crt_oracle_py as orc

SEED = 4100
N = 256
T_MIN = 1e-5
EPS = 2.0 ** -52
K = (0, 1, -1, 4, -4, 16, -16)
K_T = (0, 0, 1, -1, 4, -4, 16, -16)
P_FACTORS = (1 - 2.0 ** -30, 1 - 2.0 ** -50, 1.0, 1 + 2.0 ** -50, 1 + 2.0 ** -30)
FAMILIES = "TRQPCN"
TREES = {"default": {}, "deep": {"num_buckets": 8, "max_prims_in_node": 1}}
# The leaf filters run only where a scene has one kind of primitive (crt_device.hip: the packed f32
# sphere filter in a sphere-only scene, the generic f32 parallelogram filter in a parallelogram-only
# one, the flat-box filter where every parallelogram is axis-aligned), so the same rays also go
# through three parts of the world: world -> the families made for primitives it keeps (and `all`).
WORLDS = {"full": "TRQPCN", "spheres": "TRC", "quads": "QPC", "flat": "QPC"}
# Three distinct channels, none of them a material's. Every colour, the light's intensity and the
# background are multiples of 1/8: at depth RADIANCE_DEPTH every product and sum of ray_color is exact
# in float64 however it is associated, so a radiance query is held to the oracle's bits.
BG = (0.375, 0.625, 1.25)
N_PARTS = (96, 64, 48, 48)  # N (i) .. (iv)
R_PARTS = (112, 112, 32)

# family -> what shares() gave when the families were chosen. T: the targeted sphere's test accepts /
# rejects, discriminant_quarter == 0. R: t_min < the targeted root or not, that root within 16 ulps of
# t_min (all but the 32 rays that start on the surface). Q: alpha and beta inside [0, 1] or not.
# P: past the 1e-9 cutoff or cut by it. C: rays on which the pair's two hit times are bit-equal.
# N: rays with a NaN slab value at some node of the default / the deep tree, of all and of part (i);
# hits of part (i). hit: the oracle's hits through the default tree.
MEASURED = {
    "T": dict(accepted=0.695, rejected=0.305, zero=0.379, hit=0.82),
    "R": dict(above=0.438, not_above=0.562, within_16_ulps=0.875, hit=0.82),
    "Q": dict(inside=0.48, outside=0.52, hit=0.898),
    "P": dict(kept=0.59, cut=0.41, hit=0.727),
    "C": dict(ties=256, hit=0.891),
    "N": dict(nan_default=0.195, nan_deep=0.562, nan_i_default=0.354, nan_i_deep=1.0, hit_i=0.385, hit=0.32),
}


# ---- the reference's arithmetic, in numpy ----------------------------------------------------------
def dot(a, b):  # vec3d.h:114
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):  # vec3d.h:116
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def unit(a):  # vec3d.h:127: a * (1 / mag)
    return a * (1 / np.sqrt(dot(a, a)))[..., None]


def sphere_terms(o, d, c, r):
    """Sphere::hit_by (sphere.h:45-96): discriminant_quarter, the smaller and the larger root."""
    oc = o - c
    a, b = dot(d, d), dot(d, oc)
    cc = dot(oc, oc) - r * r
    disc = b * b - a * cc
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
    return disc, (-b - sq) / a, (-b + sq) / a


def sphere_hit(o, d, c, r, t_min=T_MIN, t_max=np.inf):
    disc, r1, r2 = sphere_terms(o, d, c, r)
    first = (t_min < r1) & (r1 < t_max)
    second = (t_min < r2) & (r2 < t_max)
    hit = (disc >= 0) & (first | second)
    return hit, np.where(first, r1, r2)


def quad_consts(v, s1, s2):  # parallelogram.h:269-296
    n = cross(s1, s2)
    return unit(n), n * (1 / dot(n, n))[..., None]


def quad_terms(o, d, v, s1, s2):
    """Parallelogram::hit_by (parallelogram.h:177-240): dot(unit_normal, d), the hit time, alpha, beta."""
    n, sn = quad_consts(v, s1, s2)
    den = dot(n, d)
    with np.errstate(all="ignore"):
        t = dot(n, v - o) / den
        p = o + d * t[..., None]
        w = p - v
        alpha, beta = dot(sn, cross(w, s2)), dot(sn, cross(s1, w))
    return den, t, alpha, beta


def quad_hit(o, d, v, s1, s2, t_min=T_MIN, t_max=np.inf):
    den, t, alpha, beta = quad_terms(o, d, v, s1, s2)
    with np.errstate(invalid="ignore"):
        hit = ~(np.abs(den) < 1e-9) & (t_min < t) & (t < t_max) & (0 <= alpha) & (alpha <= 1) & (0 <= beta) & (beta <= 1)
    return hit, t


def slab_values(bounds, rays):
    """AABB::is_hit_by_optimized's six slab values (aabb.h:141-159) of every ray at every node:
    (rays, nodes, 3) near and far times."""
    o, d = rays[:, None, :3], rays[:, None, 3:]
    with np.errstate(all="ignore"):
        inv = 1 / d
        neg = d < 0
        lo, hi = bounds[None, :, 0::2], bounds[None, :, 1::2]
        return (np.where(neg, hi, lo) - o) * inv, (np.where(neg, lo, hi) - o) * inv


def nan_slab(bounds, rays):
    near, far = slab_values(bounds, rays)
    return (np.isnan(near) | np.isnan(far)).any((1, 2))


def ulps(a, b):
    """|a - b| in units of b's spacing."""
    return np.abs(a - b) / np.spacing(b)


# ---- the world --------------------------------------------------------------------------------------
def world_data(crt):
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE, camera_with
    from cpp_raytracer_amd._capi import D3
    rng = np.random.default_rng(SEED)
    mats = np.zeros(5, MATERIAL_DTYPE)
    mats["kind"] = [1, 2, 3, 4, 1]
    mats["color"] = [[0.75, 0.25, 0.125], [0.875, 0.875, 0.75], [0.0, 0.0, 0.0], [1.0, 0.875, 0.75], [0.25, 0.625, 0.375]]
    mats["param"] = [0.0, 0.25, 1.5, 4.0, 0.0]
    objs = []

    def obj(kind, v, mat=None):
        o = np.zeros(1, OBJECT_DTYPE)[0]
        o["kind"], o["material"] = kind, len(objs) % 5 if mat is None else mat
        o["v"][:len(v)] = v
        objs.append(o)
        return len(objs) - 1

    for i in range(22):
        r = rng.integers(4, 9) / 8 * (-1 if i % 8 == 7 else 1)  # a few hollow ones
        obj(1, [*(rng.integers(-24, 25, 3) / 8), r])
    pair_s = (obj(1, [-3.0, 3.0, 3.0, 0.75], 0), obj(1, [-3.0, 3.0, 3.0, 0.75], 1))
    while len(objs) < 32:  # rotated parallelograms
        s1, s2 = rng.integers(-8, 9, 3) / 8, rng.integers(-8, 9, 3) / 8
        n = np.cross(s1, s2)
        if (n * n).sum() < 0.25 or (n == 0).sum() >= 2:
            continue
        obj(2, [*(rng.integers(-16, 17, 3) / 8), *s1, *s2])
    for _ in range(6):  # axis-aligned parallelograms
        ax = rng.permutation(3)
        s1, s2 = np.zeros(3), np.zeros(3)
        s1[ax[0]] = rng.integers(8, 17) / 8 * rng.choice([-1, 1])
        s2[ax[1]] = rng.integers(8, 17) / 8 * rng.choice([-1, 1])
        obj(2, [*(rng.integers(-16, 17, 3) / 8), *s1, *s2])
    pair_q = (obj(2, [-1.0, -1.0, 3.5, 2.0, 0, 0, 0, 2.0, 0], 0), obj(2, [0.0, 0.0, 3.5, 2.0, 0, 0, 0, 2.0, 0], 1))
    in_face = obj(2, [2.125, -3.0, 1.125, 1.0, 0, 0, 0, 0, 1.0], 3)  # off the face's centre
    first_box = len(objs)
    obj(3, [-4.0, -4.0, -4.0, -2.5, -2.5, -2.5], 2)
    obj(3, [-2.5, -4.0, -4.0, -1.0, -3.0, -3.0], 4)
    obj(3, [2.0, -4.0, 1.0, 3.5, -3.0, 2.5], 0)
    objs = np.array(objs, dtype=OBJECT_DTYPE)
    assert len(objs) == 44 and np.abs(objs["v"]).max() <= 4 and np.array_equal(objs["v"] * 8, np.round(objs["v"] * 8))
    d = crt.SceneData.named("config1")
    d.materials, d.objects = mats, objs
    d.camera = camera_with(d.camera, image_w=24, image_h=16, samples_per_pixel=1, max_depth=6,
                           center=D3(0.0, 0.0, 12.0), lookat=D3(0.0, 0.0, 0.0), has_lookat=1, up=D3(0.0, 1.0, 0.0),
                           fov=float(np.deg2rad(40.0)), fov_is_vertical=1, defocus_angle=0.0, background=D3(*BG))
    box = lambda j, face: first_box + 6 * j + face  # noqa: E731  (a Box's faces: flatten()'s order)
    # name -> (primitive a, primitive b, the axis of the shared plane's normal or None)
    coincidences = {"spheres": (*pair_s, None), "coplanar": (*pair_q, 2),
                    "box_faces": (box(0, 5), box(1, 2), 0), "in_face": (in_face, box(2, 4), 1)}
    return d, coincidences


def primitives(d):
    """Scene::get_primitive_components' order: a list of ("s", c, r, material) / ("q", v, s1, s2, material)."""
    out = []
    for o in d.objects:
        v, m = np.array(o["v"], np.float64), int(o["material"])
        if o["kind"] == 1:
            out.append(("s", v[:3], v[3], m))
        elif o["kind"] == 2:
            out.append(("q", v[:3], v[3:6], v[6:9], m))
        else:
            mn, mx = np.minimum(v[:3], v[3:6]), np.maximum(v[:3], v[3:6])
            sx, sy, sz = (np.array([mx[0] - mn[0], 0, 0]), np.array([0, mx[1] - mn[1], 0]), np.array([0, 0, mx[2] - mn[2]]))
            for a, b, c in ((mn, sx, sy), (mn, sx, sz), (mn, sy, sz), (mx, -sx, -sy), (mx, -sx, -sz), (mx, -sy, -sz)):
                out.append(("q", a, b, c, m))
    return out


def prim_hit(p, rays, t_min=T_MIN, t_max=np.inf):
    o, d = rays[:, :3], rays[:, 3:]
    return sphere_hit(o, d, p[1], p[2], t_min, t_max) if p[0] == "s" else quad_hit(o, d, p[1], p[2], p[3], t_min, t_max)


def centre(p):
    return p[1] if p[0] == "s" else p[1] + (p[2] + p[3]) / 2


def unit_vectors(rng, n):
    return unit(rng.normal(size=(n, 3)))


# ---- tree helpers (export_bvh's preorder nodes) -----------------------------------------------------
def subtree_slots(nodes, i):
    if nodes[i]["count"] > 0:
        return list(range(int(nodes[i]["index"]), int(nodes[i]["index"]) + int(nodes[i]["count"])))
    return subtree_slots(nodes, i + 1) + subtree_slots(nodes, int(nodes[i]["index"]))


def node_above(nodes, order, a, b):
    """The lowest node whose subtree holds primitives a and b."""
    i = 0
    while nodes[i]["count"] == 0:
        for child in (i + 1, int(nodes[i]["index"])):
            held = {int(order[s]) for s in subtree_slots(nodes, child)}
            if a in held and b in held:
                i = child
                break
        else:
            return i
    return i


# ---- the families -----------------------------------------------------------------------------------
def family_t(prims):
    rng = np.random.default_rng(SEED + 1)
    sph = [p for p in prims if p[0] == "s"]
    i = np.arange(N)
    k = np.array(K_T)[i % 8]
    which = (i // 8) % len(sph)
    c, r = np.array([sph[j][1] for j in which]), np.array([sph[j][2] for j in which])
    n = unit_vectors(rng, N)
    u = unit(cross(n, unit_vectors(rng, N)))
    s, f = rng.uniform(1, 10, N), rng.uniform(0.5, 2, N)
    exact = i % 8 == 0  # axis frames, dyadic lengths: every operation of the test is exact
    ax = rng.integers(0, 3, N)
    e = np.eye(3)
    n[exact] = (e[ax] * rng.choice([-1.0, 1.0], N)[:, None])[exact]
    u[exact] = (e[(ax + 1 + rng.integers(0, 2, N)) % 3] * rng.choice([-1.0, 1.0], N)[:, None])[exact]
    s[exact] = (rng.integers(8, 81, N) / 8)[exact]
    f[exact] = rng.choice([0.5, 1.0, 2.0], N)[exact]
    p = c + n * r[:, None]
    o = (p - u * s[:, None]) + n * (r * k * EPS)[:, None]
    return np.concatenate([o, u * f[:, None]], 1), dict(c=c, r=r, k=k)


def family_r(prims):
    rng = np.random.default_rng(SEED + 2)
    sph = [p for p in prims if p[0] == "s"]
    i = np.arange(N)
    which = i % len(sph)
    c, r = np.array([sph[j][1] for j in which]), np.array([sph[j][2] for j in which])
    g = unit_vectors(rng, N)  # the geometric outward normal at the surface point
    p = c + g * np.abs(r)[:, None]
    dh = unit_vectors(rng, N)
    for _ in range(64):  # clear of grazing: |dot| > 0.3
        bad = np.abs(dot(dh, g)) < 0.3
        dh[bad] = unit_vectors(rng, N)[bad]
    inward = np.concatenate([np.ones(R_PARTS[0], bool), np.zeros(R_PARTS[1], bool), i[:R_PARTS[2]] % 2 == 0])
    dh[(dot(dh, g) > 0) == inward] *= -1
    f0 = rng.uniform(0.5, 2, N)
    o = p - dh * (T_MIN * f0)[:, None]

    def root(f):  # the root next to the surface point: the smaller one entering, the larger one leaving
        _, r1, r2 = sphere_terms(o, dh * f[:, None], c, r)
        return np.where(inward, r1, r2)

    lo, hi = f0 * (1 - 1e-6), f0 * (1 + 1e-6)  # the root falls as the direction grows
    assert (root(lo) > T_MIN).all() and (root(hi) < T_MIN).all()
    for _ in range(64):
        mid = lo + (hi - lo) / 2
        above = root(mid) > T_MIN
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    # -b -+ sqrt(...) cancels: the computed root is m g / a for an integer m and the spacing g of b, some
    # 10^4 ulps of t_min a step, and m flickers between neighbouring directions. With m held, the root
    # goes as 1 / f^2: step to where this m's root is t_min, look at the 17 lengths around, repeat.
    steps = np.arange(-8, 9)
    f, cands, vals = lo, [], []
    for _ in range(8):
        cand = f[:, None] * (1 + steps[None, :] * EPS)
        val = np.stack([root(cand[:, j]) for j in range(len(steps))], 1)
        cands.append(cand)
        vals.append(val)
        col = rng.integers(0, len(steps), N)
        f = cand[i, col] * np.sqrt(val[i, col] / T_MIN)
    cand, val = np.concatenate(cands, 1), np.concatenate(vals, 1)
    near = ulps(val, T_MIN) <= 16
    wanted = near & ((val > T_MIN) == (i % 2 == 0)[:, None])
    use = np.where(wanted.any(1)[:, None], wanted, near)
    assert use.any(1).all()
    pick = np.array([rng.choice(np.flatnonzero(row)) for row in use])
    f = cand[i, pick]
    rays = np.concatenate([o, dh * f[:, None]], 1)
    # the last part: origins on the surface point itself and k 2^-52 r off it, any length
    tail = i >= R_PARTS[0] + R_PARTS[1]
    k = np.array(K)[i % 7]
    rays[tail, :3] = (p + g * (np.abs(r) * k * EPS)[:, None])[tail]
    rays[tail, 3:] = (dh * f0[:, None])[tail]
    return rays, dict(c=c, r=r, inward=inward, tail=tail)


def standalone_quads(d, prims):
    return [p for o, p in zip(d.objects, prims[:int((d.objects["kind"] != 3).sum())]) if o["kind"] == 2]


def family_q(quads):
    rng = np.random.default_rng(SEED + 3)
    i = np.arange(N)
    q = [quads[j] for j in i % len(quads)]
    v, s1, s2 = (np.array([x[m] for x in q]) for m in (1, 2, 3))
    k = np.array(K)[rng.integers(0, 7, N)]
    mode = (i // len(quads)) % 3  # a on an edge, b on an edge, a corner
    edge = lambda: rng.integers(0, 2, N) + k * EPS  # noqa: E731
    a = np.where(mode != 1, edge(), rng.uniform(0.1, 0.9, N))
    b = np.where(mode != 0, edge(), rng.uniform(0.1, 0.9, N))
    target = (v + s1 * a[:, None]) + s2 * b[:, None]
    n, _ = quad_consts(v, s1, s2)
    o = target + n * (rng.choice([-1.0, 1.0], N) * rng.uniform(1, 4, N))[:, None] \
        + s1 * rng.uniform(-0.5, 0.5, N)[:, None] + s2 * rng.uniform(-0.5, 0.5, N)[:, None]
    dd = (target - o) * rng.uniform(0.5, 2, N)[:, None]
    return np.concatenate([o, dd], 1), dict(v=v, s1=s1, s2=s2)


def family_p(quads):
    rng = np.random.default_rng(SEED + 4)
    i = np.arange(N)
    q = [quads[j] for j in i % len(quads)]
    v, s1, s2 = (np.array([x[m] for x in q]) for m in (1, 2, 3))
    n, _ = quad_consts(v, s1, s2)
    u = unit(s1 * rng.uniform(-1, 1, N)[:, None] + s2 * rng.uniform(-1, 1, N)[:, None])
    flat = ((s1 != 0).sum(1) == 1) & ((s2 != 0).sum(1) == 1)  # axis-aligned: u an axis, n an axis, exactly
    along = np.where((rng.integers(0, 2, N) == 0)[:, None], s1, s2)
    u[flat] = (np.sign(along) * rng.choice([-1.0, 1.0], N)[:, None])[flat]
    e = rng.choice([-1.0, 1.0], N) * 1e-9 * np.array(P_FACTORS)[(i // len(quads)) % 5]
    dd = u + n * e[:, None]
    target = (v + s1 * rng.uniform(0.3, 0.7, N)[:, None]) + s2 * rng.uniform(0.3, 0.7, N)[:, None]
    o = target - dd * rng.uniform(1, 3, N)[:, None]
    return np.concatenate([o, dd], 1), dict(v=v, s1=s1, s2=s2, exact=flat)


def family_c(prims, coincidences, nodes, order):
    rng = np.random.default_rng(SEED + 5)
    rays, pair = [], []
    signs = np.array([[1 if o & 1 else -1, 1 if o & 2 else -1, 1 if o & 4 else -1] for o in range(8)], np.float64)
    for name, (a, b, axis) in coincidences.items():
        split = int(nodes[node_above(nodes, order, a, b)]["axis"])
        for j in range(64):
            dd = signs[j % 8] * rng.uniform(0.2, 1.0, 3)
            if j % 9 == 3 and split != axis:
                dd[split] = -0.0
            if axis is None:  # through the spheres, off their centre
                target = prims[a][1] + rng.uniform(-0.3, 0.3, 3)
                t0 = rng.uniform(1.5, 2.5) / np.sqrt((dd * dd).sum())
            else:  # a point of the region both parallelograms cover
                lo = np.maximum(*(np.minimum(np.minimum(p[1], p[1] + p[2]), np.minimum(p[1] + p[3], p[1] + p[2] + p[3]))
                                  for p in (prims[a], prims[b])))
                hi = np.minimum(*(np.maximum(np.maximum(p[1], p[1] + p[2]), np.maximum(p[1] + p[3], p[1] + p[2] + p[3]))
                                  for p in (prims[a], prims[b])))
                target = lo + rng.uniform(0.1, 0.9, 3) * (hi - lo)
                t0 = rng.uniform(0.05, 0.1)  # from inside the Boxes: no other face in between
            rays.append(np.concatenate([target - dd * t0, dd]))
            pair.append((a, b))
    return np.array(rays), dict(pair=np.array(pair))


def family_n(prims, nodes, order):
    rng = np.random.default_rng(SEED + 6)
    bounds = nodes["bounds"]
    rays = []
    first = [int(order[subtree_slots(nodes, j)[0]]) for j in range(len(nodes))]
    for i in range(N_PARTS[0]):  # (i) on a slab plane, that component +-0, aimed at a primitive of the node
        j = (7 * i + 1) % len(nodes)
        k, side = i % 3, (i // 3) % 2
        target = centre(prims[first[j]]).copy()
        target[k] = bounds[j, 2 * k + side]
        if i % 4 == 3:  # beside it
            target += rng.uniform(-1.5, 1.5, 3)
            target[k] = bounds[j, 2 * k + side]
        dd = rng.normal(size=3)
        dd[k] = 0.0 if (i // 6) % 2 == 0 else -0.0
        o = target - dd * rng.uniform(1, 3)
        o[k] = bounds[j, 2 * k + side]
        rays.append(np.concatenate([o, dd]))
    for i in range(N_PARTS[1]):  # (ii) through a corner (even i) or an edge point (odd i), exactly
        j = (5 * i + 2) % len(nodes)
        pick = rng.integers(0, 2, 3)
        pt = bounds[j, 2 * np.arange(3) + pick].copy()
        if i % 2:
            k = i // 2 % 3
            lo, hi = bounds[j, 2 * k], bounds[j, 2 * k + 1]
            pt[k] = np.clip(np.round((lo + (hi - lo) * rng.uniform(0.2, 0.8)) * 8) / 8, lo, hi)
        dd = rng.integers(1, 9, 3) / 8 * rng.choice([-1.0, 1.0], 3)
        rays.append(np.concatenate([pt - dd * rng.choice([1.0, 2.0, 4.0]), dd]))
    for i in range(N_PARTS[2]):  # (iii) lying in a face plane
        j = (11 * i + 3) % len(nodes)
        k, side = i % 3, (i // 3) % 2
        lo, hi = bounds[j, 0::2], bounds[j, 1::2]
        pt = lo + rng.uniform(0, 1, 3) * (hi - lo)
        dd = rng.normal(size=3)
        dd[k] = 0.0 if i % 2 == 0 else -0.0
        o = pt - dd * rng.uniform(1, 3)
        o[k] = bounds[j, 2 * k + side]
        rays.append(np.concatenate([o, dd]))
    for i in range(N_PARTS[3]):  # (iv) -0.0 components, the origin off every plane
        target = centre(prims[i % len(prims)])
        o = target + rng.uniform(-5, 5, 3)
        k = i % 3
        o[k] = target[k] + rng.uniform(-0.3, 0.3)
        dd = target - o
        dd[k] = -0.0
        if i % 5 == 0:
            k2 = (k + 1) % 3
            o[k2] = target[k2] + rng.uniform(-0.3, 0.3)
            dd[k2] = -0.0
        rays.append(np.concatenate([o, dd]))
    rays = np.array(rays)
    part = np.repeat(np.arange(4), N_PARTS)
    return rays, dict(part=part)


class World:
    pass


_WORLD = None


def world(crt):
    """The world (SceneData), its coincidences, both trees' nodes, every family's rays and the
    constants of its restatement, the `all` set: computed once and left unchanged."""
    global _WORLD
    if _WORLD is None:
        w = World()
        w.d, w.coincidences = world_data(crt)
        w.prims = primitives(w.d)
        kind, v = w.d.objects["kind"], w.d.objects["v"]
        aligned = (kind == 3) | ((kind == 2) & ((v[:, 3:6] != 0).sum(1) == 1) & ((v[:, 6:9] != 0).sum(1) == 1))
        w.data = {"full": w.d}
        for name, keep in (("spheres", kind == 1), ("quads", kind != 1), ("flat", aligned)):
            part = crt.SceneData.named("config1")
            part.materials, part.objects, part.camera = w.d.materials, w.d.objects[keep].copy(), w.d.camera
            w.data[name] = part
        w.trees = {name: crt.GpuScene(w.d, **kw).export_bvh() for name, kw in TREES.items()}
        nodes, order = w.trees["deep"]
        quads = standalone_quads(w.d, w.prims)
        made = {"T": family_t(w.prims), "R": family_r(w.prims), "Q": family_q(quads), "P": family_p(quads),
                "C": family_c(w.prims, w.coincidences, nodes, order), "N": family_n(w.prims, nodes, order)}
        w.rays = {k: np.ascontiguousarray(v[0]) for k, v in made.items()}
        w.info = {k: v[1] for k, v in made.items()}
        perm = np.random.default_rng(SEED + 7).permutation(N * len(FAMILIES))
        w.rays["all"] = np.concatenate([w.rays[k] for k in FAMILIES])[perm]
        w.perm = perm
        for r in w.rays.values():
            assert r.shape[1] == 6 and len(r) <= 512 * 6 and np.isfinite(r).all() and (r[:, 3:] != 0).any(1).all()
            r.setflags(write=False)
        _WORLD = w
    return _WORLD


_WANT, _RADIANCE = {}, {}


def want(crt, tree, key, part="full"):
    """The oracle's records of a family (or "all") over (1e-5, inf) through a tree of TREES of a
    world of WORLDS, once."""
    if (tree, key, part) not in _WANT:
        w = world(crt)
        kw = TREES[tree]
        h = orc.hits(w.data[part], w.rays[key], T_MIN, np.inf, kw.get("num_buckets", 32), kw.get("max_prims_in_node", 12))
        h.setflags(write=False)
        _WANT[tree, key, part] = h
    return _WANT[tree, key, part]


def call(crt, key):
    return rs.Call(world(crt).rays[key].copy(), t_min=T_MIN)  # a writable copy: the GPU harness wraps it in a tensor


def states(base, n):
    """crt_sample_seed(base, i, 0), as the oracle computes it."""
    return np.array([orc.sample_seed(base, i, 0) for i in range(n)], np.uint32)


RADIANCE_BASE, RADIANCE_DEPTH = 977, 6


def want_radiance(crt, tree, key, part="full"):
    if (tree, key, part) not in _RADIANCE:
        w = world(crt)
        kw = TREES[tree]
        r = orc.radiance(w.data[part], w.rays[key], states(RADIANCE_BASE, len(w.rays[key])), RADIANCE_DEPTH, BG, T_MIN,
                         num_buckets=kw.get("num_buckets", 32), max_prims=kw.get("max_prims_in_node", 12))
        r.setflags(write=False)
        _RADIANCE[tree, key, part] = r
    return _RADIANCE[tree, key, part]


# ---- what each family is, by its restatement ---------------------------------------------------------
def targeted(crt):
    """family -> the arrays the CPU checks count: the targeted decision of every ray."""
    w = world(crt)
    out = {}
    r, i = w.rays["T"], w.info["T"]
    disc, _, _ = sphere_terms(r[:, :3], r[:, 3:], i["c"], i["r"])
    out["T"] = dict(accepted=sphere_hit(r[:, :3], r[:, 3:], i["c"], i["r"])[0], disc=disc, k=i["k"])
    r, i = w.rays["R"], w.info["R"]
    _, r1, r2 = sphere_terms(r[:, :3], r[:, 3:], i["c"], i["r"])
    root = np.where(i["inward"], r1, r2)
    out["R"] = dict(above=T_MIN < root, root=root, tail=i["tail"], inward=i["inward"])
    r, i = w.rays["Q"], w.info["Q"]
    den, t, alpha, beta = quad_terms(r[:, :3], r[:, 3:], i["v"], i["s1"], i["s2"])
    out["Q"] = dict(inside=(0 <= alpha) & (alpha <= 1) & (0 <= beta) & (beta <= 1), alpha=alpha, beta=beta,
                    reached=~(np.abs(den) < 1e-9) & (T_MIN < t))
    r, i = w.rays["P"], w.info["P"]
    den, _, _, _ = quad_terms(r[:, :3], r[:, 3:], i["v"], i["s1"], i["s2"])
    out["P"] = dict(cut=np.abs(den) < 1e-9, den=den, exact=i["exact"])
    r, i = w.rays["C"], w.info["C"]
    tie = np.zeros(len(r), bool)
    t_tie = np.full(len(r), np.nan)
    for a, b in sorted({tuple(p) for p in i["pair"].tolist()}):
        sel = (i["pair"] == (a, b)).all(1)
        (ha, ta), (hb, tb) = prim_hit(w.prims[a], r[sel]), prim_hit(w.prims[b], r[sel])
        both = ha & hb & (ta.view(np.uint64) == tb.view(np.uint64))
        tie[sel] = both
        t_tie[sel] = np.where(both, ta, np.nan)
    out["C"] = dict(tie=tie, t=t_tie, pair=i["pair"])
    r, i = w.rays["N"], w.info["N"]
    out["N"] = dict(part=i["part"], **{"nan_" + name: nan_slab(w.trees[name][0]["bounds"], r) for name in TREES})
    return out


def shares(crt):
    """The table MEASURED records."""
    t = targeted(crt)
    hit = {k: float((want(crt, "default", k)["prim"] >= 0).mean()) for k in FAMILIES}
    first = t["N"]["part"] == 0
    got = {
        "T": dict(accepted=t["T"]["accepted"].mean(), rejected=(~t["T"]["accepted"]).mean(), zero=(t["T"]["disc"] == 0).mean()),
        "R": dict(above=t["R"]["above"].mean(), not_above=(~t["R"]["above"]).mean(),
                  within_16_ulps=(ulps(t["R"]["root"], T_MIN) <= 16).mean()),
        "Q": dict(inside=t["Q"]["inside"].mean(), outside=(~t["Q"]["inside"]).mean()),
        "P": dict(kept=(~t["P"]["cut"]).mean(), cut=t["P"]["cut"].mean()),
        "C": dict(ties=int(t["C"]["tie"].sum())),
        "N": dict(nan_default=t["N"]["nan_default"].mean(), nan_deep=t["N"]["nan_deep"].mean(),
                  nan_i_default=t["N"]["nan_default"][first].mean(), nan_i_deep=t["N"]["nan_deep"][first].mean(),
                  hit_i=(want(crt, "default", "N")["prim"][first] >= 0).mean()),
    }
    for k in FAMILIES:
        got[k]["hit"] = hit[k]
        got[k] = {n: (v if isinstance(v, int) else round(float(v), 3)) for n, v in got[k].items()}
    return got
