"""Truth for the sampling of a scene's own lights that is no restatement of the kernel: closed-form
irradiance factors written from the geometry alone, a quadrature that checks them, the worlds they hold
in, worlds for the estimator's edge events, and LCG states crafted to reach draws of exactly 0 and above
1. tests/test_light_truth.py uses it without a GPU, tests/test_gpu_light_truth.py and
tests/test_gpu_light_nee_edges.py on one. Not a test module. Nothing here comes from light_nee_model.

A Lambertian floor point o with normal n under a diffuse light of radiance Le sends back, per channel,
rho * Le * F with F = (1 / pi) * integral of cos(theta) over the solid angle the light fills (its form
factor): the estimator's mean at depth 2, whatever its sampling and weights, if it is unbiased.

  sphere_factor    (r / d)^2 * cos(angle to the centre), the whole sphere above the horizon
  polygon_factor   Lambert's formula over the edges of a polygon that is whole above the horizon
  box_factor       polygon_factor summed over the faces whose plane faces o
  quadrature_*     midpoint quadrature of cos * cos' / (pi * dist^2) over the visible surface

Every world is SceneData.named("config1") with materials and objects replaced (light_cases does the
same). CLOSED worlds have a closed form (World.factors), OPEN ones do not, EDGE ones exist for events.
A World's query is one ray, `ray`, repeated; its floor point is `o` and the normal there `n`.
"""
import math
from dataclasses import dataclass, field

import numpy as np

RHO = (0.5, 0.6, 0.7)
COLOR, PARAM = (1.0, 0.75, 0.5), 4.0   # Le = (4, 3, 2)
LE = tuple(c * PARAM for c in COLOR)
MATE_COLOR, MATE_PARAM = (1.0, -2.0, 0.5), 3.0  # luminance below 0: weight 0, but it emits
FLOOR = (-50.0, 0.0, -50.0, 100.0, 0.0, 0.0, 0.0, 0.0, 100.0)
GROUND_SPHERE = (0.0, -1000.0, 0.0, 1000.0)  # the floor of the all-sphere variants: y = 0 at the origin
LAMBERTIAN, DIELECTRIC, LIGHT = 1, 3, 4
T_MIN = 1e-5
BG = (0.0, 0.0, 0.0)


# ---- closed forms -------------------------------------------------------------------------------------
def _a(x):
    return np.asarray(x, np.float64)


def sphere_factor(c, r, o, n):
    c, o, n = _a(c), _a(o), _a(n)
    to = c - o
    d = math.sqrt(float(to @ to))
    h = float(to @ n)
    assert abs(float(n @ n) - 1) < 1e-12 and h >= abs(r) and d > abs(r), "the whole sphere must be above the horizon"
    return (r / d) ** 2 * h / d


def polygon_factor(vertices, o, n):
    v, o, n = _a(vertices), _a(o), _a(n)
    R = v - o
    assert abs(float(n @ n) - 1) < 1e-12 and (R @ n > 0).all(), "the whole polygon must be above the horizon"
    R = R / np.sqrt((R * R).sum(1))[:, None]
    total = 0.0
    for i in range(len(R)):
        a, b = R[i], R[(i + 1) % len(R)]
        cr = np.cross(a, b)
        s = math.sqrt(float(cr @ cr))
        gamma = math.atan2(s, float(a @ b))
        total += gamma * float((cr / s) @ n)
    return abs(total) / (2 * math.pi)


def quad_vertices(v, s1, s2):
    v, s1, s2 = _a(v), _a(s1), _a(s2)
    return np.array([v, v + s1, v + s1 + s2, v + s2])


def box_faces(lo, hi):
    """The six faces of an axis-aligned box as (vertices (4, 3), outward unit normal)."""
    lo, hi = _a(lo), _a(hi)
    out = []
    for ax in range(3):
        b, c = [k for k in range(3) if k != ax]
        for side, sign in ((lo, -1.0), (hi, 1.0)):
            p = lo.copy()
            p[ax] = side[ax]
            e1, e2 = np.zeros(3), np.zeros(3)
            e1[b], e2[c] = hi[b] - lo[b], hi[c] - lo[c]
            nrm = np.zeros(3)
            nrm[ax] = sign
            out.append((np.array([p, p + e1, p + e1 + e2, p + e2]), nrm))
    return out


def box_factor(lo, hi, o, n):
    o = _a(o)
    return sum(polygon_factor(vs, o, n) for vs, nrm in box_faces(lo, hi) if float((o - vs[0]) @ nrm) > 0)


# ---- quadrature ---------------------------------------------------------------------------------------
def _integrand(p, nl, o, n):
    """cos * cos' / (pi * dist^2) at surface points p (m, 3) with unit normals nl, 0 where the point is
    below o's horizon."""
    w = p - o
    d2 = (w * w).sum(1)
    d = np.sqrt(d2)
    c = (w @ n) / d
    cl = np.abs((w * nl).sum(1)) / d
    return np.where(c > 0, c * cl / (math.pi * d2), 0.0)


def quadrature_quad(v, s1, s2, o, n, g=512):
    v, s1, s2, o, n = _a(v), _a(s1), _a(s2), _a(o), _a(n)
    cr = np.cross(s1, s2)
    A = math.sqrt(float(cr @ cr))
    t = (np.arange(g) + 0.5) / g
    a, b = (x.reshape(-1) for x in np.meshgrid(t, t, indexing="ij"))
    p = v[None, :] + a[:, None] * s1[None, :] + b[:, None] * s2[None, :]
    return float(_integrand(p, np.broadcast_to(cr / A, p.shape), o, n).sum() * (A / (g * g)))


def quadrature_sphere(c, r, o, n, g=512):
    """Over the side of the sphere that o sees, in (z, phi) about the axis through o, which are
    area-uniform: from outside the cap z in [|r| / d, 1] towards o; from the centre (the domes) the
    half z in [0, 1] about n, the part above the horizon."""
    c, o, n = _a(c), _a(o), _a(n)
    R = abs(r)
    to = o - c
    d = math.sqrt(float(to @ to))
    if d > R:
        axis, z0 = to / d, R / d
    else:
        assert d == 0, "inside a sphere only its centre is supported"
        axis, z0 = n, 0.0
    e1 = np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= math.sqrt(float(e1 @ e1))
    e2 = np.cross(axis, e1)
    t = (np.arange(g) + 0.5) / g
    z, phi = (x.reshape(-1) for x in np.meshgrid(z0 + (1 - z0) * t, 2 * math.pi * t, indexing="ij"))
    s = np.sqrt(1 - z * z)
    u = z[:, None] * axis[None, :] + (s * np.cos(phi))[:, None] * e1[None, :] + (s * np.sin(phi))[:, None] * e2[None, :]
    return float(_integrand(c[None, :] + R * u, u, o, n).sum() * (2 * math.pi * (1 - z0) * R * R / (g * g)))


def quadrature_box(lo, hi, o, n, g=512):
    o = _a(o)
    total = 0.0
    for vs, nrm in box_faces(lo, hi):
        if float((o - vs[0]) @ nrm) > 0:
            total += quadrature_quad(vs[0], vs[1] - vs[0], vs[3] - vs[0], o, n, g)
    return total


# ---- worlds -------------------------------------------------------------------------------------------
@dataclass
class World:
    name: str
    d: object                 # SceneData
    ray: tuple                # the query's one ray
    o: tuple                  # where it lands
    n: tuple                  # the normal there
    lights: list = field(default_factory=list)  # closed-form worlds: (emission (3,), shape) with shape
                                                # ("sphere", c, r) | ("quad", v, s1, s2) | ("box", lo, hi) | ("dome", c, r)
    spheres_only: bool = False

    def factors(self):
        out = []
        for _, shape in self.lights:
            if shape[0] == "sphere":
                out.append(sphere_factor(shape[1], shape[2], self.o, self.n))
            elif shape[0] == "quad":
                out.append(polygon_factor(quad_vertices(*shape[1:]), self.o, self.n))
            elif shape[0] == "box":
                out.append(box_factor(shape[1], shape[2], self.o, self.n))
            else:
                out.append(1.0)  # the centre of a sphere sees it over the whole hemisphere
        return out

    def quadratures(self, g=512):
        out = []
        for _, shape in self.lights:
            q = {"sphere": quadrature_sphere, "quad": quadrature_quad, "box": quadrature_box, "dome": quadrature_sphere}[shape[0]]
            out.append(q(*shape[1:], self.o, self.n, g))
        return out

    def expected(self):
        """rho_k * sum over the lights of Le_k * F: the mean of channel k at depth 2."""
        F = self.factors()
        return np.array([RHO[k] * sum(e[k] * f for (e, _), f in zip(self.lights, F)) for k in range(3)])

    def rays(self, count):
        return np.ascontiguousarray(np.broadcast_to(np.array(self.ray, np.float64), (count, 6)))


def _scene(crt, mats, objs):
    """mats: [(kind, color, param)], objs: [(kind, material, values)]."""
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE
    m = np.zeros(len(mats), MATERIAL_DTYPE)
    for j, (kind, color, param) in enumerate(mats):
        m["kind"][j], m["color"][j], m["param"][j] = kind, color, param
    ob = np.zeros(len(objs), OBJECT_DTYPE)
    for j, (kind, mat, vals) in enumerate(objs):
        ob["kind"][j], ob["material"][j] = kind, mat
        ob["v"][j, :len(vals)] = vals
    d = crt.SceneData.named("config1")
    d.materials, d.objects = m, ob
    return d


SPHERE_C, SPHERE_R = (1.0, 3.0, 0.5), 1.0
SKEW = ((-1.0, 3.0, -0.5), (3.0, 0.5, 0.0), (0.7, -0.4, 1.5))
BOX = ((-1.0, 2.5, -0.5), (1.0, 3.5, 1.0))
# left of o, the sphere is to its right; small, so that the channel in which the two lights nearly cancel
# (0.6 * (3 F1 - 6 F2)) keeps a mean that 2^22 paths resolve to 1 %
MATE = ((-2.3, 3.0, -0.3), (0.6, 0.0, 0.0), (0.0, 0.0, 0.6))
CLOSED = ["solid", "hollow", "skew", "skew_back", "box", "dome", "dome_hollow", "zero_mate"]
OPEN = ["stacked", "bulb"]
DEEP = {"bulb_deep": ("bulb", 8)}  # a case of the sampled-against-unsampled comparison: (world, depth)
EDGE = ["in_plane", "half_sunk", "clamp_tail", "clamp_head"]
SPHERES_ONLY = ["solid_spheres", "hollow_spheres", "half_sunk_spheres"]
PLAN_WORLDS = ["cloud-300", "mixed-278", "flat-40"]
HALF_SUNK = ((2.0, 0.0, 0.5), 1.0)  # o sees a quarter of its surface, half of that above the floor
_MATS = [(LAMBERTIAN, RHO, 0.0), (LIGHT, COLOR, PARAM)]


def world(crt, name):
    """One of CLOSED, OPEN, EDGE or SPHERES_ONLY."""
    spheres = name.endswith("_spheres")
    base = name[:-len("_spheres")] if spheres else name
    ground = (1, 0, GROUND_SPHERE) if spheres else (2, 0, FLOOR)
    up = (0.0, 1.0, 0.0)

    def over(ox, oz, mats, objs, lights=()):
        return World(name, _scene(crt, mats, [ground] + objs), (ox, 2.0, oz, 0.0, -1.0, 0.0), (ox, 0.0, oz), up, list(lights), spheres)

    if base in ("solid", "hollow"):
        r = SPHERE_R if base == "solid" else -SPHERE_R
        return over(0.0, 0.0, _MATS, [(1, 1, SPHERE_C + (r,))], [(LE, ("sphere", SPHERE_C, r))])
    if base in ("skew", "skew_back"):
        v, s1, s2 = SKEW if base == "skew" else (SKEW[0], SKEW[2], SKEW[1])
        return over(0.0, 0.0, _MATS, [(2, 1, v + s1 + s2)], [(LE, ("quad", v, s1, s2))])
    if base == "box":
        return over(2.5, 0.0, _MATS, [(3, 1, BOX[0] + BOX[1])], [(LE, ("box",) + BOX)])
    if base in ("dome", "dome_hollow"):
        r = 30.0 if base == "dome" else -30.0
        return over(0.0, 0.0, _MATS, [(1, 1, (0.0, 0.0, 0.0, r))], [(LE, ("dome", (0.0, 0.0, 0.0), r))])
    if base == "zero_mate":
        le2 = tuple(c * MATE_PARAM for c in MATE_COLOR)
        return over(0.0, 0.0, _MATS + [(LIGHT, MATE_COLOR, MATE_PARAM)],
                    [(1, 1, SPHERE_C + (SPHERE_R,)), (2, 2, MATE[0] + MATE[1] + MATE[2])],
                    [(LE, ("sphere", SPHERE_C, SPHERE_R)), (le2, ("quad",) + MATE)])
    if base == "stacked":
        # from o the lower light covers part of the upper one, and a Lambertian sheet part of both
        return over(0.0, 0.0, _MATS,
                    [(2, 1, (-1.5, 4.0, -1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 2.0)), (2, 1, (0.0, 3.0, -0.5, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0)),
                     (2, 0, (0.3, 1.5, -1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.4))])
    if base == "bulb":
        return over(0.0, 0.0, _MATS + [(DIELECTRIC, (0.0, 0.0, 0.0), 1.5)],
                    [(1, 1, (-1.5, 2.0, 0.0, 0.4)), (1, 2, (-1.5, 2.0, 0.0, 0.8)), (1, 1, (1.5, 2.5, 0.0, 0.6))])
    if base == "half_sunk":
        return over(0.0, 0.0, _MATS, [(1, 1, HALF_SUNK[0] + (HALF_SUNK[1],))])
    if base in ("clamp_tail", "clamp_head"):
        lit, dark = (2, 1, (-2.5, 3.0, -1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0)), (2, 2, (0.5, 3.0, -1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0))
        return over(0.0, 0.0, _MATS + [(LIGHT, MATE_COLOR, MATE_PARAM)], [lit, dark] if base == "clamp_tail" else [dark, lit])
    if base == "in_plane":
        d = _scene(crt, _MATS, [(1, 0, (0.0, 0.0, 0.0, 1.0)), (2, 1, (-4.0, 0.0, -1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0))])
        return World(name, d, (-5.0, 0.0, 0.0, 1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (-1.0, 0.0, 0.0))
    raise KeyError(name)


# ---- crafted LCG states -------------------------------------------------------------------------------
LCG_A, LCG_C = 1664525, 1013904223
_LCG_A_INV = pow(LCG_A, -1, 1 << 32)
RND01_OF_MAX = float(0xFFFFFFFF) * (1 / float(4294967295 - 1))  # above 1
assert RND01_OF_MAX > 1


def lcg_next(s):
    return (LCG_A * s + LCG_C) & 0xFFFFFFFF


def lcg_prev(s):
    """The state before s: the inverse of s -> 1664525 * s + 1013904223 mod 2^32."""
    return ((s - LCG_C) * _LCG_A_INV) & 0xFFFFFFFF


def states_reaching(target, k):
    """The state from which the k-th draw leaves `target` (a draw steps the state, then reads it)."""
    s = target
    for _ in range(k):
        s = lcg_prev(s)
    return s


def _unit_vector_draws(crt, s):
    """How many draws random_unit_vector's rejection loop takes from state s, and the state after."""
    k = 0
    while True:
        s, x = crt.rand_double(s, -1.0, 1.0)
        s, y = crt.rand_double(s, -1.0, 1.0)
        s, z = crt.rand_double(s, -1.0, 1.0)
        k += 3
        if x * x + y * y + z * z < 1:
            return k, s


def crafted_states(crt, w):
    """{(which, "max" | "zero"): start state} for a World whose ray lands on a Lambertian: the path's xi1
    (and, where every light is a parallelogram, xi2 and xi3) is rnd_01 of 0xFFFFFFFF or of 0. The
    scatter's rejection loop comes first and takes a multiple of three draws: the back-ups by 3, 6, ... 30
    draws are tried in turn and the first that replays to the intended draw is kept (a loop accepts
    with probability pi / 6, so a target that none of them reaches is left out: the tests say which)."""
    kinds = w.d.materials["kind"][w.d.objects["material"]]
    quads_only = bool((w.d.objects["kind"][kinds == LIGHT] == 2).all())
    out = {}
    for j, which in enumerate(("xi1", "xi2", "xi3") if quads_only else ("xi1",)):
        for label, target in (("max", 0xFFFFFFFF), ("zero", 0)):
            for loop in range(3, 31, 3):
                s0 = states_reaching(target, loop + j + 1)
                took, s = _unit_vector_draws(crt, s0)
                if took != loop:
                    continue
                for _ in range(j + 1):
                    s, x = crt.rand_double(s, 0.0, 1.0)
                assert s == target and x == (RND01_OF_MAX if label == "max" else 0.0)
                out[which, label] = s0
                break
    return out


def n_for(ratio, share, cap=22):
    """The smallest power of two N with 5 * ratio / sqrt(N) <= share, and whether it is within 2^cap."""
    k = max(0, math.ceil(2 * math.log2(5 * ratio / share)))
    while 5 * ratio / math.sqrt(2 ** k) > share:
        k += 1
    return min(k, cap), k <= cap


# ---- the measured ratios and the N they give ----------------------------------------------------------
# world -> (the model's per-path sd / mean at depth 2, the largest channel, over 2^14 paths of seed 4100;
#           log2 of the smallest N with 5 * ratio / sqrt(N) <= 1 %). tests/test_light_truth.py holds both.
RATIO = {"solid": (1.616, 20), "hollow": (1.616, 20), "skew": (0.428, 16), "skew_back": (0.430, 16), "box": (1.420, 19),
         "zero_mate": (3.030, 22)}
# world -> (sqrt(sd0^2 + sd1^2) / m0 of the unsampled (0) and sampled (1) model, the largest channel, over
#           2^12 paths of seed 4200; log2 of the smallest N with 5 * ratio / sqrt(N) <= 2 %)
# bulb_deep is bulb at depth 8, where paths cross the shell and more than half of the mean is the inner
# light's, every hit of it unweighted (pb none after glass)
RATIO2 = {"stacked": (2.973, 20), "bulb": (5.991, 22), "bulb_deep": (4.695, 21), "cloud-300": (2.873, 19), "mixed-278": (3.121, 20), "flat-40": (3.482, 20)}
