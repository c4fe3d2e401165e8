"""Truth for luminance-sampled cube-map environments that is no restatement of the kernel: the closed-form
irradiance factor and solid angle of a texel, written from the forward map (face, u, v) -> direction alone,
a quadrature that checks them, the worlds they hold in, worlds for the estimator's edge events, and LCG
states crafted to reach draws of exactly 0 and above 1. tests/test_env_truth.py uses it without a GPU,
tests/test_gpu_env_truth.py and tests/test_gpu_env_nee_edges.py on one. Not a test module. Nothing here
comes from env_nee_model; env_model gives the Env record and, for BILINEAR only, its lookup.

A Lambertian floor point o with normal n and albedo rho under a NEAREST map sends back, per channel,
rho_k * sum over the texels of L_k * F_texel at depth 2, F the texel's form factor (1 / pi times the
integral of cos over the solid angle it fills above the horizon): the estimator's mean, whatever its
sampling and weights, if it is unbiased. Truth never inverts the map: a texel is the quadrilateral of its
four corner directions, clipped to n . x >= 0, under Lambert's edge formula.

  texel_corners      the four corners of a texel from include/crt_render.h's CUBE table, times the basis
  texel_factor       the clipped quadrilateral's form factor (light_truth.polygon_factor where no clip is needed)
  texel_solid_angle  atan(u v / sqrt(1 + u^2 + v^2)) over the four corners
  quadrature_texel   a midpoint rule in (u, v) with the Jacobian 1 / s^1.5: the factor, and the integrals of
                     the nine SH basis functions and of their squares
  quadrature_lookup  a midpoint rule of env_model.lookup * cos / pi over the hemisphere: truth under BILINEAR

A World's query is one ray, repeated; it lands on a Lambertian at `o` with the normal `n` facing the ray.
CLOSED worlds have a closed form, BILINEAR ones the quadrature of the lookup, OPEN ones (glass) neither: there
the unsampled estimator is the truth. sun_bilinear's sun is a 3 x 3 block of texels: BILINEAR spreads one bright
texel over a rim where env_pdf is its dim neighbours' (DESIGN 6l), the model's sd / mean is 6.0 there and 1 % of
the mean would take 2^24 paths; with the block it is 1.10.
"""
import math
from dataclasses import dataclass

import numpy as np

import env_model as em
from light_truth import (GROUND_SPHERE, RND01_OF_MAX, _scene, lcg_prev, n_for, polygon_factor, sphere_factor,  # noqa: F401
                         states_reaching)
from test_env_model import ROTATED

RHO = (0.5, 0.6, 0.7)
ROOF_RHO = (0.8, 0.3, 0.4)
LAMBERTIAN, DIELECTRIC = 1, 3
T_MIN = 1e-5
BG = (0.0, 0.0, 0.0)
SUN = (1e4, 8e3, 6e3)
FLOOR = (-50.0, 0.0, -50.0, 100.0, 0.0, 0.0, 0.0, 0.0, 100.0)
# the real SH basis of bands 0..2 in the order of include/crt_render.h: 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2
Y0 = 0.5 * math.sqrt(1 / math.pi)
_Y1, _Y2, _Y20, _Y22 = math.sqrt(3 / (4 * math.pi)), 0.5 * math.sqrt(15 / math.pi), 0.25 * math.sqrt(5 / math.pi), 0.25 * math.sqrt(15 / math.pi)


def _a(x):
    return np.asarray(x, np.float64)


def sh_basis(d):
    """The nine functions at unit directions d (m, 3): (m, 9)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.full(len(d), Y0), _Y1 * y, _Y1 * z, _Y1 * x, _Y2 * x * y, _Y2 * y * z, _Y20 * (3 * z * z - 1), _Y2 * x * z,
                     _Y22 * (x * x - y * y)], 1)


# ---- the forward map ----------------------------------------------------------------------------------
def local_direction(face, u, v):
    """The CUBE table: the local direction of face 0..5 at (u, v), v pointing down the image."""
    one = np.ones_like(_a(u))
    u, v = _a(u) * one, _a(v) * one
    return {0: (one, -v, -u), 1: (-one, -v, u), 2: (u, one, v), 3: (u, -one, -v), 4: (u, -v, one), 5: (-u, -v, -one)}[face]


def direction(env, face, u, v):
    """World-space directions (..., 3) of (face, u, v): R x + U y + F z."""
    x, y, z = local_direction(face, u, v)
    R, U, F = _a(env.right), _a(env.up), _a(env.forward)
    return x[..., None] * R + y[..., None] * U + z[..., None] * F


def _bounds(n, row, col):
    g = 2.0 / n
    return col * g - 1.0, (col + 1) * g - 1.0, row * g - 1.0, (row + 1) * g - 1.0


def texel_corners(env, face, row, col):
    """(4, 3): the corners of texel (row_in_face, col) of a face, in order around it."""
    u0, u1, v0, v1 = _bounds(env.n, row, col)
    return direction(env, face, _a([u0, u1, u1, u0]), _a([v0, v0, v1, v1]))


# ---- closed forms -------------------------------------------------------------------------------------
def clip_to_horizon(vertices, n):
    """Sutherland-Hodgman against the half-space n . x >= 0: the clipped polygon's vertices (k, 3), k >= 0."""
    v, n = _a(vertices), _a(n)
    h = v @ n
    out = []
    for i in range(len(v)):
        j = (i + 1) % len(v)
        if h[i] >= 0:
            out.append(v[i])
        if (h[i] >= 0) != (h[j] >= 0):
            t = h[i] / (h[i] - h[j])
            out.append(v[i] + t * (v[j] - v[i]))
    return np.array(out).reshape(-1, 3)


def edge_sum_factor(vertices, n):
    """Lambert's formula over the edges of a polygon seen from the origin, vertices on the horizon allowed
    (polygon_factor refuses them) and zero-length edges, which clipping leaves, skipped."""
    R, n = _a(vertices), _a(n)
    if len(R) < 3:
        return 0.0
    R = R / np.sqrt((R * R).sum(1))[:, None]
    total = 0.0
    for i in range(len(R)):
        a, b = R[i], R[(i + 1) % len(R)]
        cr = np.cross(a, b)
        s = math.sqrt(float(cr @ cr))
        if s == 0.0:
            continue
        total += math.atan2(s, float(a @ b)) * float((cr / s) @ n)
    return abs(total) / (2 * math.pi)


def texel_factor(env, face, row, col, n):
    q = texel_corners(env, face, row, col)
    h = q @ _a(n)
    if (h > 0).all():
        return polygon_factor(q, (0.0, 0.0, 0.0), n)
    if (h <= 0).all():
        return 0.0
    return edge_sum_factor(clip_to_horizon(q, n), n)


def is_cut(env, face, row, col, n):
    h = texel_corners(env, face, row, col) @ _a(n)
    return bool((h > 0).any() and (h < 0).any())


def _A(u, v):
    return math.atan(u * v / math.sqrt(1 + u * u + v * v))


def texel_solid_angle(n, row, col):
    """The solid angle of texel (row_in_face, col) of any face of an n x n map."""
    u0, u1, v0, v1 = _bounds(n, row, col)
    return (_A(u1, v1) - _A(u0, v1)) - (_A(u1, v0) - _A(u0, v0))


def factors(env, n):
    """(6n, n): texel_factor of every texel, rows as the map's own."""
    N = env.n
    return np.array([[texel_factor(env, r // N, r % N, c, n) for c in range(N)] for r in range(6 * N)])


def solid_angles(N):
    return np.array([[texel_solid_angle(N, r % N, c) for c in range(N)] for r in range(6 * N)])


# ---- quadrature ---------------------------------------------------------------------------------------
def _cells(env, face, u0, u1, v0, v1, g):
    """Unit directions (g * g, 3) at the midpoints of a g x g grid over [u0, u1] x [v0, v1] of a face, and the
    solid angle of each cell to second order: du dv / s^1.5."""
    t = (np.arange(g) + 0.5) / g
    u, v = (x.reshape(-1) for x in np.meshgrid(u0 + (u1 - u0) * t, v0 + (v1 - v0) * t, indexing="ij"))
    s = 1 + u * u + v * v
    d = direction(env, face, u, v) / np.sqrt(s)[:, None]
    return d, ((u1 - u0) * (v1 - v0) / (g * g)) / (s * np.sqrt(s))


def quadrature_texel(env, face, row, col, n=None, g=512):
    """(the factor under normal n, or None without one; the solid angle; the integrals of the nine SH
    functions (9,); those of their squares (9,)) of a texel by the midpoint rule."""
    d, dw = _cells(env, face, *_bounds(env.n, row, col), g)
    F = None if n is None else float((np.maximum(d @ _a(n), 0.0) * dw).sum() / math.pi)
    Y = sh_basis(d)
    return F, float(dw.sum()), (Y * dw[:, None]).sum(0), (Y * Y * dw[:, None]).sum(0)


def quadrature_lookup(env, n, g=480):
    """(3,): the integral of env_model.lookup * cos / pi over the hemisphere about n, a g x g midpoint grid
    a face (g a multiple of 2 * env.n keeps the cells inside BILINEAR's smooth pieces)."""
    assert g % (2 * env.n) == 0
    total = np.zeros(3)
    for face in range(6):
        d, dw = _cells(env, face, -1.0, 1.0, -1.0, 1.0, g)
        c = np.maximum(d @ _a(n), 0.0) * dw
        total += (em.lookup(env, d, BG) * c[:, None]).sum(0)
    return total / math.pi


# ---- worlds -------------------------------------------------------------------------------------------
@dataclass
class World:
    name: str
    d: object                 # SceneData
    env: object               # env_model.Env
    basis: dict               # the keywords em.make and make_env built the basis from
    ray: tuple
    o: tuple
    n: tuple
    occluder: tuple = None    # ("roof", rows, cols of +Y texels) | ("ball", c, r, L_b)
    spheres_only: bool = False

    def rays(self, count):
        return np.ascontiguousarray(np.broadcast_to(np.array(self.ray, np.float64), (count, 6)))

    def texel_terms(self):
        """(6n, n, 3): L_k * F of every texel that o sees (a roof's block removed)."""
        F = factors(self.env, self.n)
        if self.occluder and self.occluder[0] == "roof":
            N = self.env.n
            for r in self.occluder[1]:
                for c in self.occluder[2]:
                    F[2 * N + r, c] = 0.0
        return self.env.texels * F[:, :, None]

    def irradiance(self):
        """(3,): sum L F, or under BILINEAR the quadrature of the lookup."""
        if self.env.filter == em.BILINEAR:
            assert self.occluder is None
            return quadrature_lookup(self.env, self.n)
        total = self.texel_terms().sum((0, 1))
        if self.occluder and self.occluder[0] == "ball":
            _, c, r, Lb = self.occluder
            total = total - _a(Lb) * sphere_factor(c, r, self.o, self.n)
        return total

    def expected(self):
        """rho_k * irradiance_k: the mean of channel k at depth 2."""
        return _a(RHO) * self.irradiance()

    def face_shares(self):
        """(6,): each face's largest share of a channel of sum L F (NEAREST worlds)."""
        t = self.texel_terms()
        N = self.env.n
        return np.array([(t[f * N:(f + 1) * N].sum((0, 1)) / t.sum((0, 1))).max() for f in range(6)])


def random_map(n=8, seed=6100):
    return np.random.default_rng(seed).random((6 * n, n, 3)) * 4.0


def sun_map(n, row, col, spread=0):
    """0.5 everywhere and SUN in one texel, or in the (2 spread + 1)^2 block about it."""
    t = np.full((6 * n, n, 3), 0.5)
    t[row - spread:row + spread + 1, col - spread:col + spread + 1] = SUN
    return t


SUN_AT = (1, 7)          # +X, row 1 (above the horizon of +Y), the last column: past it lies the next face
SUN_BLOCK_AT = (2, 4)    # sun_bilinear: +X, rows 1..3, columns 3..5 (see the module's note on BILINEAR)
SUN_HORIZON_AT = (2, 2)  # +X, n = 5: the middle row, v in [-0.2, 0.2]
HALF_BLACK_ROWS = (0, 3, 4, 7, 11, 12, 13, 18, 22, 26, 29)
HALF_BLACK_N = (0.36, -0.48, 0.8)  # a wall that sees the last row's last texel whole and cuts the first row
TILTED_N = tuple((np.array([0.3, 0.8, -0.52]) / math.sqrt(0.3 ** 2 + 0.8 ** 2 + 0.52 ** 2)).tolist())
ROOF_BLOCK = ((2, 3), (1, 2))  # rows, cols of the +Y face, n = 4: u in [-0.5, 0.5], v in [0, 1]
BALL_C, BALL_R, BALL_L = (0.1, 3.0, -0.1), 0.8, (1.5, 2.5, 0.7)
BALL_BLOCK = ((2, 3, 4, 5), (2, 3, 4, 5))  # rows, cols of the +Y face, n = 8: |u|, |v| <= 0.5
GLASS = (1.0, 1.0, 0.0, 0.9)

CLOSED = ["random", "tilted", "sun", "sun_horizon", "half_black", "under", "roof", "ball"]
BILINEAR = ["random_bilinear", "sun_bilinear"]
OPEN = ["glass"]
SPHERES_ONLY = ["random_spheres", "sun_horizon_spheres", "ball_spheres"]
UNSAMPLED_TOO = ["random", "tilted", "under"]
ALL = CLOSED + BILINEAR + OPEN + SPHERES_ONLY


def _tangents(n):
    n = _a(n)
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= math.sqrt(float(a @ a))
    return a, np.cross(n, a)


def ball_margin(w):
    """How far, at the least, the ball stays inside the pyramid that o and its block of texels span: the
    smallest distance of the centre from the four planes through o and a side of the block, less the radius."""
    _, c, r, _ = w.occluder
    rows, cols = BALL_BLOCK
    N = w.env.n
    q = np.array([texel_corners(w.env, 2, rows[0], cols[0])[0], texel_corners(w.env, 2, rows[0], cols[-1])[1],
                  texel_corners(w.env, 2, rows[-1], cols[-1])[2], texel_corners(w.env, 2, rows[-1], cols[0])[3]])
    centre = q.mean(0)
    dist = []
    for i in range(4):
        m = np.cross(q[i], q[(i + 1) % 4])
        m = m / math.sqrt(float(m @ m))
        if m @ centre < 0:
            m = -m
        dist.append(float(m @ (_a(c) - _a(w.o))))
    assert N == 8
    return min(dist) - r


def world(crt, name):
    spheres = name.endswith("_spheres")
    bilinear = name.endswith("_bilinear")
    base = name[:-len("_spheres")] if spheres else name[:-len("_bilinear")] if bilinear else name
    filt = em.BILINEAR if bilinear else em.NEAREST
    mats = [(LAMBERTIAN, RHO, 0.0), (LAMBERTIAN, ROOF_RHO, 0.0), (DIELECTRIC, (0.0, 0.0, 0.0), 1.5)]
    ground = (1, 0, GROUND_SPHERE) if spheres else (2, 0, FLOOR)
    up = (0.0, 1.0, 0.0)

    def over(texels, objs=(), basis=None, occluder=None, start=2.0):
        basis = basis or {}
        return World(name, _scene(crt, mats, [ground] + list(objs)), em.make(texels, filter=filt, **basis), basis,
                     (0.0, start, 0.0, 0.0, -1.0, 0.0), (0.0, 0.0, 0.0), up, occluder, spheres)

    def wall(texels, n, basis=None):
        basis = basis or {}
        n = _a(n)
        s1, s2 = _tangents(n)
        v = -50.0 * s1 - 50.0 * s2
        floor = (2, 0, tuple(v.tolist()) + tuple((100.0 * s1).tolist()) + tuple((100.0 * s2).tolist()))
        return World(name, _scene(crt, mats, [floor]), em.make(texels, filter=filt, **basis), basis,
                     tuple((2.0 * n).tolist()) + tuple((-n).tolist()), (0.0, 0.0, 0.0), tuple(n.tolist()))

    if base == "random":
        return over(random_map())
    if base == "tilted":
        return wall(random_map(), TILTED_N, ROTATED)
    if base == "sun":
        return over(sun_map(8, *SUN_AT) if not bilinear else sun_map(8, *SUN_BLOCK_AT, spread=1))
    if base == "sun_horizon":
        return over(sun_map(5, *SUN_HORIZON_AT))
    if base == "half_black":
        t = random_map(5, 6101) + 0.05
        t[list(HALF_BLACK_ROWS)] = 0.0
        return wall(t, HALF_BLACK_N)
    if base == "under":
        w = over(random_map(8, 6102))
        w.ray, w.n = (0.0, -2.0, 0.0, 0.0, 1.0, 0.0), (0.0, -1.0, 0.0)
        return w
    if base == "roof":
        # +Y is (u, 1, v) locally and the default basis has forward = -Z: at y = 2 the block is x in [-1, 1], z in [-2, 0]
        return over(random_map(4, 6103), [(2, 1, (-1.0, 2.0, -2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0))], occluder=("roof",) + ROOF_BLOCK,
                    start=1.0)
    if base == "ball":
        t = random_map(8, 6104)
        for r in BALL_BLOCK[0]:
            t[2 * 8 + r, list(BALL_BLOCK[1])] = BALL_L
        return over(t, [(1, 1, BALL_C + (BALL_R,))], occluder=("ball", BALL_C, BALL_R, BALL_L))
    if base == "glass":
        return over(random_map(8, 6105), [(1, 2, GLASS)])
    raise KeyError(name)


# ---- the probes' own estimators ------------------------------------------------------------------------
def cosine_moments(w):
    """(mean (3,), sd (3,)) of L(d) with d drawn by cosine about n, a HEMISPHERE bake's samples at max_depth
    1 and the unsampled estimator's bounce: E L = sum L F and E L^2 = sum L^2 F, closed forms both."""
    F = factors(w.env, w.n)[:, :, None]
    m1, m2 = (w.env.texels * F).sum((0, 1)), (w.env.texels ** 2 * F).sum((0, 1))
    return m1, np.sqrt(m2 - m1 * m1)


def cosine_ratio(w):
    """sd / mean of cosine_moments, the largest channel."""
    m, sd = cosine_moments(w)
    return float((sd / m).max())


def sphere_moments(env, g=128):
    """(mean (9, 3), sd (9, 3)) of one sample 4 pi Y_k(d) L(d) of a SPHERE bake in the open, d uniform: the
    mean's band 0 from texel_solid_angle, everything else from quadrature_texel."""
    N = env.n
    m1, m2 = np.zeros((9, 3)), np.zeros((9, 3))
    for r in range(6 * N):
        for c in range(N):
            _, _, y, yy = quadrature_texel(env, r // N, r % N, c, None, g)
            y[0] = Y0 * texel_solid_angle(N, r % N, c)
            L = env.texels[r, c]
            m1 += y[:, None] * L[None, :]
            m2 += 4 * math.pi * yy[:, None] * (L * L)[None, :]
    return m1, np.sqrt(m2 - m1 * m1)


# ---- crafted LCG states -------------------------------------------------------------------------------
def _unit_vector_draws(crt, s):
    k = 0
    while True:
        s, x = crt.rand_double(s, -1.0, 1.0)
        s, y = crt.rand_double(s, -1.0, 1.0)
        s, z = crt.rand_double(s, -1.0, 1.0)
        k += 3
        if x * x + y * y + z * z < 1:
            return k, s


def crafted_states(crt, w):
    """{("xi1".."xi4", "max" | "zero"): start state}: the floor bounce's xi_j is rnd_01 of 0xFFFFFFFF or of 0.
    The scatter's rejection loop comes first and takes a multiple of three draws; the back-ups by 3, 6, ...
    30 draws are tried in turn and the first that replays to the intended draw is kept. A target that the
    LCG cannot reach after a scatter is left out (the tests say which, and why)."""
    assert int(w.d.materials["kind"][w.d.objects["material"][0]]) == LAMBERTIAN
    out = {}
    for j in range(4):
        for label, target in (("max", 0xFFFFFFFF), ("zero", 0)):
            for loop in range(3, 31, 3):
                s0 = states_reaching(target, loop + j + 1)
                took, s = _unit_vector_draws(crt, s0)
                if took != loop:
                    continue
                for _ in range(j + 1):
                    s, x = crt.rand_double(s, 0.0, 1.0)
                assert s == target and x == (RND01_OF_MAX if label == "max" else 0.0)
                out[f"xi{j + 1}", label] = s0
                break
    return out


# ---- the measured ratios and the N they give ----------------------------------------------------------
# world -> (the model's per-path sd / mean at depth 2, the largest channel, over 2^14 paths of seed 6200;
#           log2 of the smallest N with 5 * ratio / sqrt(N) <= 1 %). tests/test_env_truth.py holds both.
RATIO = {"random": (0.615, 17), "tilted": (0.609, 17), "sun": (0.229, 14), "sun_horizon": (1.248, 19), "half_black": (0.906, 18),
         "under": (0.584, 17), "roof": (0.740, 18), "ball": (0.683, 17), "random_bilinear": (0.489, 16), "sun_bilinear": (1.103, 19),
         "random_spheres": (0.615, 17), "sun_horizon_spheres": (1.248, 19), "ball_spheres": (0.683, 17)}
# glass at depth -> (sqrt(sd0^2 + sd1^2) / m0 of the unsampled (0) and the sampled (1) model, the largest
#                    channel, over 2^12 paths of seed 6300; log2 of the smallest N with 5 * ratio / sqrt(N) <= 2 %)
RATIO2 = {2: (1.260, 17), 8: (0.856, 16)}
# log2 of the samples of a probe bake at max_depth 1: the smallest S with 5 * (sd / mean) / sqrt(S) <= 1 %, sd / mean the
# closed forms cosine_ratio (HEMISPHERE: 0.620 and 0.615) and sphere_moments' band 0 (SPHERE over `random`: 0.597)
PROBE_LOG2_S = {"random": 17, "tilted": 17, "sphere": 17}
