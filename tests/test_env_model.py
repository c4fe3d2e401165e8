"""CPU-side checks of tests/env_model.py, the restatement the GPU tests of cube-map environments
(tests/test_gpu_env.py) hold the kernels to. No kernel runs here.

  - the lookup inverts the CUBE lens: the direction of every texel centre finds its own texel;
  - a map of equal texels returns that texel exactly, whatever the direction and the basis;
  - the decision edges of the header's steps 2 and 3;
  - the path model with a constant background is the oracle's ray_color within the project's bar for a
    forward-throughput integrator against the reference's recursion (1e-12), and
    the paths it ends in a miss are exactly the ones whose oracle value depends on the background.
"""
import math

import numpy as np
import pytest

import env_model as em
import lens_model as lm
import probe_sets as ps
from oracle import crt_oracle_py as orc

EPS = float(np.finfo(np.float64).eps)
SIZES = (1, 2, 4, 5, 8)
FILTERS = (em.NEAREST, em.BILINEAR)
ROTATED = dict(forward=(0.3, -0.5, -0.8), up=(0.1, 1.0, 0.2))
BASES = [dict(), ROTATED]


def integer_map(n):
    """Distinct small integers, every channel of every texel its own."""
    return (np.arange(6 * n * n * 3, dtype=np.float64) + 1.0).reshape(6 * n, n, 3)


class CubeLens:
    kind = lm.CUBE
    extent_x = extent_y = 0.0
    origin = (0.0, 0.0, 0.0)

    def __init__(self, env):
        self.right, self.up, self.forward = env.right, env.up, env.forward


def centre_directions(env):
    """lens_model.direction at every texel centre of the 6n x n frame, row-major: (6 n n, 3)."""
    n, lens = env.n, CubeLens(env)
    out = []
    for row in range(6 * n):
        h_face, face, rf = lm.face_rows(lens, n, 6 * n, row)
        for col in range(n):
            a, b = lm.pixel_ab(n, h_face, col, rf)
            out.append(lm.direction(lens, a, b, face)[1])
    return np.array(out)


def test_material_kinds_are_the_packages(crt):
    assert (em.LAMBERTIAN, em.METAL, em.DIELECTRIC, em.DIFFUSE_LIGHT) == \
        (crt.CRT_LAMBERTIAN, crt.CRT_METAL, crt.CRT_DIELECTRIC, crt.CRT_DIFFUSE_LIGHT)
    assert (em.NEAREST, em.BILINEAR) == (crt.CRT_ENV_NEAREST, crt.CRT_ENV_BILINEAR)
    r, u, f = em.basis(**ROTATED)
    lens = crt.make_lens("cube", **ROTATED)
    assert (r, u, f) == (tuple(lens.right), tuple(lens.up), tuple(lens.forward))


@pytest.mark.parametrize("basis", BASES, ids=["default", "rotated"])
@pytest.mark.parametrize("filt", FILTERS, ids=["nearest", "bilinear"])
@pytest.mark.parametrize("n", SIZES)
def test_lookup_round_trip(n, filt, basis):
    """The weights of BILINEAR at a texel centre are 0 or 1 only up to the rounding of (u + 1)(n / 2):
    8 eps of the largest texel."""
    t = integer_map(n)
    env = em.make(t, filter=filt, **basis)
    got = em.lookup(env, centre_directions(env)).reshape(6 * n, n, 3)
    if filt == em.NEAREST:
        assert np.array_equal(got, t)
    else:
        err = float(np.abs(got - t).max())
        print(f"n = {n}: largest bilinear error at a texel centre = {err / (EPS * t.max()):.3g} eps max|texel|")
        assert err <= 8 * EPS * t.max()


def probe_directions():
    rng = np.random.default_rng(7)
    d = [rng.normal(size=(256, 3))]
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    d.append(axes)
    d.append(np.array([[sx, sy, 0.0] for sx in (1, -1) for sy in (1, -1)] +
                      [[sx, 0.0, sz] for sx in (1, -1) for sz in (1, -1)] +
                      [[0.0, sy, sz] for sy in (1, -1) for sz in (1, -1)]))           # face diagonals
    d.append(np.array([[s * 1.0, t * 1.0, u * 1.0] for s in (1, -1) for t in (1, -1) for u in (1, -1)]))  # corners
    z = rng.normal(size=(24, 3))
    for i in range(24):
        z[i, i % 3] = 0.0 if i % 2 else -0.0                                         # +-0 components
    d.append(z)
    base = np.concatenate(d)
    return np.concatenate([base, base * 2.0 ** 300, base * 2.0 ** -300])


@pytest.mark.parametrize("basis", BASES, ids=["default", "rotated"])
@pytest.mark.parametrize("filt", FILTERS, ids=["nearest", "bilinear"])
def test_constant_map_returns_its_texel_exactly(filt, basis):
    c = np.array([0.3, 1.7, 2.9])
    dirs = probe_directions()
    for n in (1, 5):
        env = em.make(np.broadcast_to(c, (6 * n, n, 3)).copy(), filter=filt, **basis)
        got = em.lookup(env, dirs, background=(9.0, 9.0, 9.0))
        assert np.array_equal(got, np.broadcast_to(c, got.shape)), (n, filt)


def identity_env(n, filt):
    """right, up, forward = the x, y and z axes: a direction's local coordinates are its own."""
    return em.Env(integer_map(n), filt, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def texel(env, face, row, col):
    return env.texels[face * env.n + row, col]


def test_face_ties_and_signs():
    """Step 3's order: x wins ties with y and z, y wins a tie with z; the sign picks the face."""
    env = identity_env(4, em.NEAREST)
    one = lambda d: em.lookup(env, [d])[0]  # noqa: E731
    # ax == ay > az: an X face; u = -+z / m, v = -y / m = -+1 -> the clamped edge row
    assert np.array_equal(one((1.0, 1.0, 0.25)), texel(env, 0, 0, 1))    # u = -0.25 -> fx = 1.5; v = -1 -> row 0
    assert np.array_equal(one((-1.0, 1.0, 0.25)), texel(env, 1, 0, 2))   # u = 0.25 -> fx = 2.5
    assert np.array_equal(one((1.0, -1.0, 0.25)), texel(env, 0, 3, 1))   # v = 1 -> fy = 4 -> clamped to row 3
    # ay == az > ax: a Y face
    assert np.array_equal(one((0.25, 1.0, 1.0)), texel(env, 2, 3, 2))    # +Y: u = x / m, v = z / m = 1
    assert np.array_equal(one((0.25, -1.0, 1.0)), texel(env, 3, 0, 2))   # -Y: v = -z / m = -1
    # ax == az > ay: an X face again
    assert np.array_equal(one((1.0, 0.25, 1.0)), texel(env, 0, 1, 0))    # u = -1 -> col 0; v = -0.25 -> fy = 1.5
    # all three equal: +X / -X by the sign of x alone
    assert np.array_equal(one((1.0, 1.0, 1.0)), texel(env, 0, 0, 0))
    assert np.array_equal(one((-1.0, -1.0, -1.0)), texel(env, 1, 3, 0))  # u = z / m = -1, v = -y / m = 1
    # z strictly largest: the Z faces
    assert np.array_equal(one((0.25, 0.25, 1.0)), texel(env, 4, 1, 2))   # u = 0.25, v = -0.25
    assert np.array_equal(one((0.25, 0.25, -1.0)), texel(env, 5, 1, 1))  # u = -x / m = -0.25
    # each axis, each sign: the face's centre (fx = fy = 2 -> texel (2, 2))
    for face, d in enumerate([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]):
        assert np.array_equal(one(tuple(float(v) for v in d)), texel(env, face, 2, 2)), face


@pytest.mark.parametrize("filt", FILTERS, ids=["nearest", "bilinear"])
def test_directions_without_a_major_axis_see_the_background(filt):
    env = identity_env(2, filt)
    bg = (0.125, 0.25, 0.5)
    nan, inf = math.nan, math.inf
    bad = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (nan, 1.0, 1.0), (1.0, nan, 0.0), (0.0, 1.0, nan), (nan, nan, nan),
           (inf, 0.0, 0.0), (1.0, -inf, 1.0), (0.0, 0.0, inf), (inf, -inf, inf), (inf, nan, 0.0)]
    got = em.lookup(env, bad, bg)
    assert np.array_equal(got, np.broadcast_to(np.array(bg), got.shape))
    # a rotated basis can overflow a finite direction's local coordinates: inf - inf = NaN -> background
    rot = em.make(integer_map(2), filter=filt, **ROTATED)
    got = em.lookup(rot, [(1.7e308, 1.7e308, -1.7e308)], bg)
    assert np.array_equal(got[0], np.array(bg))
    # denormal and huge finite directions still have one
    ok = em.lookup(env, [(5e-324, 0.0, 0.0), (0.0, -1.7e308, 0.0)], bg)
    assert np.array_equal(ok[0], em.lookup(env, [(1.0, 0.0, 0.0)])[0])
    assert np.array_equal(ok[1], em.lookup(env, [(0.0, -1.0, 0.0)])[0])


def test_bilinear_clamps_inside_the_face():
    """At a face's edge the second tap is the edge texel again, never the neighbouring face's row."""
    env = identity_env(2, em.BILINEAR)
    got = em.lookup(env, [(1.0, 1.0, 0.0)])[0]  # +X, u = 0 -> gx = 0.5 (between the columns), v = -1 -> gy = -0.5
    a = texel(env, 0, 0, 0) + 0.5 * (texel(env, 0, 0, 1) - texel(env, 0, 0, 0))
    assert np.array_equal(got, a + 0.5 * (a - a))


# ---- the path model against the oracle ---------------------------------------------------------------
MODEL_SCENES = ["rtow_final", "mixed", "rtow_final_lights"]


@pytest.mark.parametrize("depth", [1, 2, 3, 50])
@pytest.mark.parametrize("name", MODEL_SCENES)
def test_path_model_is_the_oracles_ray_color(crt, name, depth):
    d, _ = ps.world(crt, name)
    p = ps.probe(crt, name, "S")
    rgb, ended, _, T = em.ray_color(orc, d, p.rays, p.states, depth, ps.BG, p.t_min)
    want = ps.oracle(crt, name, "S", depth)
    err = float(np.abs(rgb - want).max())
    bar = 1e-12 * max(1.0, float(np.abs(want).max()))
    print(f"{name} depth {depth}: max |model - oracle| = {err:.3g} (bar {bar:.3g}); ends "
          f"{np.bincount(ended, minlength=4).tolist()} (miss, light, absorbed, depth)")
    assert err <= bar
    # the paths that end in a miss are the ones whose value depends on the background
    black = ps.oracle(crt, name, "S", depth, bg=(0.0, 0.0, 0.0))
    white = ps.oracle(crt, name, "S", depth, bg=(1.0, 1.0, 1.0))
    lit = (T != 0).any(1)
    assert np.array_equal((ended == em.MISS) & lit, (black != white).any(1) & lit)
    assert lit.mean() > 0.9
    if depth == 50:  # the sets are worth using: a quarter of the paths escape after a bounce
        first_miss = orc.hits(d, p.rays, p.t_min)["prim"] < 0
        share = float(((ended == em.MISS) & ~first_miss).mean())
        print(f"{name}: {share:.3f} of the paths end in a miss after one or more bounces")
        assert share >= 0.25


def test_refused_rays_and_depth_zero(crt):
    d, _ = ps.world(crt, "rtow_final")
    rays = np.array([[math.nan, 0, 0, 0, 1, 0], [0, 50, 0, 0, 0, 0], [0, 50, 0, 0, 1, 0], [0, 50, 0, math.inf, 1, 0]], np.float64)
    st = np.array([1, 2, 3, 4], np.uint32)
    env = identity_env(2, em.NEAREST)
    rgb, ended, _, _ = em.ray_color(orc, d, rays, st, 5, ps.BG, 1e-5, env=env)
    assert (ended == em.MISS).all()
    up = em.lookup(env, [(0.0, 1.0, 0.0)])[0]
    # a refused ray is a first-segment miss with its own direction: the NaN origin still looks up
    assert np.array_equal(rgb[0], up) and np.array_equal(rgb[2], up)
    # the zero and the infinite direction have no major axis: the constant background
    assert np.array_equal(rgb[1], np.array(ps.BG)) and np.array_equal(rgb[3], np.array(ps.BG))
    rgb, ended, _, _ = em.ray_color(orc, d, rays, st, 0, ps.BG, 1e-5, env=env)
    assert not rgb.any() and (ended == em.DEPTH).all()
