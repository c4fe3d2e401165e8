"""Closed-form truth for the lit estimator: a Lambertian floor point of albedo rho under a cube map and a
lamp returns, at depth 2, rho * (sum of L F over the texels it sees + Le F_lamp) per channel. Restates
nothing of tests/lighting_model.py; the factors are env_truth's (texels) and light_truth's (polygon, sphere).
Not a test module.

  lamp_roof          env_truth's `roof` with the roof a DiffuseLight: its outline is a 2 x 2 block of +Y
                     texels, so the texel sum already leaves the block out; + Le * polygon_factor
  lamp_ball          env_truth's `ball` with the ball a DiffuseLight sphere: the sum - L_b * sphere_factor
                     (env_truth's own subtraction) + Le * sphere_factor
  lamp_ball_spheres  the same on a ground sphere (sphere-only instances)
  lamp_sun           env_truth's `sun` map over the floor with a parallelogram lamp at y = 2 whose outline is
                     the 2 x 2 block of +Y texels about the zenith (rows 3, 4, columns 3, 4 of n = 8, all
                     0.5): the sum without the block's own terms + Le * polygon_factor

Each world runs under a sampler and under a plain map (`sampled`). RATIO holds the model's per-path
sd / mean at depth 2 (the largest channel) over 2^14 paths of seed 7100 and log2 of the smallest N with
5 * ratio / sqrt(N) <= 1 % (light_truth.n_for, cap 22), the path counts of tests/test_gpu_lighting_truth.py;
tests/test_lighting_truth.py holds both.
"""
import numpy as np

import env_truth as et
import light_truth as lt
from env_truth import factors  # noqa: F401 (re-exported: the texel factors)
from light_truth import n_for, polygon_factor, sphere_factor  # noqa: F401

LE_COLOR, LE_PARAM = (1.0, 0.8, 0.6), 6.0
LE = tuple(c * LE_PARAM for c in LE_COLOR)
WORLDS = ["lamp_roof", "lamp_ball", "lamp_ball_spheres", "lamp_sun"]
SUN_LAMP = (-0.5, 2.0, -0.5, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)
SUN_LAMP_BLOCK = ((3, 4), (3, 4))  # rows, cols of the +Y face, n = 8: |u|, |v| <= 0.25, at y = 2 |x|, |z| <= 0.5
SEED = 7100


def world(crt, name):
    """(env_truth.World with the lamp in place of the occluder, the expected mean (3,))."""
    if name == "lamp_sun":
        w = et.world(crt, "sun")
        mats = [(lt.LAMBERTIAN, et.RHO, 0.0), (lt.LIGHT, LE_COLOR, LE_PARAM)]
        w.d = et._scene(crt, mats, [(2, 0, et.FLOOR), (2, 1, SUN_LAMP)])
        rows, cols = SUN_LAMP_BLOCK
        N = w.env.n
        F = factors(w.env, w.n)
        block = sum(w.env.texels[2 * N + r, c] * F[2 * N + r, c] for r in rows for c in cols)
        assert all((w.env.texels[2 * N + r, c] == 0.5).all() for r in rows for c in cols)
        f_lamp = polygon_factor(lt.quad_vertices(SUN_LAMP[:3], SUN_LAMP[3:6], SUN_LAMP[6:9]), w.o, w.n)
        assert abs(sum(F[2 * N + r, c] for r in rows for c in cols) - f_lamp) < 1e-12  # the lamp covers the block exactly
        total = (w.env.texels * F[:, :, None]).sum((0, 1)) - block
    else:
        w = et.world(crt, name[len("lamp_"):])
        m = w.d.materials
        m["kind"][1], m["color"][1], m["param"][1] = lt.LIGHT, LE_COLOR, LE_PARAM
        total = w.irradiance()  # the roof's block left out, or the ball's share subtracted
        if w.occluder[0] == "roof":
            v = np.array(w.d.objects["v"][1][:9], np.float64)
            f_lamp = polygon_factor(lt.quad_vertices(v[:3], v[3:6], v[6:9]), w.o, w.n)
        else:
            _, c, r, _ = w.occluder
            f_lamp = sphere_factor(c, r, w.o, w.n)
    want = np.asarray(et.RHO) * (total + np.asarray(LE) * f_lamp)
    return w, want


# (world, sampled) -> (sd / mean, log2 N); tests/test_lighting_truth.py prints and holds them
RATIO = {
    ("lamp_roof", True): (0.470, 16), ("lamp_roof", False): (0.473, 16),
    ("lamp_ball", True): (0.593, 17), ("lamp_ball", False): (0.606, 17),
    ("lamp_ball_spheres", True): (0.593, 17), ("lamp_ball_spheres", False): (0.606, 17),
    # under the plain map the one bright texel is found by chance alone: 1 % would take 2^27 paths, so the cap
    # (2^22) holds and 5 standard errors are there about 4.3 % of the mean
    ("lamp_sun", True): (0.2264, 14), ("lamp_sun", False): (17.555, 22),
}


# ---- where no closed form exists: the lit estimator against the unlit one ------------------------------
# Plan worlds (every fifth object a light) under env_truth.random_map (n = 8, NEAREST): truth is the estimator
# that samples nothing, radiance(env=plain), which the oracle holds; the lit call (the map sampled or plain, with
# the lights) must agree with it in the mean. Rays: env_cases.ray_set's 1536 repeated, plan_worlds.DEPTH.
PLAN_WORLDS = ["cloud-300", "mixed-278"]
SEED0, SEED1 = 7300, 7301  # two seeds: the two means are independent, as the combined bound assumes
N2 = 1 << 12


def plan_world(crt, name):
    """(SceneData, GpuScene keywords, oracle keywords, the 1536 rays, the map's env_model.Env)."""
    import env_cases as ec
    import env_model as em
    import plan_worlds as pw
    family, k = name.split("-")
    d, kw = pw.world(crt, family, int(k))
    return d, kw, ec.bvh_of(family), ec.ray_set(crt, family, int(k))[0], em.make(et.random_map(8), filter=em.NEAREST)


# (world, sampled) -> (sqrt(sd0^2 + sd1^2) / m0 of the unlit (0) and the lit (1) model, the largest channel, over
#                      2^12 paths of seeds 7300 and 7301; log2 of the smallest N with 5 * ratio / sqrt(N) <= 2 %)
RATIO2 = {
    ("cloud-300", True): (0.9830, 16), ("cloud-300", False): (0.9833, 16),
    ("mixed-278", True): (0.9748, 16), ("mixed-278", False): (0.9738, 16),
}
