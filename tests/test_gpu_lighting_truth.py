"""The lit estimator on the GPU against closed-form truth (tests/lighting_truth.py, which restates nothing of
the model): the mean of N depth-2 paths from one floor point under a map and a lamp is
rho * (sum L F + Le F_lamp) within 5 standard errors, the project's rule, for four worlds, each under a
sampled and under a plain map. N is lighting_truth.RATIO's: the smallest power of two at which 5 standard
errors are 1 % of the mean by the model's per-path sd on 2^14 paths (tests/test_lighting_truth.py), capped
at 2^22 (lamp_sun under a plain map: 5 se are about 4 % there). The device's own noise is held to the
model's within test_gpu_light_truth.SLACK. Seed 7200, the first and only one tried.

Where no closed form exists (plan worlds cloud 300 and mixed 278 under env_truth.random_map, every fifth object
a light, env_cases.ray_set's 1536 rays repeated, plan_worlds.DEPTH) truth is the estimator that samples
nothing, radiance(env=plain), which the oracle holds elsewhere: the lit call's mean (the map sampled or plain,
with the lights; another seed, so the two means are independent) agrees with it within 5 combined standard
errors, at the N where those are 2 % of the unlit mean by both models' per-path sd on 2^12 paths
(lighting_truth.RATIO2: 2^16). Seeds 7300 and 7301, the first and only ones tried.

Measured on an MI355X (z of the three channels; the device's largest sd / mean): lamp_roof sampled 1.43, -0.57,
1.34, 0.470; plain 1.62, -1.20, 0.60, 0.476; lamp_ball and lamp_ball_spheres (the same bits) sampled 1.04,
0.78, 0.16, 0.600; plain 0.10, 0.36, 0.23, 0.609; lamp_sun sampled 0.22, 0.22, 0.22, 0.228; plain 1.50, 1.50,
1.50, 18.59. Plan worlds (z; 5 combined se / unlit mean): cloud-300 sampled -0.58, -0.08, 0.46 and plain -0.29,
0.14, 0.57, 1.5 to 1.9 %; mixed-278 sampled -0.11, 0.14, -0.06 and plain -0.16, 0.23, -0.04, 1.4 to 1.9 %.

The largest call is 2^22 paths at depth 2. Outputs are pre-filled with 0xFF bytes and followed by a sentinel
tail (test_gpu_lighting.run); every scene's parity guard count is 0 afterwards and it is closed in the test."""
import math

import numpy as np
import pytest

import lighting_truth as ltr
import plan_worlds as pw
import test_gpu_env as tge
import test_gpu_env_nee as tgn
import test_gpu_lighting as tgl
from test_gpu_light_truth import SLACK, moments, opened
from test_gpu_radiance import guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
SEED = 7200


@pytest.mark.parametrize("sampled", [True, False])
@pytest.mark.parametrize("name", ltr.WORLDS)
def test_the_kernels_mean_is_the_closed_form(crt, name, sampled):
    ratio, log2n = ltr.RATIO[name, sampled]
    n = 1 << log2n
    assert log2n <= 22 and (5 * ratio / math.sqrt(n) <= 0.01 or log2n == 22)
    w, want = ltr.world(crt, name)
    with opened(crt, w.d) as s:
        assert w.spheres_only == (s.launch_plan("radiance").prim_mode == 0)  # the sphere-only instances, or not
        lit = crt.Lighting(env=tgn.device_env(crt, w.env, w.basis, importance=sampled), lights=s.light_sampler(0))
        got = tgl.run(crt, s, w.rays(n), None, 2, lit, bg=ltr.et.BG, t_min=ltr.et.T_MIN, base_seed=SEED)
        del lit
    mean, se = moments(got, n)
    print(f"{name} sampled={sampled}: N = 2^{log2n}, want {want.tolist()}, mean {mean.tolist()}, se {se.tolist()}, "
          f"z {((mean - want) / se).tolist()}, sd / mean {(se * math.sqrt(n) / mean).tolist()}")
    assert (np.abs(mean - want) <= 5 * se).all()
    if log2n < 22:  # the device's noise is the model's; not where N is capped: there a path sees the bright texel about
        # once in a thousand, so the sd of 2^14 paths has a relative standard error of some 40 % (sqrt(kurtosis / n))
        assert (5 * se <= SLACK * (5 * ratio / math.sqrt(n)) * np.abs(want)).all()


@pytest.mark.parametrize("sampled", [True, False])
@pytest.mark.parametrize("name", ltr.PLAN_WORLDS)
def test_lit_and_unlit_means_agree_on_plan_worlds(crt, name, sampled):
    ratio, log2n = ltr.RATIO2[name, sampled]
    n = 1 << log2n
    assert log2n <= 22 and 5 * ratio / math.sqrt(n) <= 0.02
    d, kw, _, rays, menv = ltr.plan_world(crt, name)
    rays = np.ascontiguousarray(np.resize(rays, (n, 6)))
    with opened(crt, d, **kw) as s:
        plain_env = tgn.device_env(crt, menv, {}, importance=False)
        lit = crt.Lighting(env=tgn.device_env(crt, menv, {}, importance=sampled), lights=s.light_sampler(0))
        flat = tge.run(s, rays, None, pw.DEPTH, plain_env, bg=ltr.et.BG, t_min=ltr.et.T_MIN, base_seed=ltr.SEED0)
        got = tgl.run(crt, s, rays, None, pw.DEPTH, lit, bg=ltr.et.BG, t_min=ltr.et.T_MIN, base_seed=ltr.SEED1)
        del lit
    (m0, se0), (m1, se1) = moments(flat, n), moments(got, n)
    se = np.sqrt(se0 ** 2 + se1 ** 2)
    print(f"{name} sampled={sampled}: N = 2^{log2n}, unlit {m0.tolist()} (se {se0.tolist()}), lit {m1.tolist()} (se {se1.tolist()}), "
          f"z {((m1 - m0) / se).tolist()}, 5 combined se / unlit mean {(5 * se / m0).tolist()}")
    assert (np.abs(m0 - m1) <= 5 * se).all()
    assert (5 * se <= SLACK * (5 * ratio / math.sqrt(n)) * m0).all()  # the device's noise is the models'
