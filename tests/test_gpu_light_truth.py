"""The lights instances of the radiance kernels on the GPU, held to truth that is no restatement of them
(tests/light_truth.py): closed-form irradiance, and the unsampled estimator, which samples no light and is
held to the oracle elsewhere. Statistics, not bits: tests/test_gpu_light_nee_edges.py holds the same
worlds to the model bit for bit.

  1. closed forms  one sampled call of N paths of the world's one ray at depth 2, fast route, states
                   sample_seed(SEED, i, 0): per channel |mean - rho Le F| <= 5 standard errors, the standard
                   error from the same N values (test_light_nee_model.py's bound rule). N is the smallest
                   power of two with 5 * (sd / mean) / sqrt(N) <= 1 %, sd / mean the model's, measured
                   without a GPU on 2^14 paths (light_truth.RATIO, held by tests/test_light_truth.py), so a
                   bias of 1 % of the mean and more fails, and the condition is asserted on that ratio:
                       solid 1.616 -> 2^20   hollow 1.616 -> 2^20   skew 0.428 -> 2^16
                       skew_back 0.430 -> 2^16   box 1.420 -> 2^19   zero_mate 3.030 -> 2^22
  2. domes         4096 paths, both routes: every path is (1 * rho_k) * Le_k bit for bit
  3. sampled against unsampled on stacked and bulb (depth 2) and the plan worlds cloud-300, mixed-278 and
                   flat-40 (env_cases.ray_set's 1536 rays repeated, plan_worlds.DEPTH), background 0: two
                   GPU calls with the same rays and N, lights=None and the scene's sampler, base seeds SEED0
                   and SEED1 (two seeds, so that the two means are independent as the bound assumes):
                   per channel |m0 - m1| <= 5 * sqrt(se0^2 + se1^2). N is the smallest power of two at which
                   that bound is at most 2 % of the unsampled mean, from both models' per-path sd on 2^12
                   paths without a GPU (light_truth.RATIO2: sqrt(sd0^2 + sd1^2) / m0):
                       stacked 2.973 -> 2^20   bulb 5.991 -> 2^22   cloud-300 2.873 -> 2^19
                       mixed-278 3.121 -> 2^20   flat-40 3.482 -> 2^20
                   At depth 2 bulb's glass shell ends every path that meets it, so bulb_deep adds the same
                   world at depth 8 (4.695 -> 2^21): there more than half of the mean is the light in the
                   shell, found only through glass, with pb none and f = 1.
                   Both conditions are asserted on the recorded ratios. The device's own noise is held to
                   them too, within SLACK: a per-path sd measured on 2^12 to 2^14 values whose kurtosis is
                   of order 30 (most paths give 0, few give much) has a relative standard error of about
                   sqrt(30 / 4n), 4 % at 2^12; five of those are 20 %, so 1.25.

Seeds: SEED = 5100, SEED0 = 5200, SEED1 = 5201: each the first and only one tried. Measured on an MI355X
(z of the three channels; the device's own sd / mean or 5 combined se / unsampled mean): solid and hollow
-0.53, 1.605; skew -1.04, 0.429; skew_back -0.30, 0.427; box -0.82, 1.429; zero_mate -0.81, 0.78, -0.81,
2.710; stacked -0.17, 1.44 %; bulb 0.06, 1.34 %; bulb_deep -0.07 to -0.05, 1.49 %; cloud-300 -0.13 to -0.06, 1.99 %; mixed-278 -0.13 to -0.06,
1.52 %; flat-40 0.02 to 0.04, 1.70 %. The plan worlds' z is small because most of their per-path sd is the
spread between the 1536 rays, which both calls share: the bound is conservative there.

The largest call is 2^22 paths (bulb and zero_mate at depth 2); the plan worlds' largest is 2^20 at depth 8.
Outputs are pre-filled with 0xFF bytes and followed by a sentinel tail (test_gpu_light_nee.run); every
scene's parity guard count is 0 afterwards and it is closed in the test."""
import contextlib
import math

import numpy as np
import pytest

import env_cases as ec
import light_truth as lt
import plan_worlds as pw
import test_gpu_light_nee as tgl
from test_gpu_radiance import bits, guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
SEED, SEED0, SEED1 = 5100, 5200, 5201
PLAIN = tgl.PLAIN
SLACK = 1.25
STATISTICAL = [w for w in lt.CLOSED if not w.startswith("dome")]


@contextlib.contextmanager
def opened(crt, d, **kw):
    s = crt.GpuScene(d, **kw)
    try:
        s.upload(0)
        yield s
        assert s.guard(0) == 0
    finally:
        s.close()


def moments(x, n):
    m = x.mean(0)
    return m, x.std(0, ddof=1) / math.sqrt(n)


# ---- 1. closed forms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STATISTICAL)
def test_the_kernels_mean_is_the_closed_form(crt, name):
    ratio, log2n = lt.RATIO[name]
    n = 1 << log2n
    assert log2n <= 22 and 5 * ratio / math.sqrt(n) <= 0.01  # a bias of 1 % of the mean cannot hide in the noise
    w = lt.world(crt, name)
    want = w.expected()
    with opened(crt, w.d) as s:
        smp = s.light_sampler(0)
        got = tgl.run(s, w.rays(n), None, 2, smp, bg=lt.BG, t_min=lt.T_MIN, base_seed=SEED)
        del smp
    mean, se = moments(got, n)
    print(f"{name}: N = 2^{log2n}, F = {w.factors()}, rho Le F = {want.tolist()}, mean {mean.tolist()}, se {se.tolist()}, "
          f"z {((mean - want) / se).tolist()}, sd / mean {(se * math.sqrt(n) / mean).tolist()}")
    assert (np.abs(mean - want) <= 5 * se).all()
    assert (5 * se <= SLACK * (5 * ratio / math.sqrt(n)) * np.abs(want)).all()  # the device's noise is the model's


# ---- 2. the domes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dome", "dome_hollow"])
def test_from_inside_a_sphere_every_path_is_exact(crt, name):
    w = lt.world(crt, name)
    n = 4096
    one = np.broadcast_to([(1.0 * lt.RHO[k]) * (lt.COLOR[k] * lt.PARAM) for k in range(3)], (n, 3))
    with opened(crt, w.d) as s:
        smp = s.light_sampler(0)
        for flags in (0, PLAIN):
            got = tgl.run(s, w.rays(n), None, 2, smp, bg=lt.BG, t_min=lt.T_MIN, flags=flags, base_seed=SEED)
            assert np.array_equal(bits(got), bits(one)), (name, flags, got[:3])
        del smp


# ---- 3. sampled against unsampled ----------------------------------------------------------------------
@pytest.mark.parametrize("name", lt.OPEN + list(lt.DEEP) + lt.PLAN_WORLDS)
def test_sampled_and_unsampled_means_agree(crt, name):
    ratio, log2n = lt.RATIO2[name]
    n = 1 << log2n
    assert log2n <= 22 and 5 * ratio / math.sqrt(n) <= 0.02
    if name in lt.OPEN or name in lt.DEEP:
        world, depth = lt.DEEP.get(name, (name, 2))
        w = lt.world(crt, world)
        d, kw, rays = w.d, {}, w.rays(n)
    else:
        family, k = name.split("-")
        d, kw = pw.world(crt, family, int(k))
        rays = np.ascontiguousarray(np.resize(ec.ray_set(crt, family, int(k))[0], (n, 6)))
        depth = pw.DEPTH
    with opened(crt, d, **kw) as s:
        smp = s.light_sampler(0)
        flat = tgl.run(s, rays, None, depth, None, bg=lt.BG, t_min=lt.T_MIN, base_seed=SEED0)
        nee = tgl.run(s, rays, None, depth, smp, bg=lt.BG, t_min=lt.T_MIN, base_seed=SEED1)
        del smp
    (m0, se0), (m1, se1) = moments(flat, n), moments(nee, n)
    se = np.sqrt(se0 ** 2 + se1 ** 2)
    print(f"{name}: N = 2^{log2n}, unsampled {m0.tolist()} (se {se0.tolist()}), sampled {m1.tolist()} (se {se1.tolist()}), "
          f"z {((m1 - m0) / se).tolist()}, 5 combined se / unsampled mean {(5 * se / m0).tolist()}")
    assert (np.abs(m0 - m1) <= 5 * se).all()
    assert (5 * se <= SLACK * (5 * ratio / math.sqrt(n)) * m0).all()
