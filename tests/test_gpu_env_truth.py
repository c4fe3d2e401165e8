"""The sampled-environment instances of the radiance kernels on the GPU, held to truth that is no restatement
of them (tests/env_truth.py): the closed-form irradiance of a cube map's texels, the quadrature of the lookup
under BILINEAR, and the unsampled estimator. Statistics, not bits: tests/test_gpu_env_nee_edges.py holds the
same worlds to the model bit for bit.

  1. closed forms  one crt_radiance_env_sampled_async call of N paths of the world's one ray at depth 2, fast
                   route, states sample_seed(SEED, i, 0): per channel |mean - rho sum L F| <= 5 standard errors,
                   the standard error from the same N values. N is the smallest power of two with
                   5 * (sd / mean) / sqrt(N) <= 1 %, sd / mean the model's on 2^14 paths without a GPU
                   (env_truth.RATIO, held by tests/test_env_truth.py); the condition is asserted on that ratio:
                       random 0.615 -> 2^17   tilted 0.609 -> 2^17   sun 0.229 -> 2^14   sun_horizon 1.248 -> 2^19
                       half_black 0.906 -> 2^18   under 0.584 -> 2^17   roof 0.740 -> 2^18   ball 0.683 -> 2^17
                       random_bilinear 0.489 -> 2^16   sun_bilinear 1.103 -> 2^19   the all-sphere variants as
                       their namesakes
                   The device's own noise is held to the ratio within SLACK = 1.25 (a per-path sd measured on
                   2^14 values of high kurtosis has a relative standard error of a few per cent; five of those).
  2. unsampled     random, tilted and under through crt_radiance_env_async against the same truth; there a
                   path is rho L(d) with d drawn by cosine, so sd / mean is env_truth.cosine_ratio, a closed
                   form, and N follows from it by the same rule (2^17 each)
  3. glass         sampled against unsampled at depths 2 and 8 (at 8 a quarter of the paths leave through the
                   glass with pb none), base seeds SEED0 and SEED1 so that the two means are independent:
                   |m0 - m1| <= 5 * sqrt(se0^2 + se1^2), N the smallest power of two at which that is at most
                   2 % of the unsampled mean (env_truth.RATIO2: 1.260 -> 2^17, 0.856 -> 2^16)
  4. hemisphere    a HEMISPHERE bake at max_depth 1 of one probe above random's and tilted's floor point is
                   pi * sum L F within 5 standard errors, the standard error pi * sd / sqrt(S) with sd the
                   closed form env_truth.cosine_moments and S = 2^17 by the same rule
  5. sphere        a SPHERE bake at max_depth 1 of a point in the floor's own plane beside it (no direction of
                   positive measure meets the floor): c_0 against Y0 * sum L * solid angle, c_1 .. c_8 against
                   the texels' SH integrals by quadrature_texel, each within 5 standard errors, the per-sample
                   sd from env_truth.sphere_moments; S = 2^17 from band 0's ratio

Seeds: SEED = 6500, SEED0 = 6600, SEED1 = 6601, PROBE_SEED = 6700: each the first and only one tried; every
comparison passed at the first run. Measured on an MI355X (z of the three channels; the device's own sd / mean,
the largest channel): random and random_spheres -1.11, -0.72, -1.13; 0.619. tilted -1.15, -1.12, -0.29; 0.613.
sun -0.15; 0.231. sun_horizon and sun_horizon_spheres 0.34; 1.252. half_black 0.50, 0.69, -0.45; 0.914. under
1.60, 1.86, 1.73; 0.589. roof 1.42, 0.45, 0.24; 0.739. ball and ball_spheres 0.88, -0.57, -0.28; 0.684.
random_bilinear -2.16, 0.45, -1.02; 0.491. sun_bilinear -0.22; 1.112. Unsampled: random -0.26, 2.02, 0.64; 0.621
(closed form 0.620). tilted 0.04, 1.43, 2.26; 0.615 (0.615). under 0.28, 0.83, -0.21; 0.587 (0.587). Glass: depth 2
z -2.11, -1.24, -0.82, 5 combined se 1.73 % of the unsampled mean; depth 8 z -2.40, -0.29, 0.46, 1.66 %.
Hemisphere bakes: random 1.24, -0.14, 0.67; tilted -0.82, -0.93, -0.41. Sphere bake: |z| at most 2.12 over the
27 coefficients, band 0 1.05, 1.70, 1.04.

The largest call is 2^19 paths at depth 2. Outputs are pre-filled with 0xFF bytes and followed by a sentinel
tail (test_gpu_env_nee.run); every scene's parity guard count is 0 afterwards and it is closed in the test."""
import contextlib
import math

import numpy as np
import pytest

import env_truth as et
import test_gpu_env as tge
import test_gpu_env_nee as tgn
from test_gpu_radiance import guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
SEED, SEED0, SEED1, PROBE_SEED = 6500, 6600, 6601, 6700
SLACK = 1.25
STATISTICAL = et.CLOSED + et.BILINEAR + et.SPHERES_ONLY


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
    return x.mean(0), x.std(0, ddof=1) / math.sqrt(n)


# ---- 1. closed forms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STATISTICAL)
def test_the_kernels_mean_is_the_closed_form(crt, name):
    ratio, log2n = et.RATIO[name]
    n = 1 << log2n
    assert log2n <= 22 and 5 * ratio / math.sqrt(n) <= 0.01  # a bias of 1 % of the mean cannot hide in the noise
    w = et.world(crt, name)
    want = w.expected()
    with opened(crt, w.d) as s:
        env = tgn.device_env(crt, w.env, w.basis)
        got = tgn.run(s, w.rays(n), None, 2, env, bg=et.BG, t_min=et.T_MIN, base_seed=SEED)
        del env
    mean, se = moments(got, n)
    print(f"{name}: N = 2^{log2n}, rho sum L F = {want.tolist()}, mean {mean.tolist()}, se {se.tolist()}, "
          f"z {((mean - want) / se).tolist()}, sd / mean {(se * math.sqrt(n) / mean).tolist()}")
    assert (np.abs(mean - want) <= 5 * se).all()
    assert (5 * se <= SLACK * (5 * ratio / math.sqrt(n)) * np.abs(want)).all()  # the device's noise is the model's


# ---- 2. the unsampled entry ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", et.UNSAMPLED_TOO)
def test_the_unsampled_kernels_mean_is_the_closed_form(crt, name):
    w = et.world(crt, name)
    ratio = et.cosine_ratio(w)
    log2n, ok = et.n_for(ratio, 0.01)
    n = 1 << log2n
    assert ok and 5 * ratio / math.sqrt(n) <= 0.01
    want = w.expected()
    with opened(crt, w.d) as s:
        env = tgn.device_env(crt, w.env, w.basis, importance=False)
        got = tge.run(s, w.rays(n), None, 2, env, bg=et.BG, t_min=et.T_MIN, base_seed=SEED)
        del env
    mean, se = moments(got, n)
    print(f"{name} unsampled: N = 2^{log2n}, cosine ratio {ratio:.4f}, mean {mean.tolist()}, z {((mean - want) / se).tolist()}, "
          f"sd / mean {(se * math.sqrt(n) / mean).tolist()}")
    assert (np.abs(mean - want) <= 5 * se).all()
    assert (5 * se <= SLACK * (5 * ratio / math.sqrt(n)) * np.abs(want)).all()


# ---- 3. sampled against unsampled through glass --------------------------------------------------------
@pytest.mark.parametrize("depth", [2, 8])
def test_sampled_and_unsampled_means_agree_through_glass(crt, depth):
    ratio, log2n = et.RATIO2[depth]
    n = 1 << log2n
    assert log2n <= 22 and 5 * ratio / math.sqrt(n) <= 0.02
    w = et.world(crt, "glass")
    with opened(crt, w.d) as s:
        env = tgn.device_env(crt, w.env, w.basis)
        flat = tge.run(s, w.rays(n), None, depth, tgn.device_env(crt, w.env, w.basis, importance=False), bg=et.BG, t_min=et.T_MIN,
                       base_seed=SEED0)
        nee = tgn.run(s, w.rays(n), None, depth, env, bg=et.BG, t_min=et.T_MIN, base_seed=SEED1)
        del env
    (m0, se0), (m1, se1) = moments(flat, n), moments(nee, n)
    se = np.sqrt(se0 ** 2 + se1 ** 2)
    print(f"glass at depth {depth}: N = 2^{log2n}, unsampled {m0.tolist()} (se {se0.tolist()}), sampled {m1.tolist()} (se {se1.tolist()}), "
          f"z {((m1 - m0) / se).tolist()}, 5 combined se / unsampled mean {(5 * se / m0).tolist()}")
    assert (np.abs(m0 - m1) <= 5 * se).all()
    assert (5 * se <= SLACK * (5 * ratio / math.sqrt(n)) * m0).all()


# ---- 4. and 5. probes -----------------------------------------------------------------------------------
def bake(scene, point, normal, log2s, env):
    import torch
    P = torch.tensor([point], dtype=torch.float64, device="cuda")
    Nn = torch.tensor([normal], dtype=torch.float64, device="cuda") if normal is not None else None
    out = scene.probes(P, Nn, samples=1 << log2s, mode="hemisphere" if normal is not None else "sphere", max_depth=1,
                       background=et.BG, t_min=et.T_MIN, base_seed=PROBE_SEED, env=env)
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


@pytest.mark.parametrize("name", ["random", "tilted"])
def test_a_hemisphere_bake_is_pi_times_the_closed_form(crt, name):
    w = et.world(crt, name)
    log2s = et.PROBE_LOG2_S[name]
    m, sd = et.cosine_moments(w)
    assert 5 * float((sd / m).max()) / math.sqrt(1 << log2s) <= 0.01
    want, se = math.pi * m, math.pi * sd / math.sqrt(1 << log2s)
    point = tuple(float(o + 0.5 * k) for o, k in zip(w.o, w.n))
    with opened(crt, w.d) as s:
        sampled = bake(s, point, w.n, log2s, tgn.device_env(crt, w.env, w.basis))
        plain = bake(s, point, w.n, log2s, tgn.device_env(crt, w.env, w.basis, importance=False))
    print(f"{name} hemisphere: S = 2^{log2s}, pi sum L F = {want.tolist()}, bake {sampled[0].tolist()}, z {((sampled[0] - want) / se).tolist()}")
    assert sampled.shape == (1, 3) and tgn.same(sampled, plain)  # one segment: the sampled entry is the unsampled one
    assert (np.abs(sampled[0] - want) <= 5 * se).all()


def test_a_sphere_bake_in_the_open_is_the_texels_sh_integrals(crt):
    w = et.world(crt, "random")
    log2s = et.PROBE_LOG2_S["sphere"]
    m, sd = et.sphere_moments(w.env)
    assert 5 * float((sd[0] / m[0]).max()) / math.sqrt(1 << log2s) <= 0.01
    se = sd / math.sqrt(1 << log2s)
    with opened(crt, w.d) as s:
        got = bake(s, (200.0, 0.0, 0.0), None, log2s, tgn.device_env(crt, w.env, w.basis))
    z = (got - m) / se
    print(f"sphere: S = 2^{log2s}, c_0 {got[0].tolist()} against {m[0].tolist()}, z of the nine bands by channel {np.round(z, 2).tolist()}")
    assert got.shape == (9, 3) and (np.abs(got - m) <= 5 * se).all()
