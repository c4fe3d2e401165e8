"""tests/probe_model.py checked on its own, without a GPU: the constants of the basis, the band
factors of sh_eval, the reduction's order on sums whose value is known, and the hemisphere generator's
directions. tests/test_gpu_probes.py then holds the kernels to this model bit for bit."""
import math

import numpy as np
import pytest

import probe_model as pm


def quadrature():
    """Product quadrature on the sphere: Gauss-Legendre in z (32 nodes), uniform in phi (64): exact for
    polynomials of degree <= 63 in z and <= 63 in (x, y), far above the degree 4 of Y_k * Y_l."""
    z, wz = np.polynomial.legendre.leggauss(32)
    phi = (np.arange(64) + 0.5) * (2 * math.pi / 64)
    s = np.sqrt(1 - z * z)
    d = np.stack([s[:, None] * np.cos(phi), s[:, None] * np.sin(phi), np.broadcast_to(z[:, None], (32, 64))], -1)
    return d.reshape(-1, 3), np.repeat(wz * (2 * math.pi / 64), 64)


def test_basis_is_orthonormal():
    d, w = quadrature()
    Y = pm.basis(d)
    gram = (Y * w[:, None]).T @ Y
    assert np.abs(gram - np.eye(9)).max() <= 1e-12, gram


def test_band_factors_and_weights_are_the_header_literals():
    assert pm.A_IRRADIANCE == (math.pi,) + (2 * math.pi / 3,) * 3 + (math.pi / 4,) * 5
    assert (pm.W_SPHERE, pm.W_HEMISPHERE) == (4 * math.pi, math.pi)
    from conftest import ROOT
    text = (ROOT / "include" / "crt_render.h").read_text()
    for v in (pm.A_IRRADIANCE[0], pm.A_IRRADIANCE[1], pm.A_IRRADIANCE[4], pm.W_SPHERE, pm.C0, pm.C1, pm.C2, pm.C6, pm.C8):
        assert repr(v) in text, v


@pytest.mark.parametrize("B", [1.0, 0.35, 15.0])
def test_irradiance_of_constant_radiance(B):
    """Constant radiance B projects to c_0 = B * sqrt(4 pi) and nothing else; a surface under it
    receives pi * B from every side."""
    c = np.zeros((1, 9, 3))
    c[0, 0] = B / pm.C0  # the integral of B * Y0 over the sphere = B * 4 pi * Y0 = B / Y0
    dirs = quadrature()[0][::97]
    got = pm.sh_eval(c, np.zeros(len(dirs), np.uint32), dirs, irradiance=True)
    assert np.abs(got / (math.pi * B) - 1).max() <= 1e-14
    assert np.abs(pm.sh_eval(c, np.zeros(len(dirs), np.uint32), dirs) / B - 1).max() <= 1e-14


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("W", [pm.W_SPHERE, pm.W_HEMISPHERE])
def test_reduction_of_ones(S, W):
    got = pm.reduce_terms(np.ones((3, S, 2, 3)), W)
    assert got.shape == (3, 2, 3)
    assert (got == float(S) * (W / float(S))).all()


def test_reduction_order_is_lane_strided():
    """Terms whose sum depends on the order: 2^53 at sample 0, ones elsewhere, S = 130. Lane 0 adds
    samples 0, 64, 128, so two ones are lost to 2^53 there; lane 1 holds 3, every other lane 2, and the
    tree brings them to lane 0 as exact even partial sums until the last step adds 65: 2^53 + 127,
    a tie that rounds to 2^53 + 128. A sum in sample order would lose every one and give 2^53."""
    S = 130
    t = np.ones((1, S, 1, 1))
    t[0, 0] = 2.0 ** 53
    lanes = [sum([float(t[0, s, 0, 0]) for s in range(l, S, 64)], 0.0) for l in range(64)]
    assert lanes[:3] == [2.0 ** 53, 3.0, 2.0]
    step = 32
    while step:
        lanes = [lanes[l] + lanes[l + step] for l in range(step)] + lanes[step:]
        step //= 2
    got = pm.reduce_terms(t, float(S))[0, 0, 0]  # weight / S = 1
    assert got == lanes[0] == 2.0 ** 53 + 128
    assert sum([float(v) for v in t[0, :, 0, 0]], 0.0) == 2.0 ** 53


def test_hemisphere_directions_point_into_the_normals_half(crt):
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(100, 3))
    nrm /= np.sqrt((nrm * nrm).sum(1))[:, None]
    rays, states = pm.rays(crt, rng.normal(size=(100, 3)), nrm, 100, base_seed=9)
    assert rays.shape == (10000, 6) and states.dtype == np.uint32
    d = rays[:, 3:].reshape(100, 100, 3)
    assert ((d * nrm[:, None, :]).sum(-1) >= 0).all()
    u = d - nrm[:, None, :]
    assert np.abs((u * u).sum(-1) - 1).max() < 1e-12


def test_sphere_directions_are_the_unit_vectors_of_the_seeds(crt):
    """Record p * S + s starts from sample_seed(base, p, s), whatever came before it."""
    pts = np.arange(9.0).reshape(3, 3)
    rays, states = pm.rays(crt, pts, None, 4, base_seed=3)
    st, u = pm.unit_vector(crt, crt.sample_seed(3, 2, 1))
    assert list(rays[2 * 4 + 1]) == list(pts[2]) + u and states[2 * 4 + 1] == st
    again, _ = pm.rays(crt, pts[1:], None, 4, base_seed=3, first_probe=1)
    assert np.array_equal(again, rays[4:])


def test_sh_eval_model_zeroes_an_index_past_the_probes():
    c = np.ones((2, 9, 3))
    got = pm.sh_eval(c, np.array([0, 2, 1, 0xFFFFFFFF], np.uint32), np.tile([0.0, 0.0, 1.0], (4, 1)))
    assert (got[[1, 3]] == 0).all() and (got[[0, 2]] != 0).all()
