"""crt_sh_eval_async's model (probe_model.sh_eval) held to what irradiance means, without a GPU: the
irradiance at a surface with normal n of the radiance field Y_k is the integral of Y_k(d) max(0, n . d) over the
sphere (Funk-Hecke: A_band Y_k(n)). The integral is taken in n's own frame, Gauss-Legendre on t = n . d in [0, 1]
(16 nodes) times a uniform rule in azimuth (32 nodes): the integrand is a polynomial of degree 3 in t and the
azimuth's harmonics stop at 2, so both rules are exact and the result is the integral to rounding. The basis is
env_truth.sh_basis, written from square roots; nothing here reads probe_model's or the header's literals.
tests/test_gpu_lens_truth.py runs the same comparison on the kernel."""
import math

import numpy as np
import pytest

import env_truth as et
import probe_model as pm

SEED = 7300        # the normals: the first and only seed tried
TOL_IRRADIANCE, TOL_RADIANCE = 1e-13, 1e-14   # the model's largest errors are 1.44e-15 and 1.11e-16


def normals(m=50, seed=SEED):
    v = np.random.default_rng(seed).normal(size=(m, 3))
    return v / np.sqrt((v * v).sum(1))[:, None]


def clamped_cosine_integrals(n):
    """(m, 9): the integral over the sphere of Y_k(d) max(0, n . d) for unit normals n (m, 3)."""
    t, wt = np.polynomial.legendre.leggauss(16)
    t, wt = 0.5 * (t + 1), 0.5 * wt
    phi = 2 * math.pi * (np.arange(32) + 0.5) / 32
    out = np.empty((len(n), 9))
    for i, nn in enumerate(n):
        e1 = np.cross(nn, [1.0, 0.0, 0.0] if abs(nn[0]) < 0.9 else [0.0, 1.0, 0.0])
        e1 /= math.sqrt(float(e1 @ e1))
        e2 = np.cross(nn, e1)
        T, P = (x.reshape(-1) for x in np.meshgrid(t, phi, indexing="ij"))
        W = np.repeat(wt, len(phi)) * (2 * math.pi / len(phi))
        s = np.sqrt(1 - T * T)
        d = np.outer(T, nn) + np.outer(s * np.cos(P), e1) + np.outer(s * np.sin(P), e2)
        out[i] = (et.sh_basis(d) * (W * T)[:, None]).sum(0)
    return out


def one_hot_queries(n):
    """(coeff (9, 9, 3): probe k holds 1 in coefficient k, every channel; index and dirs: every probe at every n)."""
    coeff = np.zeros((9, 9, 3))
    for k in range(9):
        coeff[k, k, :] = 1.0
    return coeff, np.repeat(np.arange(9), len(n)).astype(np.int32), np.tile(n, (9, 1))


def check(sh_eval, label=""):
    """sh_eval(coeff, index, dirs, irradiance) -> (m, 3), the model's or the kernel's."""
    n = normals()
    want = clamped_cosine_integrals(n)
    coeff, index, dirs = one_hot_queries(n)
    got = np.asarray(sh_eval(coeff, index, dirs, True)).reshape(9, len(n), 3)
    err = float(np.abs(got - want.T[:, :, None]).max())
    plain = np.asarray(sh_eval(coeff, index, dirs, False)).reshape(9, len(n), 3)
    err0 = float(np.abs(plain - et.sh_basis(n).T[:, :, None]).max())
    print(f"{label}largest |irradiance - integral| = {err:.3g}, largest |radiance - Y_k(n)| = {err0:.3g}")
    assert err <= TOL_IRRADIANCE, err
    assert err0 <= TOL_RADIANCE, err0
    return err, err0


def test_the_quadrature_is_the_integral():
    """Band 0 along any normal is Y0 * pi; the integral of Y_2 (z) along n = z is sqrt(3 / (4 pi)) * 2 pi / 3;
    band 2's zonal function integrates (3 t^2 - 1) t; the others vanish by symmetry."""
    z = np.array([[0.0, 0.0, 1.0]])
    got = clamped_cosine_integrals(z)[0]
    assert abs(got[0] - et.Y0 * math.pi) < 1e-14 and abs(got[2] - math.sqrt(3 / (4 * math.pi)) * 2 * math.pi / 3) < 1e-14
    assert np.abs(got[[1, 3, 4, 5, 7, 8]]).max() < 1e-14
    assert abs(got[6] - 0.25 * math.sqrt(5 / math.pi) * 2 * math.pi * (3 / 4 - 1 / 2)) < 1e-14  # int of (3 t^2 - 1) t


def test_the_models_irradiance_is_the_clamped_cosine_integral():
    check(pm.sh_eval, "model: ")


@pytest.mark.parametrize("band,wrong", [(1, math.pi / 2), (2, math.pi / 8)])
def test_a_wrong_band_factor_is_caught(band, wrong, monkeypatch):
    a = list(pm.A_IRRADIANCE)
    for k in ((1, 2, 3) if band == 1 else (4, 5, 6, 7, 8)):
        a[k] = wrong
    monkeypatch.setattr(pm, "A_IRRADIANCE", tuple(a))
    with pytest.raises(AssertionError):
        check(pm.sh_eval)
