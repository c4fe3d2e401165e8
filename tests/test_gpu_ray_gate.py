"""The wave-level gate of a traversal set-up's range checks (crt_ray_gate.h, trav_init)
through crt_radiance_async, which traces the caller's own rays: 64 rays, one wave, on a small sphere
scene. As given, every lane passes the gate and the wave takes the checks as known; with ray 63
replaced by a ray outside the gate the whole wave evaluates them one by one, as every set-up used to.
Rays 0-62 must come out bit-identical either way, and both runs must equal the oracle (the
project's bar of 1e-12 relative on a path's radiance). The odd rays:
  one component just past a gate threshold, still inside every old range: a direction component
  under 2^-29, and an origin component that takes the origin's sum over 2^29;
  a zero direction component (the EXACT walk);
  the direction scaled between the gate and each old threshold: under 2^30 (the packed leaf filter's),
  between 2^30 and 2^39 (the f32 walk's), between 2^39 and 2^40, and past 2^40; an origin component
  likewise;
  an infinite origin component and a NaN direction component: outside crt_radiance_async's contract,
  such a path sees the background and never reaches a set-up; its neighbours must not notice."""
import numpy as np
import pytest

import denoise_model as dm
import plan_worlds as pw
from oracle import crt_oracle_py as orc
from test_gpu_radiance import PLAIN, bits, run

pytestmark = pytest.mark.gpu

BG = (0.35, 0.6, 1.25)
DEPTH, T_MIN, BAR = 8, 1e-5, 1e-12
_JOB = {}


def job(crt):
    """(SceneData, resident GpuScene, 64 centre rays of a 16 x 4 camera, states, the oracle's radiance,
    the all-pass run), computed once."""
    if not _JOB:
        from cpp_raytracer_amd import camera_with
        d, _ = pw.world(crt, "cloud", 40)
        objs = d.objects.copy()
        objs["v"][:, 3] = 1.2  # large enough that a quarter of the 64 centre rays hit one
        d.objects = objs
        d.camera = camera_with(d.camera, image_w=16, image_h=4, fov=float(2 * np.arctan(4 / 44)))
        s = crt.GpuScene(d)
        s.upload(0)
        rays = dm.centre_rays(crt.resolve_camera(d.camera, 5)).reshape(-1, 6).copy()
        assert rays.shape == (64, 6)
        states = (np.arange(64, dtype=np.uint64) * 2654435761 + 12345).astype(np.uint32)
        want = orc.radiance(d, rays, states, DEPTH, BG, T_MIN)
        got = run(s, rays, states, DEPTH, BG, T_MIN)
        for a in (rays, states, want, got):
            a.setflags(write=False)
        _JOB.update(d=d, s=s, rays=rays, states=states, want=want, got=got)
    return _JOB


def close(got, want):
    return float(np.abs(got - want).max()) <= BAR * max(1.0, float(np.abs(want).max()))


def test_every_lane_inside_the_gate(crt):
    j = job(crt)
    o, d = np.abs(j["rays"][:, :3]), np.abs(j["rays"][:, 3:])
    assert o.sum(1).max() < 2.0 ** 28 and d.sum(1).max() < 2.0 ** 28 and d.min() > 2.0 ** -28
    hit = np.any(np.abs(j["want"] - np.array(BG)) > 1e-9, axis=1)
    assert 8 <= hit.sum() <= 60  # paths that hit the spheres and paths that do not
    assert close(j["got"], j["want"])
    assert np.array_equal(bits(run(j["s"], j["rays"], j["states"], DEPTH, BG, T_MIN, PLAIN)), bits(j["got"]))
    assert j["s"].guard(0) == 0


def scaled(k):
    def f(r):
        r = r.copy()
        r[3:] *= 2.0 ** k
        return r
    return f


def setc(i, v):
    def f(r):
        r = r.copy()
        r[i] = v
        return r
    return f


ODD = {
    "dir_under_2^-29": (setc(3, 2.0 ** -29 * (1 - 2.0 ** -10)), True),
    "origin_sum_over_2^29": (setc(0, 2.0 ** 29), True),  # + |o_z| = 44
    "zero_dir_component": (setc(3, 0.0), True),
    "negative_zero_dir_component": (setc(4, -0.0), True),
    "dir_under_2^30": (scaled(29.5), True),
    "dir_2^30_to_2^39": (scaled(35), True),
    "dir_2^39_to_2^40": (scaled(39.5), True),
    "dir_past_2^40": (scaled(41), True),
    "origin_2^30_to_2^39": (setc(1, -2.0 ** 35), True),
    "origin_2^39_to_2^40": (setc(1, 2.0 ** 39.5), True),
    "origin_past_2^40": (setc(2, 2.0 ** 41), True),
    "inf_origin_component": (setc(2, np.inf), False),
    "nan_dir_component": (setc(5, np.nan), False),
}


@pytest.mark.parametrize("odd", sorted(ODD))
def test_one_lane_outside_the_gate(crt, odd):
    j = job(crt)
    make, in_contract = ODD[odd]
    rays = j["rays"].copy()
    rays[63] = make(rays[63])
    if odd.startswith("dir_") and "2^" in odd and odd != "dir_under_2^-29":  # the scaled ones: where they should be
        lo, hi = {"dir_under_2^30": (29, 30), "dir_2^30_to_2^39": (30, 39), "dir_2^39_to_2^40": (39, 40),
                  "dir_past_2^40": (40, 60)}[odd]
        assert 2.0 ** lo < np.abs(rays[63, 3:]).max() < 2.0 ** hi
    got = run(j["s"], rays, j["states"], DEPTH, BG, T_MIN)
    assert np.array_equal(bits(got[:63]), bits(j["got"][:63])), "the odd ray's neighbours changed"
    assert np.array_equal(bits(run(j["s"], rays, j["states"], DEPTH, BG, T_MIN, PLAIN)), bits(got))
    if in_contract:
        want = orc.radiance(j["d"], rays, j["states"], DEPTH, BG, T_MIN)
        assert np.array_equal(bits(want[:63]), bits(j["want"][:63]))
        print(f"{odd}: ray 63 gpu {got[63].tolist()} oracle {want[63].tolist()}")
        assert close(got, want)
    else:
        assert close(got[:63], j["want"][:63])
        assert np.array_equal(bits(got[63]), bits(np.array(BG)))
    assert j["s"].guard(0) == 0
