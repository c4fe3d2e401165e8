"""CPU checks of the ray-query tests' inputs (tests/ray_sets.py): every (scene, set) pair the GPU
tests use has hits and misses in the oracle, so no comparison there is vacuous; and the ray
classification the query kernels start with (csrc/crt_ray_class.h), compiled for the host."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import ray_sets as rs
from conftest import ROOT

# the (primary hit, secondary hit, shadow occluded) shares measured when the sets were chosen
MEASURED = {"rtow_final": (0.85, 0.53, 0.85), "cornell": (0.61, 0.75, 0.44), "christmas_tree": (0.75, 0.07, 0.10)}


@pytest.mark.parametrize("name", list(rs.SCENE_SETS))
def test_every_set_has_hits_and_misses(crt, name):
    d, kw, sets, want = rs.world(crt, name)
    assert set(sets) == set(rs.SCENE_SETS[name])
    for k, calls in sets.items():
        assert all(len(c.rays) == len(w) for c, w in zip(calls, want[k])) and sum(len(c.rays) for c in calls) >= 2000
        share = rs.hit_share(want[k])
        print(name, k, "hit share", round(share, 3))
        assert 0.05 <= share <= 0.95, (name, k, share)
    if name in MEASURED:
        for k, m in zip("ABC", MEASURED[name]):  # the generators are seeded: the shares are reproducible
            assert abs(rs.hit_share(want[k]) - m) < 0.01, (name, k)


def test_set_shapes(crt):
    d, kw, sets, want = rs.world(crt, "rtow_final")
    a, b, c, dd = sets["A"][0], sets["B"][0], sets["C"][0], sets["D"][0]
    assert a.rays.shape == (96 * 64, 6) and dd.rays.shape == (20_000, 6)
    assert len(b.rays) == len(c.rays) == int((want["A"][0]["prim"] >= 0).sum())
    assert set(np.unique(c.tmax)) == {0.5, 1.0, 2.0, math.inf}
    assert len(sets["E"]) == 6 and all(len(e.rays) == 4096 for e in sets["E"])
    z = (dd.rays[:, 3:] == 0).any(1)
    assert z[:1000].all() and not z[1000:].any()


@pytest.fixture(scope="module")
def classify(tmp_path_factory):
    so = tmp_path_factory.mktemp("ray_class") / "ray_class_check.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                        f"-I{ROOT / 'cpp_raytracer_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "ray_class_check.cpp"),
                        "-o", str(so)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(so))
    f, g = lib.ray_class_traceable, lib.ray_class_interval_open
    f.argtypes, f.restype = [C.POINTER(C.c_double), C.c_double], C.c_int
    g.argtypes, g.restype = [C.c_double, C.c_double], C.c_int

    def classify(ray, tmax):
        return bool(f((C.c_double * 6)(*ray), tmax))
    classify.interval_open = lambda t_min, t_max: bool(g(t_min, t_max))
    return classify


def test_ray_classification(classify):
    inf, nan, den = math.inf, math.nan, 5e-324
    ok = [0.5, -2.0, 3.0, 0.1, -0.2, 1.0]
    assert classify(ok, inf) and classify(ok, -inf) and classify(ok, 0.0) and classify(ok, -3.5)
    assert not classify(ok, nan)
    for k in range(6):
        for v in (inf, -inf, nan):
            r = list(ok)
            r[k] = v
            assert not classify(r, 1.0), (k, v)
    for z in ([0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 0.0]):
        assert not classify(ok[:3] + z, 1.0)
    # one non-zero component is a direction, a denormal one too; zero and denormal origins are fine
    for k in range(3):
        for v in (1.0, -den, den, 1e308):
            z = [0.0, -0.0, 0.0]
            z[k] = v
            assert classify(ok[:3] + z, 1.0), (k, v)
    assert classify([0.0, -0.0, den, den, -den, den], den)
    assert classify([1.7e308, -1.7e308, 0.0, 1e-320, 0.0, 0.0], 1e308)
    for name, ray, tmax in rs.invalid_rays():
        assert not classify(ray, tmax), name


def test_empty_intervals_are_not_traced(classify):
    inf, den = math.inf, 5e-324
    for t_min, t_max in [(1e-5, inf), (-1.0, 0.0), (0.0, den), (-den, 0.0), (-2.0, -1.0), (1e6, 1e6 + 1), (-0.0, den)]:
        assert classify.interval_open(t_min, t_max), (t_min, t_max)
    for t_min, t_max in [(1e-5, 1e-5), (1e-5, 0.0), (0.0, -0.0), (-0.0, 0.0), (-2.0, -inf), (-2.0, -2.0 ** 120), (5.0, 4.0),
                         (1e6, 3.0), (0.0, math.nan)]:
        assert not classify.interval_open(t_min, t_max), (t_min, t_max)
