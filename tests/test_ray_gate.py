"""The one gate of a traversal set-up's range checks (cpp_raytracer_amd/csrc/crt_ray_gate.h), as host
code: ray_gate must imply each of the four checks the kernels skip for a wave whose lanes all pass it
(gate_walk_plain, gate_walk_f32, gate_leaf32, gate_recip), on the numbers trav_init feeds them.

  1. 10^6 seeded rays whose six components draw sign, exponent and mantissa bits independently over
     the whole f64 range (denormals, infinities and NaN included), and 10^6 with exponents within
     +-40 of 0, where the gate's own thresholds lie and most rays pass it;
  2. every edge value in every component: each threshold of the gate and of the checks, its f64
     neighbours, its f32 neighbours and the f32 rounding midpoints next to it, both signs, +-0,
     denormals of both formats, +-inf and NaN, one component at a time on a benign ray, all three
     direction (origin) components at once, and 300,000 seeded six-tuples of edge values;
  3. NaN and +-inf in any component fail the gate, whatever the others hold;
  4. the camera rays and the reflected secondaries of rtow_final and cornell (tests/ray_sets.py, sets
     A and B) and the camera rays of millions pass the gate, and so does any ray that starts inside
     three times a scene's extent with direction components of camera or scatter size.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import denoise_model as dm
import ray_sets as rs
from conftest import ROOT

GATE, PLAIN, F32, LEAF32, RECIP = 1, 2, 4, 8, 16
CHECKS = {"gate_walk_plain": PLAIN, "gate_walk_f32": F32, "gate_leaf32": LEAF32, "gate_recip": RECIP}


@pytest.fixture(scope="module")
def classify(tmp_path_factory):
    so = tmp_path_factory.mktemp("ray_gate") / "ray_gate_check.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                        f"-I{ROOT / 'cpp_raytracer_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "ray_gate_check.cpp"),
                        "-o", str(so)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(so))
    lib.ray_gate_classify.argtypes, lib.ray_gate_classify.restype = [C.c_void_p, C.c_size_t, C.c_void_p], None
    lib.ray_gate_max.restype = lib.ray_gate_min_dir.restype = C.c_float

    def classify(rays):
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        out = np.zeros(len(rays), np.uint8)
        lib.ray_gate_classify(rays.ctypes.data, len(rays), out.ctypes.data)
        return out
    classify.max, classify.min_dir = float(lib.ray_gate_max()), float(lib.ray_gate_min_dir())
    return classify


def implied(classify, rays, label):
    """gate => every check; returns the classes."""
    c = classify(rays)
    g = (c & GATE) != 0
    for name, bit in CHECKS.items():
        bad = g & ((c & bit) == 0)
        assert not bad.any(), (label, name, np.asarray(rays).reshape(-1, 6)[np.flatnonzero(bad)[:3]].tolist())
    return c


def random_rays(rng, n, exp_lo, exp_hi):
    """Sign, biased exponent in [exp_lo, exp_hi] and 52 mantissa bits, each uniform."""
    sign = rng.integers(0, 2, (n, 6), dtype=np.uint64) << np.uint64(63)
    exp = rng.integers(exp_lo, exp_hi + 1, (n, 6), dtype=np.uint64) << np.uint64(52)
    man = rng.integers(0, 1 << 52, (n, 6), dtype=np.uint64)
    return (sign | exp | man).view(np.float64)


def test_gate_implies_every_check_on_random_rays(classify):
    rng = np.random.default_rng(20260)
    wide = implied(classify, random_rays(rng, 1_000_000, 0, 2047), "whole range")
    near = implied(classify, random_rays(rng, 1_000_000, 1023 - 40, 1023 + 40), "2^+-40")
    # the wide draw hardly ever passes (six exponents within 59 of 2047 values); the near one does
    # often, and fails often: both sides of the implication are exercised
    passed = int(((near & GATE) != 0).sum())
    assert 50_000 < passed < 950_000, passed
    assert int(((wide & GATE) != 0).sum()) < 1000
    for bit in CHECKS.values():  # every check fails somewhere, and holds somewhere outside the gate
        assert ((wide & bit) == 0).any() and (((near & bit) != 0) & ((near & GATE) == 0)).any()


def edge_values(classify):
    thresholds = [classify.min_dir, classify.max, 2.0 ** 30, 2.0 ** -39, 2.0 ** 39, 2.0 ** 40, 2.0 ** -30, 2.0 ** -60,
                  2.0 ** 60, 2.0 ** -250, 2.0 ** 250, 2.0 ** -500, 2.0 ** 500, 2.0 ** -1000, 2.0 ** 1000,
                  classify.max / 3, classify.max / 2]
    v = []
    for t in thresholds:
        v += [t, np.nextafter(t, np.inf), np.nextafter(t, 0.0)]
        if 2.0 ** -126 <= t <= 2.0 ** 127:  # the f32 neighbours and the rounding midpoints on either side
            f = np.float32(t)
            up, dn = float(np.nextafter(f, np.float32(np.inf))), float(np.nextafter(f, np.float32(0)))
            for m in (up, dn, (t + up) / 2, (t + dn) / 2):
                v += [m, np.nextafter(m, np.inf), np.nextafter(m, 0.0)]
    v += [0.0, 5e-324, 2.0 ** -1030, 2.0 ** -1022, 2.0 ** -149, 2.0 ** -140, 2.0 ** -126, np.finfo(np.float32).max,
          np.finfo(np.float64).max, np.inf, np.nan, 1.0, 0.5, 3.0]
    v = np.array(v, np.float64)
    return np.concatenate([v, -v])


def test_gate_implies_every_check_at_every_edge(classify):
    v = edge_values(classify)
    assert np.signbit(v[np.flatnonzero(v == 0)]).any()  # -0.0 is among them
    benign = np.array([0.5, -1.0, 3.0, 1.0, -0.5, 0.25])
    sets = []
    for k in range(6):  # one component at a time
        r = np.tile(benign, (len(v), 1))
        r[:, k] = v
        sets.append(r)
    for part in (slice(0, 3), slice(3, 6)):  # the whole origin, the whole direction (a = 3 v^2)
        r = np.tile(benign, (len(v), 1))
        r[:, part] = v[:, None]
        sets.append(r)
    rng = np.random.default_rng(20261)
    sets.append(v[rng.integers(0, len(v), (300_000, 6))])
    c = implied(classify, np.concatenate(sets), "edges")
    assert ((c & GATE) != 0).sum() > 100 and ((c & GATE) == 0).sum() > 100
    # the gate's own edges, on the direction and on the origin: at the threshold inside, one f32 step
    # past it outside (a sum that rounds back to the threshold is inside)
    hi, lo = classify.max, classify.min_dir
    f32 = lambda x: float(np.float32(x))
    up = float(np.nextafter(np.float32(hi), np.float32(np.inf)))
    inside = [[0, 0, 0, hi / 2, hi / 4, hi / 4], [0, 0, 0, hi, 1, 1], [hi / 2, hi / 4, hi / 4, 1, 1, 1], [0, 0, 0, lo, lo, lo], [0, 0, -0.0, -lo, 1, 1]]
    outside = [[0, 0, 0, up, lo, lo], [0, 0, 0, hi, up - hi, 1], [up, 0, 0, 1, 1, 1], [hi, up - hi, 0, 1, 1, 1],
               [0, 0, 0, f32(np.nextafter(np.float32(lo), np.float32(0))), 1, 1], [0, 0, 0, 0.0, 1, 1], [0, 0, 0, 1, -0.0, 1]]
    assert ((classify(inside) & GATE) != 0).all()
    assert ((classify(outside) & GATE) == 0).all()


def test_nan_and_inf_fail_the_gate(classify):
    rng = np.random.default_rng(20262)
    for bad in (np.nan, np.inf, -np.inf):
        r = random_rays(rng, 60_000, 1023 - 20, 1023 + 20)
        assert ((classify(r) & GATE) != 0).sum() > 10_000
        r[np.arange(len(r)), rng.integers(0, 6, len(r))] = bad
        assert ((classify(r) & GATE) == 0).all(), bad


@pytest.mark.parametrize("name", ["rtow_final", "cornell"])
def test_scene_rays_pass_the_gate(crt, classify, name):
    d, _, sets, _ = rs.world(crt, name)
    for key in "AB":
        rays = sets[key][0].rays
        assert len(rays) > 2000
        c = classify(rays)
        assert ((c & GATE) != 0).all(), (name, key, rays[np.flatnonzero((c & GATE) == 0)[:3]].tolist())
    bounds_pass(crt, classify, d)


def bounds_pass(crt, classify, d):
    """Rays from anywhere within three times the scene's reach (objects and camera), with direction
    components between 2^-20 and the reach: what a camera ray or a scattered ray (a unit vector, or
    the sum of two) can hold short of a component that cancels to almost nothing."""
    reach = max(float(np.abs(np.asarray(d.objects["v"], np.float64)).max()), max(abs(float(x)) for x in d.camera.center))
    assert 3 * 3 * reach < classify.max
    rng = np.random.default_rng(20263)
    o = (rng.random((4000, 3)) * 2 - 1) * 3 * reach
    dd = np.exp2(rng.uniform(-20, np.log2(reach), (4000, 3))) * rng.choice([-1.0, 1.0], (4000, 3))
    assert ((classify(np.concatenate([o, dd], 1)) & GATE) != 0).all()


def test_millions_camera_rays_pass_the_gate(crt, classify):
    d = crt.SceneData.named("millions", 42)
    rays = dm.centre_rays(rs.camera(crt, d)).reshape(-1, 6)
    assert len(rays) == rs.W * rs.H
    assert ((classify(rays) & GATE) != 0).all()
    bounds_pass(crt, classify, d)
