"""The render kernel on both sides of every fast-path range guard: the cases of tests/guard_cases.py
(tests/test_guard_cases.py shows where each one sits) rendered on the GPU from the LDS scene, from
HBM (CRT_NO_LDS_SCENE: the pair walk) and, one case per ladder, with the traversal stack in HBM
(CRT_FORCE_GSTACK), against the C oracle at test_gpu_fuzz_scenes.py's bar (1e-12 x max(1, |want|),
all finite, Schlick guard 0); the HBM frame bit-identical to the LDS one; Ladder A frames
bit-identical to the base frame (sphere family; the others from F = 2^-31 down to one another: the
reference's 1e-9 parallelogram cutoff, tests/test_guard_cases.py). A frame is a piecewise-constant
function of the geometry (products of albedos, lights and the background), so frames catch a wrong
decision, not a wrong last bit of t; the closest-hit tests compare t itself. render_count at max_depth 1 shows
that the guard really switched the path; crt_closest_hits and crt_render_features_async (trace():
its own coarse reject, div_a, sqrt_from_rsq) run scaled rays and exact t_min / t_max ties."""
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import crt_oracle_py as orc  # noqa: E402
import denoise_model as dm  # noqa: E402
import guard_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12  # relative to max(1, |want|): test_gpu_fuzz_scenes.py's bar
# CRT_FORCE_GSTACK moves the stack of the HBM-scene kernels only (a scene that fits LDS takes its stack along)
ROUTES = {"lds": {}, "hbm": {"CRT_NO_LDS_SCENE": "1"}, "gstack": {"CRT_NO_LDS_SCENE": "1", "CRT_FORCE_GSTACK": "1"}}
_frames = {}


def render_gpu(crt, monkeypatch, d, route):
    with monkeypatch.context() as m:
        for k, v in ROUTES[route].items():
            m.setenv(k, v)
        s = crt.GpuScene(d)
        out, _ = s.render(crt.resolve_camera(d.camera, gc.BASE_SEED), 1)
        guard = s.guard(0)
        s.close()
    return out, guard


def gpu_frame(crt, monkeypatch, case, fam):
    """The LDS-route frame of a case (rendered once; Ladder A compares against two of them)."""
    key = (case.id, fam)
    if key not in _frames:
        _frames[key] = render_gpu(crt, monkeypatch, gc.scene(crt, fam, case.s, case.e, case.cam), "lds")
    return _frames[key]


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.id)
def test_frames_match_the_oracle_on_every_route(crt, monkeypatch, case):
    for fam in case.families:
        d = gc.scene(crt, fam, case.s, case.e, case.cam)
        want = orc.render(d, gc.BASE_SEED, threads=16)
        got, guard = gpu_frame(crt, monkeypatch, case, fam)
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print(f"{case.id} {fam}: max rel err {err.max():.3g}")
        assert guard == 0, fam
        assert np.isfinite(got).all() and err.max() <= TOL, \
            f"{fam}: max rel err {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
        for route in ("hbm", "gstack") if case.gstack else ("hbm",):
            other, guard = render_gpu(crt, monkeypatch, d, route)
            assert guard == 0, (fam, route)
            assert dm.bits(other).tobytes() == dm.bits(got).tobytes(), (fam, route)
        if case.ladder == "A":  # the paths are bit-identical and the colour does not see the scale
            ref = None
            if fam == "spheres":
                ref = gc.BY_ID["A-s0-e0-origin"]
            elif gc.quads_cut(case):
                ref = gc.BY_ID["A-s0-e-31-origin"]
            if ref is not None:
                base, _ = gpu_frame(crt, monkeypatch, ref, fam)
                assert dm.bits(got).tobytes() == dm.bits(base).tobytes(), fam


# ---- the guard really switched: render_count at max_depth 1 (primary rays only) --------------------
def counters(crt, monkeypatch, case, fam, route):
    d = gc.scene(crt, fam, case.s, case.e, case.cam, max_depth=1)
    with monkeypatch.context() as m:
        for k, v in ROUTES[route].items():
            m.setenv(k, v)
        m.setenv("CRT_COUNT_SPEC", "1")  # walk like the timed kernel (test_gpu_vs_oracle.py)
        s = crt.GpuScene(d)
        s.upload(0)
        st = s.render_count(0, crt.resolve_camera(d.camera, gc.BASE_SEED))
        s.close()
    print(f"{case.id} {fam} {route}: rays {st.rays} nodes {st.nodes_visited} slow {st.slow_node_tests} "
          f"spheres {st.sphere_tests} quads {st.parallelogram_tests} candidates {st.candidate_tests}")
    assert st.rays == gc.W * gc.H * gc.SPP and st.nodes_visited > 0
    return st


# (guard, inside case, outside case) of the f32 node test: trav_init's per-ray range and the
# per-scene kF32BoundMax
NODE_PAIRS = [
    ("trav_d_lo", "A-s0-e0-origin", "A-s0-e-40-origin"),
    ("trav_d_lo", "A-s0-e0-origin", "A-s0-e-42-origin"),
    ("trav_d_hi", "B-s22-e38-origin", "B-s24-e41-origin"),
    ("trav_d_hi", "B-s22-e38-offset", "B-s24-e41-offset"),
    ("bound_40", "C-s36-e0-offset", "C-s37-e0-offset"),
    ("o_40", "C-s35-e0-far", "C-s36-e0-far"),
]
# the share of node tests left to f64 that test_f32_walk_decides_almost_every_node allows: 1e-3 for
# its sphere scene from LDS, 1e-2 for the pair walk from HBM. The parallelogram families have no
# entry there; the flat one's faces lie on node bounds (exact ties the f32 margin cannot decide:
# crt_device.hip slab64_inv names ~28 % for Cornell), so inside its range it is only required to
# leave most tests to f32.
SHARE = {("spheres", "lds"): 1e-3, ("spheres", "hbm"): 1e-2, ("rotated", "lds"): 1e-2, ("rotated", "hbm"): 1e-2,
         ("mixed", "lds"): 1e-2, ("mixed", "hbm"): 1e-2, ("flat", "lds"): 0.5, ("flat", "hbm"): 0.5}


@pytest.mark.parametrize("guard,inside,outside", NODE_PAIRS, ids=lambda v: str(v))
def test_node_test_guard_switches_the_walk(crt, monkeypatch, guard, inside, outside):
    """Outside the range marg = inf: every node test is decided in f64. slow_node_tests also counts
    the walk's sentinel node (nodes_visited does not), which a traversal reaches at most once and
    the pair walk tests beside at most one sibling, so it lies in [nodes, nodes + 2 rays]. Inside,
    the share of f64 decisions stays under SHARE."""
    for fam in gc.FAMILIES:
        for route in ("lds", "hbm"):
            out = counters(crt, monkeypatch, gc.BY_ID[outside], fam, route)
            assert out.nodes_visited <= out.slow_node_tests <= out.nodes_visited + 2 * out.rays, (fam, route)
            ins = counters(crt, monkeypatch, gc.BY_ID[inside], fam, route)
            assert ins.slow_node_tests <= SHARE[fam, route] * ins.nodes_visited, (fam, route)


def test_rays_on_both_sides_of_the_node_test_range(crt, monkeypatch):
    """F = 2^-33: every centre ray is inside 2^-39, but the jittered samples of the two centre
    columns and rows (|d_x| or |d_y| below one pixel = 2^-38) are not always: some node tests in
    f64, well under all of them. F = 2^-36: more, still not all."""
    for fam in gc.FAMILIES:
        a = counters(crt, monkeypatch, gc.BY_ID["A-s0-e-33-origin"], fam, "lds")
        b = counters(crt, monkeypatch, gc.BY_ID["A-s0-e-36-origin"], fam, "lds")
        assert a.slow_node_tests <= b.slow_node_tests < b.nodes_visited, fam
        assert a.slow_node_tests <= 0.5 * a.nodes_visited, fam


# (guard, inside case, outside case) of the leaf filters: leaf_ray32_ok (sphere pairs),
# quad_ray32_ok (generic parallelogram filter), the per-scene record ranges
LEAF_PAIRS = [
    ("leaf_a_lo", "A-s0-e-29-origin", "A-s0-e-31-origin"),
    ("leaf_a_hi", "B-s12-e29-origin", "B-s12-e30-origin"),
    ("leaf_a_hi", "B-s12-e29-offset", "B-s12-e30-offset"),
    ("leaf_d_hi", "B-s12-e29-origin", "B-s12-e31-origin"),
    ("leaf_d_hi", "B-s12-e29-offset", "B-s12-e31-offset"),
    ("o_30", "C-s25-e0-far", "C-s26-e0-far"),
    ("rec_30", "C-s26-e0-offset", "C-s27-e0-offset"),
    ("o_30", "C-s27-e0-offset", "C-s28-e0-offset"),  # both outside the record range: no filter at all
    ("sn1_hi", "C-s-19-e-19-offset", "C-s-21-e-21-offset"),
]


@pytest.mark.parametrize("guard,inside,outside", LEAF_PAIRS, ids=lambda v: str(v))
def test_leaf_filter_guard_switches_the_leaf(crt, monkeypatch, guard, inside, outside):
    """candidate_tests is counted only in leaf_step's two-pass branches: 0 where a guard turns them
    off (gc.filter_expected restates which do, per family and route), positive where they run, and
    then below the primitive count (the filter rejects). The walk is the same on both sides, so the
    inside case tests no more primitives than the outside one (where the rays are the same)."""
    switched = 0
    for fam in gc.BY_ID[inside].families:
        for route in ("lds", "hbm"):
            sts = []
            for cid in (inside, outside):
                case = gc.BY_ID[cid]
                on = gc.filter_expected(fam, route, gc.measure(crt, gc.scene(crt, fam, case.s, case.e, case.cam)))
                assert on is not None, (cid, fam)
                st = counters(crt, monkeypatch, case, fam, route)
                prims = st.sphere_tests + st.parallelogram_tests
                if on:
                    assert 0 < st.candidate_tests < prims, (cid, fam, route)
                else:
                    assert st.candidate_tests == 0, (cid, fam, route)
                sts.append((on, prims))
            switched += sts[0][0] != sts[1][0]
            # Ladder B from the origin: d is the partner's times a power of two exactly, the same rays.
            # With the camera off the origin pixel - origin rounds at the camera's scale (2^-23 of
            # |d| at worst, Ladder C's s = 28): only grazing rays can enter another leaf. (Ladder A's
            # 1e-9 cutoff changes t_max, and so the walk.)
            if gc.BY_ID[inside].ladder == "B" and gc.BY_ID[inside].cam == "origin":
                assert sts[0][1] <= sts[1][1], (fam, route)
            elif gc.BY_ID[inside].ladder != "A":
                assert abs(sts[0][1] - sts[1][1]) <= 0.02 * sts[1][1], (fam, route)
    assert switched or inside == "C-s27-e0-offset"  # (that pair: both beyond the records' range)


def test_generic_parallelogram_filter_needs_directions_of_2_to_the_minus_30(crt, monkeypatch):
    """quad_ray32_ok's D = max |d_k| >= 2^-30: F = 2^-29 inside, F = 2^-31 outside (there the
    reference's cutoff misses every parallelogram, so only the counter can tell)."""
    ins = counters(crt, monkeypatch, gc.BY_ID["A-s0-e-29-origin"], "rotated", "lds")
    out = counters(crt, monkeypatch, gc.BY_ID["A-s0-e-31-origin"], "rotated", "lds")
    assert 0 < ins.candidate_tests < ins.parallelogram_tests
    assert out.candidate_tests == 0 and out.parallelogram_tests > 0


def test_flat_box_filter_keeps_every_parallelogram_outside_the_walks_range(crt, monkeypatch):
    """marg = inf: no flat box is rejected, every parallelogram of an entered leaf is a candidate."""
    ins = counters(crt, monkeypatch, gc.BY_ID["B-s22-e38-origin"], "flat", "lds")
    out = counters(crt, monkeypatch, gc.BY_ID["B-s24-e41-origin"], "flat", "lds")
    assert 0 < ins.candidate_tests < ins.parallelogram_tests
    assert out.candidate_tests == out.parallelogram_tests > 0
    none = counters(crt, monkeypatch, gc.BY_ID["C-s37-e0-offset"], "flat", "lds")  # no f32 walk: no flat boxes
    assert none.candidate_tests == 0


# ---- trace(): crt_closest_hits and the features ----------------------------------------------------
def same_hits(got, want):
    assert np.array_equal(got["prim"], want["prim"])
    hit = want["prim"] >= 0
    for name in ("t", "point", "normal"):
        assert np.array_equal(dm.bits(got[name][hit]), dm.bits(want[name][hit])), name


@pytest.fixture(scope="module", params=gc.FAMILIES)
def hit_job(request, crt):
    fam = request.param
    d = gc.scene(crt, fam)
    s = crt.GpuScene(d)
    rays = gc.closest_hit_rays(fam)
    base = s.closest_hits(rays, 1e-5)
    yield fam, d, s, rays, base
    s.close()


def test_closest_hits_of_scaled_directions(hit_job):
    fam, d, s, rays, base = hit_job
    same_hits(base, orc.hits(d, rays, 1e-5))
    hit = base["prim"] >= 0
    assert hit.sum() > 500
    for k in gc.HIT_SCALES[1:]:
        r = rays.copy()
        r[:, 3:] *= 2.0 ** k
        tmin = 1e-5 * 2.0 ** -k
        got = s.closest_hits(r, tmin)
        same_hits(got, orc.hits(d, r, tmin))
        if fam == "spheres" or k > 0:  # the scaling is exact (test_guard_cases.py shows it for the oracle)
            assert np.array_equal(got["prim"], base["prim"]), k
            assert np.array_equal(dm.bits(got["t"][hit] * 2.0 ** k), dm.bits(base["t"][hit])), k
            for name in ("point", "normal"):
                assert np.array_equal(dm.bits(got[name][hit]), dm.bits(base[name][hit])), (k, name)


def test_closest_hits_at_exact_interval_ties(hit_job):
    """(t_min, t_max) is exclusive: for every base hit at parameter t, t_max = t and t_min = t must
    not return that hit, t_max = nextafter(t, inf) and t_min = nextafter(t, 0) must, and all four
    are the oracle's answer: the 2^-30 margins of lim_tmax / lim_tmin and the 2^-12 coarse reject
    of hit_sphere at exact ties."""
    fam, d, s, rays, base = hit_job
    idx = np.flatnonzero(base["prim"] >= 0)
    assert len(idx) > 500
    for i in idx:
        ray, t, prim = rays[i:i + 1], float(base["t"][i]), int(base["prim"][i])
        for tmin, tmax, returns in ((1e-5, t, False), (1e-5, np.nextafter(t, np.inf), True),
                                    (t, np.inf, False), (np.nextafter(t, 0.0), np.inf, True)):
            got = s.closest_hits(ray, tmin, tmax)
            want = orc.hits(d, ray, tmin, tmax)
            same_hits(got, want)
            same = int(got["prim"][0]) == prim and float(got["t"][0]) == t
            assert same == returns, (i, tmin, tmax, got["t"][0], t)


@pytest.mark.parametrize("case", ["A-s0-e-251-origin", "A-s0-e-385-origin", "B-s236-e251-offset"])
def test_features_of_scaled_cameras(crt, case):
    """crt_render_features_async equals the oracle's hits of the centre rays (as
    test_gpu_denoise.py checks at ordinary scale)."""
    import torch
    case = gc.BY_ID[case]
    for fam in case.families:
        d = gc.scene(crt, fam, case.s, case.e, case.cam)
        cam = crt.resolve_camera(d.camera, gc.BASE_SEED)
        hits = orc.hits(d, dm.centre_rays(cam).reshape(-1, 6), cam.t_min).reshape(gc.H, gc.W)
        want = dm.features_from_hits(hits, d.materials, list(cam.background), crt.FEATURE_DTYPE)
        s = crt.GpuScene(d)
        s.upload(0)
        buf = torch.full((gc.H * gc.W, 88), 0xFF, dtype=torch.uint8, device="cuda")
        s.render_features(0, cam, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(crt.FEATURE_DTYPE).reshape(gc.H, gc.W)
        s.close()
        if not (gc.quads_cut(case) and fam in ("flat", "rotated")):
            assert (want["prim"] >= 0).mean() >= 0.2, fam
        for name in ("prim", "material"):
            assert np.array_equal(got[name], want[name]), (fam, name)
        for name in ("t", "point", "normal", "albedo"):
            assert np.array_equal(dm.bits(got[name]), dm.bits(want[name])), (fam, name)
