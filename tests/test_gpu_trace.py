"""crt_trace_async on the GPU: the fast route (query_kernel: the render kernel's traversal), the
plain route (CRT_TRACE_PLAIN: crt_closest_hits' loop on the same buffers) and the oracle
(oracle/crt_oracle_py.py hits) agree on every record, on every instance device_trace can launch.
prim, front_face and material are compared with ==, t, point and normal as bit patterns.
Buffers are device tensors: outputs pre-filled with 0xFF bytes and followed by a sentinel tail that
must be intact afterwards, the rays followed by NaN rays past n. The ray sets are tests/ray_sets.py's
(tests/test_ray_sets.py: each has hits and misses in the oracle)."""
import math

import numpy as np
import pytest

import denoise_model as dm
import ray_sets as rs
from oracle import crt_oracle_py as orc

pytestmark = pytest.mark.gpu
TAIL = 9
ANY, PLAIN = 1, 2


@pytest.fixture(autouse=True)
def fast_instances(monkeypatch):
    """Scenes that fit LDS take the plain route by default (it measured faster there); the tests are
    about the fast instances, so they ask for them."""
    monkeypatch.setenv("CRT_TRACE_FAST", "1")


def run(scene, call, flags=0, n=None):
    """One crt_trace_async call on device 0 and the current stream; closest mode returns HIT_DTYPE
    records, any mode a bool array."""
    import torch
    from cpp_raytracer_amd import HIT_DTYPE
    rays = call.rays if n is None else call.rays[:n]
    n = len(rays)
    buf = torch.full((n + TAIL, 6), math.nan, dtype=torch.float64, device="cuda")
    buf[:n] = torch.from_numpy(np.ascontiguousarray(rays))
    tm = None
    if call.tmax is not None:
        tm = torch.full((n + TAIL,), math.nan, dtype=torch.float64, device="cuda")
        tm[:n] = torch.from_numpy(np.ascontiguousarray(call.tmax[:n]))
    width = 4 if flags & ANY else HIT_DTYPE.itemsize
    out = torch.full((n + TAIL, width), 0xFF, dtype=torch.uint8, device="cuda")
    scene.trace_async(0, buf.data_ptr(), n, hits_ptr=0 if flags & ANY else out.data_ptr(),
                      occluded_ptr=out.data_ptr() if flags & ANY else 0, t_min=call.t_min, t_max=call.t_max,
                      tmax_ptr=tm.data_ptr() if tm is not None else 0, flags=flags,
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[n:] == 0xFF).all(), "the call wrote past its n records"
    if flags & ANY:
        occ = host[:n].copy().view(np.uint32).reshape(n)
        assert np.isin(occ, (0, 1)).all()
        return occ == 1
    return host[:n].copy().view(HIT_DTYPE).reshape(n)


def same(got, want, what=""):
    assert got.shape == want.shape, what
    for f in ("prim", "front_face", "material", "reserved"):
        assert np.array_equal(got[f], want[f]), (what, f, int((got[f] != want[f]).sum()))
    for f in ("t", "point", "normal"):
        assert np.array_equal(dm.bits(got[f]), dm.bits(want[f])), (what, f)


_SCENES = {}


def resident(crt, name):
    """The test scene on device 0, built under the default switches and kept for the module."""
    if name not in _SCENES:
        d, kw, _, _ = rs.world(crt, name)
        s = crt.GpuScene(d, **kw)
        s.upload(0)
        _SCENES[name] = s
    return _SCENES[name]


def check_world(crt, name, scene, letters=None, routes=(0, PLAIN)):
    """Every call of the scene's sets: closest records equal the oracle's, any-hit flags equal
    "the oracle found something", on each route."""
    _, _, sets, want = rs.world(crt, name)
    for k, calls in sets.items():
        if letters and k not in letters:
            continue
        for j, (call, w) in enumerate(zip(calls, want[k])):
            for route in routes:
                same(run(scene, call, route), w, f"{name} {k}{j} route {route}")
                assert np.array_equal(run(scene, call, route | ANY), w["prim"] >= 0), f"{name} {k}{j} any, route {route}"


# ---- routes and instances ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rs.SCENE_SETS))
def test_fast_route_plain_route_and_oracle_agree(crt, name):
    """rtow_final: LDS scene, sphere-only, the packed sphere filter. cornell: LDS, the flat-box filter
    in the general instance. rotated / mixed: the generic parallelogram filter / no filter.
    christmas_tree: HBM scene, LDS treelet and stack, the pair walk. big / big_mixed: u32 stack
    entries. bvh_pathological: one 135-primitive leaf. rotated_linear / mixed_linear: one always-entered leaf
    of 30 parallelograms (the generic filter) / of 36 primitives (the plain loop)."""
    check_world(crt, name, resident(crt, name))


@pytest.mark.parametrize("name", ["rtow_final", "cornell", "mixed", "christmas_tree"])
def test_default_dispatch(crt, monkeypatch, name):
    """Without CRT_TRACE_FAST (LDS-sized scenes then go to the plain route): the same records."""
    monkeypatch.delenv("CRT_TRACE_FAST")
    check_world(crt, name, resident(crt, name), routes=(0,))


SWITCHES = [
    ("christmas_tree", {"CRT_NO_PAIR_WALK": "1"}), ("christmas_tree", {"CRT_FORCE_GSTACK": "1"}),
    ("christmas_tree", {"CRT_FORCE_GSTACK": "1", "CRT_NO_PAIR_WALK": "1"}),
    ("rtow_final", {"CRT_NO_LDS_SCENE": "1"}), ("rtow_final", {"CRT_NO_LDS_SCENE": "1", "CRT_FORCE_GSTACK": "1"}),
    ("mixed", {"CRT_NO_LDS_SCENE": "1"}), ("mixed", {"CRT_NO_LDS_SCENE": "1", "CRT_FORCE_GSTACK": "1"}),
    ("mixed", {"CRT_NO_LDS_SCENE": "1", "CRT_NO_PAIR_WALK": "1"}),
    ("big", {"CRT_FORCE_GSTACK": "1"}), ("big_mixed", {"CRT_FORCE_GSTACK": "1"}), ("big", {"CRT_NO_PAIR_WALK": "1"}),
    ("rtow_final", {"CRT_F64_NODES": "1"}), ("rtow_final", {"CRT_F64_SPHERES": "1"}), ("rtow_final", {"CRT_EXACT_SLAB": "1"}),
    ("cornell", {"CRT_F64_NODES": "1"}), ("cornell", {"CRT_F64_QUADS": "1"}), ("cornell", {"CRT_GENERIC_QUADS": "1"}),
    ("cornell", {"CRT_EXACT_SLAB": "1"}), ("rotated", {"CRT_F64_QUADS": "1"}), ("christmas_tree", {"CRT_EXACT_SLAB": "1"}),
    ("christmas_tree", {"CRT_F64_NODES": "1"}),
]


@pytest.mark.parametrize("name,env", SWITCHES, ids=[n + "-" + "+".join(k[4:] for k in e) for n, e in SWITCHES])
def test_every_switch_gives_the_same_bytes(crt, monkeypatch, name, env):
    """The run-time switches device_trace shares with the render kernel, each on a scene it
    affects (the scene is built and uploaded under the switch: the filter switches are read then).
    The fast route's records still equal the oracle's, hence the default run's bytes."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d, kw, _, _ = rs.world(crt, name)
    s = crt.GpuScene(d, **kw)
    s.upload(0)
    check_world(crt, name, s, routes=(0,))
    s.close()


def test_no_lds_scene_bytes_equal_the_lds_run(crt, monkeypatch):
    s = resident(crt, "rtow_final")
    call = rs.world(crt, "rtow_final")[2]["D"][0]
    lds = run(s, call)
    monkeypatch.setenv("CRT_NO_LDS_SCENE", "1")
    assert run(s, call).tobytes() == lds.tobytes()


# ---- ray counts and refill --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree"])
def test_ray_counts(crt, name):
    s = resident(crt, name)
    _, _, sets, want = rs.world(crt, name)
    call, w = sets["D"][0], want["D"][0]
    for n in (1, 63, 64, 65, 257, 4097):
        for route in (0, PLAIN):
            same(run(s, call, route, n), w[:n], f"{name} n={n} route {route}")
            assert np.array_equal(run(s, call, route | ANY, n), w["prim"][:n] >= 0)


@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree", "cornell"])
@pytest.mark.parametrize("blocks", ["1", "3"])
def test_small_grids_refill_every_lane(crt, monkeypatch, name, blocks):
    """20,000 rays on 1 and 3 blocks: every lane takes dozens of rays, from batch after batch."""
    s = resident(crt, name)
    _, _, sets, want = rs.world(crt, name)
    monkeypatch.setenv("CRT_GRID_BLOCKS", blocks)
    same(run(s, sets["D"][0]), want["D"][0], f"{name} on {blocks} blocks")
    assert np.array_equal(run(s, sets["D"][0], ANY), want["D"][0]["prim"] >= 0)
    c = sets["C"][0]
    same(run(s, c), want["C"][0], f"{name} C on {blocks} blocks")


# ---- interval edges ---------------------------------------------------------------------------------
def edge_oracle(d, call, t):
    """The oracle's record of every ray i over (t_min, t[i]), one oracle run a ray."""
    from cpp_raytracer_amd import HIT_DTYPE
    out = np.zeros(len(call.rays), HIT_DTYPE)
    for i in range(len(call.rays)):
        out[i] = orc.hits(d, call.rays[i:i + 1], call.t_min, float(t[i]))[0]
    return out


@pytest.mark.parametrize("name,limit", [("cornell", None), ("rtow_final", 256), ("christmas_tree", 64)])
def test_upper_bound_edges(crt, name, limit):
    """For hits of set A at distance t (all of cornell's; a seeded 256 / 64 of the larger scenes',
    whose oracle builds its tree again for every ray): t_max = t must not return the hit, t_max =
    nextafter(t, inf) must. The oracle is shown to change its answer across the edge first."""
    d, _, sets, want = rs.world(crt, name)
    a, w = sets["A"][0], want["A"][0]
    idx = np.flatnonzero(w["prim"] >= 0)
    if limit:
        idx = np.sort(np.random.default_rng(5).choice(idx, limit, replace=False))
    rays, hit = a.rays[idx], w[idx]
    at = rs.Call(rays, tmax=hit["t"].copy())
    above = rs.Call(rays, tmax=np.nextafter(hit["t"], math.inf))
    o_at, o_above = edge_oracle(d, at, at.tmax), edge_oracle(d, above, above.tmax)
    assert not ((o_at["prim"] == hit["prim"]) & (dm.bits(o_at["t"]) == dm.bits(hit["t"]))).any()
    assert (o_at["prim"] < 0).all()  # nothing lies before the first hit
    same(o_above, hit, "oracle above the edge")
    s = resident(crt, name)
    for route in (0, PLAIN):
        same(run(s, at, route), o_at, f"{name} t_max = t, route {route}")
        same(run(s, above, route), hit, f"{name} t_max = nextafter(t), route {route}")
        assert np.array_equal(run(s, at, route | ANY), o_at["prim"] >= 0)
        assert run(s, above, route | ANY).all()


@pytest.mark.parametrize("name", ["cornell", "rtow_final", "christmas_tree"])
def test_lower_bound_edges(crt, name):
    """16 hits of set A, each in calls of one ray: t_min = t must not return the hit (the oracle
    then reports what lies behind it, or nothing), t_min = nextafter(t, 0) must."""
    d, _, sets, want = rs.world(crt, name)
    a, w = sets["A"][0], want["A"][0]
    idx = np.random.default_rng(6).choice(np.flatnonzero(w["prim"] >= 0), 16, replace=False)
    s = resident(crt, name)
    changed = 0
    for i in idx:
        t = float(w["t"][i])
        for t_min, keeps in ((t, False), (float(np.nextafter(t, 0.0)), True)):
            call = rs.Call(a.rays[i:i + 1], t_min=t_min)
            o = orc.hits(d, call.rays, t_min)
            if keeps:
                same(o, w[i:i + 1], "oracle below the edge")
            else:
                assert not (o["prim"][0] == w["prim"][i] and dm.bits(o["t"])[0] == dm.bits(w["t"][i:i + 1])[0])
                changed += 1
            for route in (0, PLAIN):
                same(run(s, call, route), o, f"{name} ray {i} t_min {t_min!r} route {route}")
                assert run(s, call, route | ANY)[0] == (o["prim"][0] >= 0)
    assert changed == 16


@pytest.mark.parametrize("name", ["cornell", "rtow_final", "christmas_tree", "mixed"])
@pytest.mark.parametrize("t_min", [1e6, -1.0, 5e-324, -3e4, 2.0 ** 101, -(2.0 ** 101)])
def test_large_negative_and_denormal_t_min(crt, name, t_min):
    """t_min far outside the camera's 1e-5: beyond every hit, negative (hits behind the origin count;
    the leaf filters are off), denormal, and beyond +-2^100 where the call leaves the f32 node test."""
    d, _, sets, _ = rs.world(crt, name)
    s = resident(crt, name)
    for k in "AB":
        call = rs.Call(sets[k][0].rays, t_min=t_min)
        o = orc.hits(d, call.rays, t_min)
        for route in (0, PLAIN):
            same(run(s, call, route), o, f"{name} {k} t_min {t_min} route {route}")
        assert np.array_equal(run(s, call, ANY), o["prim"] >= 0)
    if t_min == -1.0:  # the oracle does report hits at negative distances there
        assert (orc.hits(d, sets["B"][0].rays, t_min)["t"] < 0).any()


def test_upper_bounds_of_either_sign(crt):
    """Per-ray upper bounds that are negative, zero, -inf, below -2^100 and t_min itself, under a
    negative t_min: the last three leave an empty interval, which is a miss and is never traced
    (the walks' sentinel would not be entered: crt_ray_class.h)."""
    d, _, sets, _ = rs.world(crt, "rtow_final")
    s = resident(crt, "rtow_final")
    rays = sets["B"][0].rays[:4096]
    vals = np.array([-0.5, 0.0, -math.inf, -(2.0 ** 120), 3.0, math.inf, -1e-3, -2.0, -5.0])
    call = rs.Call(rays, t_min=-2.0, tmax=vals[np.arange(len(rays)) % len(vals)])
    o = rs.oracle(d, call)
    assert (o["prim"] >= 0).any() and (o["t"][o["prim"] >= 0] < 0).any()
    assert not (o["prim"][call.tmax <= -2.0] >= 0).any()
    for route in (0, PLAIN):
        same(run(s, call, route), o, f"route {route}")
        assert np.array_equal(run(s, call, route | ANY), o["prim"] >= 0)


# ---- rays outside the contract ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree", "mixed"])
def test_rays_outside_the_contract_are_misses(crt, name):
    from cpp_raytracer_amd import HIT_DTYPE
    _, _, sets, want = rs.world(crt, name)
    s = resident(crt, name)
    base, w = sets["D"][0].rays[:1500], want["D"][0][:1500]
    bad = rs.invalid_rays()
    rays, tmax, valid = [], [], []
    j = 0
    for i in range(len(base)):
        if i % 23 == 5:  # one in every wave or so, each class many times over
            _, r, tm = bad[j % len(bad)]
            j += 1
            rays.append(r)
            tmax.append(tm)
            valid.append(False)
        rays.append(base[i])
        tmax.append(math.inf)
        valid.append(True)
    assert j >= 3 * len(bad)
    call = rs.Call(np.array(rays), tmax=np.array(tmax))
    valid = np.array(valid)
    miss = np.zeros(1, HIT_DTYPE)
    miss["prim"] = -1
    for route in (0, PLAIN):
        got = run(s, call, route)
        same(got[valid], w, f"{name} valid neighbours, route {route}")
        assert all(r.tobytes() == miss.tobytes() for r in got[~valid]), f"route {route}"
        occ = run(s, call, route | ANY)
        assert np.array_equal(occ[valid], w["prim"] >= 0) and not occ[~valid].any()


# ---- streams ----------------------------------------------------------------------------------------
def test_trace_follows_the_tensors_stream(crt):
    """Rays made by torch ops on a side stream, GpuScene.trace on that stream with no
    synchronisation in between, one synchronise at the end."""
    import torch
    from cpp_raytracer_amd import HIT_DTYPE
    d, _, sets, want = rs.world(crt, "rtow_final")
    s = resident(crt, "rtow_final")
    call, w = sets["D"][0], want["D"][0]
    host = torch.from_numpy(call.rays).pin_memory()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        half = host.to("cuda", non_blocking=True) * 0.5
        filler = torch.ones((4096, 4096), device="cuda")
        for _ in range(4):  # work queued ahead of the rays' last op
            filler = filler @ filler * 1e-4
        rays = half + half  # x * 0.5 + x * 0.5 == x exactly
        hits = s.trace(rays)
        occ = s.trace(rays, any_hit=True)
        tm = torch.full((len(w),), 7.5, dtype=torch.float64, device="cuda")
        short = s.trace(rays, tmax=tm, plain=True)
    side.synchronize()
    assert hits.shape == (len(w), 72) and hits.dtype == torch.uint8 and occ.dtype == torch.bool
    same(hits.cpu().numpy().view(HIT_DTYPE).reshape(-1), w, "side stream")
    assert np.array_equal(occ.cpu().numpy(), w["prim"] >= 0)
    same(short.cpu().numpy().view(HIT_DTYPE).reshape(-1), orc.hits(d, call.rays, 1e-5, 7.5), "side stream, bounded")
    empty = s.trace(torch.zeros((0, 6), dtype=torch.float64, device="cuda"))
    assert empty.shape == (0, 72)


# ---- agreement with what exists ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtow_final", "cornell", "christmas_tree"])
def test_agrees_with_features_and_closest_hits(crt, name):
    import torch
    from cpp_raytracer_amd import FEATURE_DTYPE
    d, _, sets, _ = rs.world(crt, name)
    s = resident(crt, name)
    a = sets["A"][0]
    got = run(s, a)
    assert got.tobytes() == s.closest_hits(a.rays, 1e-5).tobytes()
    cam = rs.camera(crt, d)
    feat = torch.full((rs.H * rs.W, FEATURE_DTYPE.itemsize), 0xFF, dtype=torch.uint8, device="cuda")
    s.render_features(0, cam, feat.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    f = feat.cpu().numpy().view(FEATURE_DTYPE).reshape(-1)
    assert np.array_equal(f["prim"], got["prim"]) and np.array_equal(f["material"], got["material"])
    for k in ("t", "point", "normal"):
        assert np.array_equal(dm.bits(f[k]), dm.bits(got[k])), k
