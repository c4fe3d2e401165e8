"""CPU checks of the radiance-probe tests' inputs (tests/probe_sets.py) and of the oracle entry that
judges them (oracle_radiance): every set has the paths it was made for, in the oracle, so that no
comparison of tests/test_gpu_radiance_probes.py is vacuous; the new entry equals the one
tests/test_oracle.py pins on a camera's own rays, and the reference's own ray_color on the fixtures
tests/golden/gen_golden.py recorded (radiance_<scene>.npz), bit for bit."""
import numpy as np
import pytest

import probe_sets as ps
import radiance_model as rm
import ray_sets as rs
from conftest import load_npz
from oracle import crt_oracle_py as orc


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def hit_share(d, p):
    return float((orc.first_events(d, p.rays, p.t_min) != 0).mean())


@pytest.mark.parametrize("name", ps.SCENES)
def test_shapes_and_states(crt, name):
    d, sets = ps.world(crt, name)
    s, i, v = sets["S"], sets["I"], sets["V"]
    assert s.rays.shape == (ps.N_S, 6) and i.rays.shape == (ps.N_I, 6) and v.rays.shape == (ps.N_V, 6)
    assert [len(x.rays) for x in sets["X"]] == [2 * ps.N_X] * len(ps.X_SCALES) == [4096] * 6
    for p in [s, i, v] + sets["X"]:
        assert p.states.dtype == np.uint32 and len(p.states) == len(p.rays)
        for special in ps.SPECIAL_STATES:
            assert (p.states == special).sum() >= 3, special
        assert len(np.unique(p.states)) > 0.99 * len(p.states)
    z = (v.rays[:, 3:] == 0).any(1)
    assert z[: ps.N_V // 20].all() and not z[ps.N_V // 20:].any()
    for k, x in zip(ps.X_SCALES, sets["X"]):
        assert x.t_min == 1e-5 * 2.0 ** -k and 0 < x.t_min <= 2.0 ** 100
        assert np.array_equal(x.rays[:, :3], np.concatenate([s.rays[:ps.N_X, :3], v.rays[:ps.N_X, :3]]))
        assert np.array_equal(x.rays[:, 3:], np.concatenate([s.rays[:ps.N_X, 3:], v.rays[:ps.N_X, 3:]]) * 2.0 ** k)


@pytest.mark.parametrize("name", ps.SCENES)
def test_every_set_has_the_paths_it_was_made_for(crt, name):
    d, sets = ps.world(crt, name)
    s, i, v = sets["S"], sets["I"], sets["V"]
    # S: origins are hit points of set A, and the directions leave into the normal's hemisphere
    a = rs.set_a(crt, d)
    h = rs.oracle(d, a)
    pts = {p.tobytes() for p in np.ascontiguousarray(h["point"][h["prim"] >= 0])}
    on = np.mean([o.tobytes() in pts for o in np.ascontiguousarray(s.rays[:, :3])])
    z2 = float((ps.oracle(crt, name, "S", 2) == 0).all(1).mean())
    nz50 = float((ps.oracle(crt, name, "S", 50) != 0).any(1).mean())
    # I: back faces first, of every material kind
    ev = orc.first_events(d, i.rays)
    back = (ev & orc.EVENT_BACK) != 0
    kinds = sorted(set(d.materials["kind"][d.objects["material"]].tolist()))
    per_kind = {k: int((back & ((ev & 7) == k)).sum()) for k in kinds}
    tir = int(((ev & orc.EVENT_TIR) != 0).sum())
    vh = hit_share(d, v)
    xh = [hit_share(d, x) for x in sets["X"]]
    got = dict(S_on_hit_points=round(float(on), 3), S_zero_at_2=round(z2, 3), S_nonzero_at_50=round(nz50, 3),
               I_back=round(float(back.mean()), 3), I_back_per_kind=per_kind, I_tir=tir, V_hit=round(vh, 3),
               X_hit=[round(x, 3) for x in xh])
    print(name, got)
    assert on >= 0.9
    assert z2 >= 0.05 and nz50 >= 0.05
    assert back.mean() >= 0.5
    assert all(n >= 16 for n in per_kind.values()), per_kind
    assert 0.05 <= vh <= 0.95
    for k, share in zip(ps.X_SCALES, xh):
        if k < 0 and name in ps.QUADS_ONLY:
            assert share == 0, (k, share)  # the reference's 1e-9 cutoff: see probe_sets' docstring
        else:
            assert 0.05 <= share <= 0.95, (k, share)
    if name in ("rtow_final", "big"):
        assert tir >= 16  # total internal reflection as a path's first event
    m = ps.MEASURED[name]  # the generators are seeded: the shares are reproducible
    assert np.abs(np.array([z2, nz50, back.mean(), vh, *xh]) - np.array([*m[:4], *m[4]])).max() < 0.01


@pytest.mark.parametrize("name", ps.SCENES)
def test_t_min_zero_is_a_live_edge(crt, name):
    """With t_min = 0 a segment that starts on a surface has a root within rounding of 0 on either
    side of it: the oracle's paths differ from the 1e-5 run's in at least 1 % of S."""
    a, b = ps.oracle(crt, name, "S", 50, 0.0), ps.oracle(crt, name, "S", 50)
    share = float((u64(a) != u64(b)).any(1).mean())
    print(name, "records of S that differ at t_min = 0:", round(share, 3))
    assert share >= 0.01
    for t in (1e-3, 0.5):  # few roots lie in (1e-5, t): printed, not required
        print(name, "t_min", t, float((u64(ps.oracle(crt, name, "S", 50, t)) != u64(b)).any(1).mean()))


def test_a_different_state_changes_the_path(crt):
    d, sets = ps.world(crt, "rtow_final")
    s = sets["S"]
    other = orc.radiance(d, s.rays, s.states ^ np.uint32(0x9E3779B9), 50, ps.BG)
    assert (u64(other) != u64(ps.oracle(crt, "rtow_final", "S", 50))).any(1).mean() > 0.05  # the paths that scatter at all


@pytest.mark.parametrize("name", ["rtow_final", "cornell"])
def test_radiance_of_camera_rays_is_the_render_entry(crt, name):
    """oracle_radiance on radiance_model.camera_rays' rays and states is oracle_render's per-sample
    radiance (the entry tests/test_oracle.py pins to the reference), bit for bit."""
    from cpp_raytracer_amd import camera_with
    d = ps.scene_data(crt, name)
    d.camera = camera_with(d.camera, image_w=24, image_h=16, samples_per_pixel=4, max_depth=50)
    cam = crt.resolve_camera(d.camera, 33)
    rays, states = rm.camera_rays(crt, cam)
    _, want = orc.render(d, 33, samples=True)
    got = orc.radiance(d, rays, states, 50, tuple(cam.background), cam.t_min)
    assert np.abs(want).max() > 0
    assert np.array_equal(u64(got), u64(want.reshape(-1, 3)))
    for threads in (1, 3):
        assert np.array_equal(u64(orc.radiance(d, rays, states, 50, tuple(cam.background), cam.t_min, threads)), u64(got))


@pytest.mark.parametrize("name", ps.FIXTURE_SCENES)
def test_radiance_equals_the_references_own_ray_color(crt, name):
    g = load_npz(f"radiance_{name}.npz")
    d = ps.scene_data(crt, name)
    assert str(g["scene_digest"]) == ps.scene_digest(d)
    rays, states = ps.fixture_records(crt, name)
    assert np.array_equal(u64(rays), u64(g["rays"])) and np.array_equal(states, g["states"])
    assert len(rays) <= 1024 and g["depths"].tolist() == list(ps.FIXTURE_DEPTHS) == [1, 3, 50]
    assert np.array_equal(g["background"], np.array(d.camera.background[:]))
    for depth, want in zip(g["depths"], g["rgb"]):
        got = orc.radiance(d, g["rays"], g["states"], int(depth), g["background"])
        assert np.array_equal(u64(got), u64(want)), depth
    assert len(np.unique(u64(g["rgb"][2]), axis=0)) > 8  # paths of several kinds (cornell: 11)


def test_default_states_are_the_oracles_sample_seeds(crt):
    """What the GPU tests compare a `states = NULL` call with: oracle_sample_seed(base, i, 0), restated
    here from include/crt_render.h's crt_sample_seed without the package."""
    def seed(base, pixel, sample):
        m = (1 << 64) - 1
        z = ((pixel << 32) | sample) + base * 0x9E3779B97F4A7C15 & m
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & m
        z = (z ^ (z >> 27)) * 0x94D049BB133111EB & m
        z ^= z >> 31
        return (z ^ (z >> 32)) & 0xFFFFFFFF

    st = ps.default_states(0xDEADBEEF, 4096)
    assert st.dtype == np.uint32 and st.tolist() == [seed(0xDEADBEEF, i, 0) for i in range(4096)]
    assert st.tolist() != [seed(0xDEADBEEF, i, 1) for i in range(4096)]
    d, sets = ps.world(crt, "rtow_final")
    a = orc.radiance(d, sets["S"].rays, st, 50, ps.BG)
    b = orc.radiance(d, sets["S"].rays, np.array([seed(0xDEADBEEF, i, 1) for i in range(4096)], np.uint32), 50, ps.BG)
    assert (u64(a) != u64(b)).any(1).mean() > 0.05  # the paths that scatter at all


def test_rays_outside_the_contract_are_refused(crt):
    d, _ = ps.world(crt, "cornell")
    ok = np.array([[0.5, 0.25, 3.0, 0.1, -0.2, -1.0]])
    assert orc.radiance(d, ok, [1], 5, ps.BG).shape == (1, 3)
    for _, ray, tmax in rs.invalid_rays():
        if tmax == rs.INF:
            with pytest.raises(ValueError, match="outside the query contract"):
                orc.radiance(d, np.array([ok[0], ray]), [1, 2], 5, ps.BG)
    with pytest.raises(ValueError, match="states"):
        orc.radiance(d, ok, [1, 2], 5, ps.BG)
