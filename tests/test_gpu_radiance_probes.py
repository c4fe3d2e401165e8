"""crt_radiance_async on rays that no camera made, held to the reference: tests/probe_sets.py's surface
probes (S), inside starts (I), volume rays (V) and scaled rays (X) with seeded and special LCG states,
at call t_min values other than the camera's, through both routes. The judge is the oracle's ray_color
on the same records (oracle_radiance, which tests/test_probe_sets.py ties to the reference's own
ray_color and to the render entry), and for three fixtures the reference's stored output itself.

Every call asserts: the fast route's bits are the plain route's, and max |gpu - oracle| <=
1e-12 * max(1, max |oracle|), the bar of tests/test_gpu_parity.py and of
test_gpu_radiance.test_per_path_radiance_matches_the_oracle (the paths are the reference's; only the
association of the throughput product differs). The harness is tests/test_gpu_radiance.py's: NaN rays
past n, 0xFF-prefilled outputs, a sentinel tail, and every scene's parity guard at 0 after every test."""
import numpy as np
import pytest

import probe_sets as ps
import test_gpu_radiance as tgr
from conftest import load_npz
from test_gpu_radiance import PLAIN, bits, guard_stays_zero, run  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
BAR = 1e-12
DEPTHS = (1, 2, 3, 50)
T_MINS = (0.0, 1e-3, 0.5)


def resident(crt, name):
    """test_gpu_radiance.resident, which also keeps rtow_final_lights (not a scene of ray_sets)."""
    if name not in tgr._SCENES and name == "rtow_final_lights":
        d = ps.scene_data(crt, name)
        s = crt.GpuScene(d)
        s.upload(0)
        tgr._SCENES[name] = (d, s)
    return tgr.resident(crt, name)


def held(scene, label, rays, states, depth, bg, t_min, want, **kw):
    """One call through both routes against `want`; returns the fast route's radiance."""
    fast = run(scene, rays, states, depth, tuple(bg), t_min, 0, **kw)
    plain = run(scene, rays, states, depth, tuple(bg), t_min, PLAIN, **kw)
    top = float(np.abs(want).max())
    err = float(np.abs(fast - want).max())
    print(f"{label} depth {depth} t_min {t_min:.3g}: max |gpu - oracle| = {err:.3g}, max |oracle| = {top:.3g}")
    assert np.array_equal(bits(fast), bits(plain)), f"{label}: fast route differs from the plain route"
    assert err <= BAR * max(1.0, top), (label, depth, t_min, err)
    return fast


@pytest.mark.parametrize("key", ["S", "I", "V"])
@pytest.mark.parametrize("name", ps.SCENES)
def test_probe_sets_match_the_oracle(crt, name, key):
    _, s = resident(crt, name)
    p = ps.probe(crt, name, key)
    seen = []
    for depth in DEPTHS:
        got = held(s, f"{name} {key}", p.rays, p.states, depth, ps.BG, 1e-5, ps.oracle(crt, name, key, depth))
        seen.append(bits(got))
    if key != "I":  # a path that starts inside an opaque sphere never leaves it: I can be one answer at all depths
        assert not np.array_equal(seen[0], seen[3])


@pytest.mark.parametrize("name", ps.SCENES)
def test_call_t_min_other_than_the_cameras(crt, name):
    """t_min = 0 (a surface-origin segment has a root within rounding of 0 on either side), 1e-3 and
    0.5, on S and V at depth 50. At 0 the oracle's S differs from the 1e-5 run's in at least 1 % of
    the records (tests/test_probe_sets.py checks that first, without a GPU)."""
    _, s = resident(crt, name)
    for key in ("S", "V"):
        p = ps.probe(crt, name, key)
        base = ps.oracle(crt, name, key, 50)
        for t_min in T_MINS:
            want = ps.oracle(crt, name, key, 50, t_min)
            if key == "S" and t_min == 0.0:
                assert (bits(want) != bits(base)).any(1).mean() >= 0.01
            held(s, f"{name} {key}", p.rays, p.states, 50, ps.BG, t_min, want)


@pytest.mark.parametrize("k", ps.X_SCALES)
@pytest.mark.parametrize("name", ps.SCENES)
def test_scaled_first_segments(crt, name, k):
    """Directions times 2^k with t_min = 1e-5 * 2^-k: the first segment's |d| is far from 1 (shade
    normalises it for metal and glass there only), on radiance_kernel's instances."""
    _, s = resident(crt, name)
    p = ps.probe(crt, name, ("X", k))
    held(s, f"{name} X{k:+d}", p.rays, p.states, 50, ps.BG, p.t_min, ps.oracle(crt, name, ("X", k), 50))


def test_cornell_probes_at_depth_1000(crt):
    _, s = resident(crt, "cornell")
    for key in ("S", "I"):
        p = ps.probe(crt, "cornell", key)
        want = ps.oracle(crt, "cornell", key, 1000)[:2048]
        held(s, f"cornell {key}", p.rays[:2048], p.states[:2048], 1000, ps.BG, 1e-5, want)


@pytest.mark.parametrize("name", ["rtow_final", "cornell"])
def test_default_seeding_against_the_oracles_seeds(crt, name):
    """states = NULL with base_seed 0xDEADBEEF is the oracle run on its own
    oracle_sample_seed(0xDEADBEEF, i, 0): no sample_seed of the package's takes part."""
    from oracle import crt_oracle_py as orc
    d, s = resident(crt, name)
    p = ps.probe(crt, name, "S")
    base = 0xDEADBEEF
    want = orc.radiance(d, p.rays, ps.default_states(base, len(p.rays)), 50, ps.BG)
    got = held(s, f"{name} S default seeds", p.rays, None, 50, ps.BG, 1e-5, want, base_seed=base)
    assert not np.array_equal(bits(got), bits(ps.oracle(crt, name, "S", 50)))  # not the explicit states' answer


@pytest.mark.parametrize("name", ps.FIXTURE_SCENES)
def test_the_references_own_ray_color(crt, name):
    """tests/golden/radiance_<scene>.npz: the reference's Camera::ray_color on S, I, V and X records at
    depths 1, 3 and 50, with the scene's own background and its t_min = 1e-5."""
    g = load_npz(f"radiance_{name}.npz")
    d, s = resident(crt, name)
    assert str(g["scene_digest"]) == ps.scene_digest(d)
    for depth, want in zip(g["depths"], g["rgb"]):
        held(s, f"{name} fixture", g["rays"], g["states"], int(depth), g["background"], 1e-5, want)


@pytest.mark.parametrize("name", ps.SCENES)
def test_all_kinds_on_one_block(crt, monkeypatch, name):
    """S, I and V concatenated and permuted, 8192 records of them on a grid of one block: the lanes
    refill with paths of all three kinds between scattered segments."""
    _, s = resident(crt, name)
    parts = [ps.probe(crt, name, k) for k in "SIV"]
    rays = np.concatenate([p.rays for p in parts])
    states = np.concatenate([p.states for p in parts])
    want = np.concatenate([ps.oracle(crt, name, k, 50) for k in "SIV"])
    keep = np.random.default_rng(61).permutation(len(rays))[:8192]
    assert all(((keep >= lo) & (keep < hi)).sum() > 500 for lo, hi in ((0, 4096), (4096, 6144), (6144, 14336)))
    monkeypatch.setenv("CRT_GRID_BLOCKS", "1")
    held(s, f"{name} S+I+V one block", rays[keep], states[keep], 50, ps.BG, 1e-5, want[keep])
