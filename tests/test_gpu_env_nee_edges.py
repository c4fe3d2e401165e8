"""The sampled-environment instances of the radiance kernels on the worlds of tests/env_truth.py, bit for bit,
and the sampler's tables and searches at the sizes the other tests leave out.

  1. routes   every world of env_truth (CLOSED, BILINEAR, glass and the all-sphere variants), each under
              plan_worlds.route("default") and route("gstack"), the plan read through launch_plan("radiance")
              and asserted first: the worlds with a parallelogram reach the PM 1 instances, the all-sphere ones
              the sphere-only instances; default gives an LDS scene, gstack the HBM stack. A call is 4096 paths
              of the world's one ray at depths 2 and 8: probe_sets.states(2048, 87), then the four crafted
              start states (env_truth.crafted_states: xi1 .. xi4 above 1 on the floor bounce, so the clamps of
              env_sample's searches and a d_s 2.3e-10 of a texel past its texel, or past its face, go through
              the kernel), then ordinary states that pad the call to sixteen blocks of 256. The fast route's
              bytes are the plain route's and both are tests/env_nee_model.py's, and the model's Trace of this
              very call holds the world's event on the very path: below the horizon everywhere, zero_pdf on
              half_black's clamped path, sun's xi3 path free and on the next face, occluded samples under roof
              and ball, escapes with pb none after glass at depth 8.
  2. tables   Env.tables == the model's for n in {10, 11, 32, 64, 512}: 60 and 66 rows, either side of
              env_rows_kernel's block of 64 threads, 192 and 384 rows, whole blocks, and 3072 rows for the
              deepest searches tested; a random map and one whose first and last rows are empty.
  3. searches 1024 probe_sets paths of rtow_final at depth 8 under an n = 512 random map, both filters, both
              routes, equal to the model, whose picks reach row and column indices in the first, middle and
              last eighth: 12 and 9 search steps where no other radiance call takes more than 6 and 3.

n = 2048 is left out: it needs 1 GB of texels and tables; its refusal at 2049 is test_gpu_env_nee's.
Outputs are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact afterwards
(test_gpu_env_nee.run); every scene's parity guard count is 0 afterwards."""
import numpy as np
import pytest

import env_model as em
import env_nee_model as nm
import env_truth as et
import plan_worlds as pw
import probe_sets as ps
import test_gpu_env_nee as tgn
from oracle import crt_oracle_py as orc
from test_gpu_radiance import guard_stays_zero, resident  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
PLAIN = tgn.PLAIN
DEPTHS = (2, 8)
KLASS = {"default": pw.LDS_SCENE, "gstack": pw.HBM_STACK}
N_CALL = 4096
FIRST_CRAFTED = 2048

_WANT = {}


def call_states(crt, w):
    cs = et.crafted_states(crt, w)
    crafted = np.array(list(cs.values()), np.uint32)
    pad = ps.states(N_CALL - FIRST_CRAFTED - len(crafted), 88)
    return np.concatenate([ps.states(FIRST_CRAFTED, 87), crafted, pad]), [k[0] for k in cs]


def modelled(crt, w, states, depth):
    k = (w.name, depth)
    if k not in _WANT:
        want, _, tr = nm.ray_color(orc, w.d, w.rays(len(states)), states, depth, et.BG, et.T_MIN, w.env, nm.tables(w.env), crt=crt)
        want.setflags(write=False)
        _WANT[k] = (want, tr)
    return _WANT[k]


def paths_of(entries):
    return [e if isinstance(e, int) else e[0] for e in entries]


def assert_events(w, tr, depth, which):
    """The world's event, on the very path where a crafted state makes it."""
    first = {i: (r, k, xi, ds) for i, r, k, xi, ds in reversed(tr.picks)}  # a path's floor bounce is its first sample
    at = {name: FIRST_CRAFTED + j for j, name in enumerate(which)}
    for j, name in enumerate(("xi1", "xi2", "xi3", "xi4")):
        assert first[at[name]][2][j] == et.RND01_OF_MAX
    n = w.env.n
    assert first[at["xi1"]][0] == 6 * n - 1  # the clamp: the count of rows was 6n
    # sun_bilinear's nine bright texels lie whole above the horizon and take all but a few samples in ten thousand
    assert len(tr.below) >= (0 if w.name == "sun_bilinear" else 20) and len(tr.nee_free) >= N_CALL // 4
    base = w.name.split("_spheres")[0]
    if base == "half_black":
        assert at["xi1"] in tr.zero_pdf and first[at["xi1"]][1] == n - 1
    if base in ("sun", "glass", "random", "tilted"):
        r, k, xi, ds = first[at["xi3"]]
        face = int(nm.project(w.env, [ds])[1][0])
        if base == "sun":
            assert (r, k) == et.SUN_AT and face == 5 and at["xi3"] in paths_of(tr.nee_free)
        else:
            assert face == r // n
    if base in ("roof", "ball"):
        assert len(tr.nee_occluded) >= 30 and {kind for _, kind in tr.nee_occluded} == {em.LAMBERTIAN}
    if base == "glass":
        assert {kind for _, kind in tr.nee_occluded} == {em.DIELECTRIC}
        assert (len(tr.escapes_plain) >= N_CALL // 8) if depth == 8 else not tr.escapes_plain
    else:
        assert not tr.escapes_plain


# ---- 1. routes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["default", "gstack"])
@pytest.mark.parametrize("name", et.ALL)
def test_truth_worlds_and_crafted_states_are_the_model_bit_for_bit(crt, name, route):
    w = et.world(crt, name)
    states, which = call_states(crt, w)
    assert len(states) == N_CALL and N_CALL % 256 == 0 and which == ["xi1", "xi2", "xi3", "xi4"]
    rays = w.rays(N_CALL)
    with pw.route(route):
        s = crt.GpuScene(w.d)
        try:
            p = pw.plan_dict(s.launch_plan("radiance"))
            print(f"{name} under {route}: klass {p['klass']}, entry_bytes {p['entry_bytes']}, prim_mode {p['prim_mode']}")
            assert (p["klass"], p["prim_mode"]) == (KLASS[route], 0 if w.spheres_only else 1), (name, route, p)
            s.upload(0)
            env = tgn.device_env(crt, w.env, w.basis)
            for depth in DEPTHS:
                want, tr = modelled(crt, w, states, depth)
                assert_events(w, tr, depth, which)
                fast = tgn.run(s, rays, states, depth, env, bg=et.BG, t_min=et.T_MIN)
                plain = tgn.run(s, rays, states, depth, env, bg=et.BG, t_min=et.T_MIN, flags=PLAIN)
                bad = tgn.differing(fast, plain)
                assert len(bad) == 0, (name, route, depth, "fast != plain", len(bad), bad[:5], fast[bad[:3]], plain[bad[:3]])
                bad = tgn.differing(fast, want)
                assert len(bad) == 0, (name, route, depth, "fast != model", len(bad), bad[:5], states[bad[:3]], fast[bad[:3]], want[bad[:3]])
            del env
            assert s.guard(0) == 0, (name, route)
        finally:
            s.close()


# ---- 2. table sizes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 11, 32, 64, 512])
def test_tables_are_the_models_around_and_on_whole_blocks_of_rows(crt, n):
    import torch
    rng = np.random.default_rng(400 + n)
    base = rng.random((6 * n, n, 3)) * 4.0 + 0.01
    empty = base.copy()
    empty[[0, 6 * n - 1]] = 0.0
    empty[rng.permutation(6 * n)[:n]] = 0.0
    for name, texels in (("random", base), ("empty first and last rows", empty)):
        menv = em.make(texels, **tgn.ROTATED)
        tb = nm.tables(menv)
        assert nm.usable(tb)
        env = tgn.device_env(crt, menv, tgn.ROTATED)
        got = env.tables
        torch.cuda.synchronize()
        assert got.w.shape == (6 * n, n) and got.c.shape == (6 * n, n) and got.m.shape == (6 * n,)
        assert tgn.same(got.w.cpu().numpy(), tb.w), (n, name)
        assert tgn.same(got.c.cpu().numpy(), tb.c), (n, name)
        assert tgn.same(got.m.cpu().numpy(), tb.m), (n, name)
        assert tgn.same(np.array([got.W]), np.array([tb.W])), (n, name)
        if name != "random":
            assert tb.m[0] == 0 and tb.m[-1] == tb.m[-2] and (tb.c[0] == 0).all()


# ---- 3. deep searches in the kernel ---------------------------------------------------------------------
def eighths(index, size):
    x = np.asarray(index) / float(size)
    return bool((x < 0.125).any() and ((x >= 0.4375) & (x < 0.5625)).any() and (x >= 0.875).any())


@pytest.mark.parametrize("filt", tgn.FILTERS)
def test_searches_of_twelve_and_nine_steps_are_the_models(crt, filt):
    n, depth = 512, 8
    d, s = resident(crt, "rtow_final")
    rays, states = tgn.query_rays(crt, "rtow_final", 512, 512)
    assert len(rays) == 1024
    menv = em.make(tgn.random_map(n, 500), filter=filt, **tgn.ROTATED)
    rgb, _, tr = nm.ray_color(orc, d, rays, states, depth, tgn.BG, 1e-5, menv, nm.tables(menv), crt=crt)
    rows, cols = [r for _, r, _, _, _ in tr.picks], [k for _, _, k, _, _ in tr.picks]
    print(f"n = {n}, filter {filt}: {len(tr.picks)} samples, rows {min(rows)} .. {max(rows)} of {6 * n}, columns {min(cols)} .. {max(cols)}")
    assert len(tr.picks) >= 500 and eighths(rows, 6 * n) and eighths(cols, n)
    assert len(tr.nee_free) >= 50 and len(tr.nee_occluded) >= 50 and len(tr.escapes_weighted) >= 50
    env = tgn.device_env(crt, menv, tgn.ROTATED)
    fast = tgn.run(s, rays, states, depth, env)
    plain = tgn.run(s, rays, states, depth, env, flags=PLAIN)
    assert tgn.same(fast, plain), filt
    bad = tgn.differing(fast, rgb)
    assert len(bad) == 0, (filt, len(bad), bad[:5], fast[bad[:3]], rgb[bad[:3]])
