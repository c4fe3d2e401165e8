"""Every reachable environment instance of the radiance kernels on the GPU, held to tests/env_model.py
bit for bit at the smallest worlds that reach it (tests/env_cases.py; tests/test_env_instances.py checks
the table, the ray sets and the model without a GPU).

  1. instances  every row, both filters, a random map behind a rotated basis: the fast route's bytes are
                the plain route's and both are the model's; the map is seen; without an environment the
                scene still gives the constant-background model's bytes. One row with default states.
  2. refill     1536 paths on grids of 1 and 3 blocks: a lane's env_miss runs while its wave refills
  3. refused    rays the query contract refuses between traced paths of one wave
  4. edges      the lookup's face ties and texel boundaries reached by a direction the kernel made: one
                bounce off an axis-aligned mirror
  5. texels     -0.0, negative, subnormal, huge, infinite and NaN texels are carried, not inspected
  6. blocking   crt_render_lens_env with host texels is the async entry's frame, twice over
  7. probes and a lens frame on an HBM-stack world with parallelograms

Every call has at most 1536 paths at depth 8 (probes and frames: at most 325 paths at depth 50), frames
are at most 18 x 3 pixels, the largest world has 2950 objects. Outputs are pre-filled with 0xFF bytes and
followed by a sentinel tail that must be intact afterwards (test_gpu_env.run); a row's scene is built
and uploaded under its route's switches, its parity guard count is 0 afterwards and it is closed in the
row."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import env_cases as ec
import env_model as em
import lens_model as lm
import plan_worlds as pw
import probe_model as pm
import probe_sets as ps
import ray_sets as rs
import test_gpu_env as tge
import test_gpu_lens as tgl
import test_gpu_probes as tgp
from oracle import crt_oracle_py as orc
from test_env_model import ROTATED, identity_env, integer_map, probe_directions
from test_gpu_radiance import bits, guard_stays_zero, resident  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
BG, PLAIN, FILTERS, FILTER_ID = ec.BG, tge.PLAIN, tge.FILTERS, tge.FILTER_ID
DEPTH = pw.DEPTH
LABELS = [r.label for r in ec.ROWS]
TWO_ROWS = ["lds-u16-pm1", "gstack-u16-pm1"]  # the LDS-scene PM 1 row and the u16 HBM-stack PM 1 row
same = tge.same


@contextlib.contextmanager
def opened(crt, row):
    """(the row's scene on device 0, the model's paths of its ray set): the plan asserted first, the
    scene built and uploaded under the row's route, which stays set for the calls; guard 0, closed."""
    p = ec.paths(crt, row.family, row.n, orc)
    _, kw = pw.world(crt, row.family, row.n)
    with pw.route(row.route):
        s = crt.GpuScene(p.d, **kw)
        try:
            plan = ec.plan_of(s, row)
            print(f"{row.label}: {row.family} {row.n} under {row.route}, (klass, entry_bytes, prim_mode) = {plan}")
            s.upload(0)
            yield s, p
            assert s.guard(0) == 0, row.label
        finally:
            s.close()


def differing(got, want):
    return np.flatnonzero((bits(got) != bits(want)).any(1))


def held(s, p, env, want, what, bg=BG, depth=DEPTH):
    """Both routes' bytes under `env` are `want`'s; returns the fast route's."""
    fast = tge.run(s, p.rays, p.states, depth, env, bg=bg, t_min=ec.T_MIN)
    plain = tge.run(s, p.rays, p.states, depth, env, bg=bg, t_min=ec.T_MIN, flags=PLAIN)
    bad = differing(fast, plain)
    assert len(bad) == 0, (what, "fast != plain", len(bad), bad[:5], fast[bad[:3]], plain[bad[:3]])
    bad = differing(fast, want)
    assert len(bad) == 0, (what, "fast != model", len(bad), bad[:5], p.rays[bad[:3]], fast[bad[:3]], want[bad[:3]])
    return fast


# ---- 1. every instance against the model ---------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_every_instance_is_the_model_bit_for_bit(crt, label):
    """Paths are the reference's bit for bit and the lookup is correctly rounded arithmetic on both
    sides: == and nothing looser."""
    row = ec.BY_LABEL[label]
    with opened(crt, row) as (s, p):
        held(s, p, None, p.flat, (label, "constant"))  # the model's paths are the device's
        for filt in FILTERS:
            menv = em.make(tge.random_map(5, 300 + len(label)), filter=FILTER_ID[filt], **ROTATED)
            want = ec.lit_by(menv, p)
            assert not same(want, p.flat)  # the map is seen
            held(s, p, tge.device_env(crt, menv), want, (label, filt))
        held(s, p, None, p.flat, (label, "constant again"))  # env = None is the call it was


@pytest.mark.parametrize("label", TWO_ROWS)
def test_default_states_under_an_environment(crt, label):
    row = ec.BY_LABEL[label]
    base = 0xDEADBEEF
    with opened(crt, row) as (s, p):
        states = ps.default_states(base, len(p.rays))
        menv = em.make(tge.random_map(5, 41), filter=em.BILINEAR, **ROTATED)
        want, ended, _, _ = em.ray_color(orc, p.d, p.rays, states, DEPTH, BG, ec.T_MIN, env=menv, crt=crt, bvh=p.bvh)
        assert ((ended == em.MISS) & ~p.first_miss).mean() >= ec.MIN_ESCAPE_SHARE
        env = tge.device_env(crt, menv)
        for flags in (0, PLAIN):
            got = tge.run(s, p.rays, None, DEPTH, env, bg=BG, t_min=ec.T_MIN, flags=flags, base_seed=base)
            bad = differing(got, want)
            assert len(bad) == 0, (label, flags, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
        assert not same(want, tge.run(s, p.rays, None, DEPTH, env, bg=BG, t_min=ec.T_MIN, base_seed=base + 1))


# ---- 2. refill ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", TWO_ROWS)
def test_small_grids_under_an_environment(crt, monkeypatch, label):
    """1536 paths on 1 and 3 blocks: every lane takes path after path, and a lane that missed looks its
    texel up while the lanes beside it are refilled."""
    row = ec.BY_LABEL[label]
    with opened(crt, row) as (s, p):
        for filt in FILTERS:
            menv = em.make(tge.random_map(5, 51), filter=FILTER_ID[filt], **ROTATED)
            env = tge.device_env(crt, menv)
            want = ec.lit_by(menv, p)
            whole = tge.run(s, p.rays, p.states, DEPTH, env, bg=BG, t_min=ec.T_MIN)
            for blocks in ("1", "3"):
                with monkeypatch.context() as m:
                    m.setenv("CRT_GRID_BLOCKS", blocks)
                    got = tge.run(s, p.rays, p.states, DEPTH, env, bg=BG, t_min=ec.T_MIN)
                assert same(got, whole), (label, filt, blocks, "the default grid's bytes")
                bad = differing(got, want)
                assert len(bad) == 0, (label, filt, blocks, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


# ---- 3. refused rays among traced ones -------------------------------------------------------------------
@pytest.mark.parametrize("label", TWO_ROWS)
def test_refused_rays_between_traced_paths_under_an_environment(crt, label):
    """test_gpu_radiance's arrangement: one ray outside the query contract before every 23rd record, so
    each class sits in a wave of traced paths many times over. It is shaded as a first-segment miss: a
    direction with a major axis sees E(that direction), the others see the call's background."""
    row = ec.BY_LABEL[label]
    bad_rays = [r for _, r, tm in rs.invalid_rays() if tm == rs.INF]
    call_bg = (0.25, 0.5, 3.0)  # not BG: no traced path's value may depend on it
    with opened(crt, row) as (s, p):
        rr, ss, valid = [], [], []
        j = 0
        for i in range(len(p.rays)):
            if i % 23 == 5:
                rr.append(bad_rays[j % len(bad_rays)])
                ss.append(np.uint32(j * 2654435761 & 0xFFFFFFFF))
                valid.append(False)
                j += 1
            rr.append(p.rays[i])
            ss.append(p.states[i])
            valid.append(True)
        assert j >= 3 * len(bad_rays)
        rr, ss, valid = np.array(rr, np.float64), np.array(ss, np.uint32), np.array(valid)
        assert not em.traceable(rr[~valid]).any() and em.traceable(rr[valid]).all()
        dirs = rr[~valid, 3:]
        with np.errstate(all="ignore"):
            has_axis = np.isfinite(dirs).all(1) & (dirs != 0).any(1)
        assert has_axis.sum() >= 20 and (~has_axis).sum() >= 20
        for filt in FILTERS:
            menv = em.make(tge.random_map(5, 61), filter=FILTER_ID[filt], **ROTATED)
            env = tge.device_env(crt, menv)
            want = ec.lit_by(menv, p)
            refused = np.where(has_axis[:, None], em.lookup(menv, np.where(has_axis[:, None], dirs, 1.0)), np.array(call_bg))
            for flags in (0, PLAIN):
                got = tge.run(s, rr, ss, DEPTH, env, bg=call_bg, t_min=ec.T_MIN, flags=flags)
                assert same(got[valid], want), (label, filt, flags, "valid neighbours", differing(got[valid], want)[:5])
                assert same(got[~valid], refused), (label, filt, flags, "refused rays", differing(got[~valid], refused)[:5])
                assert (bits(tge.run(s, rr, ss, 0, env, bg=call_bg, t_min=ec.T_MIN, flags=flags)) == 0).all(), "depth 0"


# ---- 4. the lookup's edges after a bounce -------------------------------------------------------------------
@pytest.mark.parametrize("axis", [1, 0], ids=["normal-y", "normal-x"])
def test_face_ties_and_texel_edges_after_a_mirror_bounce(crt, axis):
    """Reflection about an exact axis normal only flips a sign and the normalisation scales x, y and z
    alike, so the ties |x| = |y|, |y| = |z| and |x| = |z| of tests/test_env_model.py's directions reach
    env_lookup in a direction that shade wrote, not the caller."""
    d = ec.mirror_world(crt, axis)
    rays = ec.mirror_rays(probe_directions(), axis)
    p = ec.model_paths(crt, orc, d, rays, ps.states(len(rays), 5), DEPTH, None)
    bounced = (p.ended == em.MISS) & ~p.first_miss
    tied = bounced & ec.ties(p.last)
    print(f"mirror with normal {'xyz'[axis]}: {len(rays)} rays, {int(bounced.sum())} bounce and escape, "
          f"{int(tied.sum())} of them on an exact tie")
    assert tied.sum() >= 10
    s = crt.GpuScene(d)
    try:
        s.upload(0)
        held(s, p, None, p.flat, (axis, "constant"))
        for filt in FILTERS:
            for menv in (identity_env(5, FILTER_ID[filt]), em.make(integer_map(5), filter=FILTER_ID[filt], **ROTATED)):
                want = ec.lit_by(menv, p)
                assert not same(want[tied], p.flat[tied])
                held(s, p, tge.device_env(crt, menv), want, (axis, filt, menv.right))
        assert s.guard(0) == 0
    finally:
        s.close()


# ---- 5. texel values are not inspected ---------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_odd_texels_are_carried_not_inspected(crt, filt):
    """NaN payloads are the hardware's business: where the model's value is NaN the device's is NaN,
    everywhere else the bits are the model's (inf - inf in BILINEAR is NaN on both sides)."""
    _, s = resident(crt, "rtow_final")
    rays, states, ended, last, T, flat = tge.paths(crt, "rtow_final", 50)
    t = ec.odd_map(4)
    assert np.isnan(t).any() and np.isinf(t).any() and (t < 0).any() and (np.signbit(t) & (t == 0)).any()
    assert ((t != 0) & (np.abs(t) < np.finfo(np.float64).tiny)).any() and (np.abs(t) == 1e300).any()
    menv = em.make(t, filter=FILTER_ID[filt], **ROTATED)
    with np.errstate(all="ignore"):
        want = tge.lit_by(menv, ended, last, T, flat)
    nan = np.isnan(want)
    miss = ended == em.MISS
    assert nan.any() and np.isinf(want).any() and (want < 0).any() and not nan[~miss].any()
    env = tge.device_env(crt, menv)
    for flags in (0, PLAIN):
        got = tge.run(s, rays, states, 50, env, flags=flags)
        assert np.array_equal(np.isnan(got), nan), (filt, flags)
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (filt, flags)
        assert same(got[~miss], flat[~miss]), (filt, flags)  # a path that met no sky keeps its bytes


# ---- 6. the blocking entry -----------------------------------------------------------------------------------
PAD = 7  # doubles of NaN either side of the host texels: a misplaced or short upload reads them


def blocking(crt, scene, cam, lens, menv):
    """crt_render_lens_env (menv None: crt_render_lens) into a host array: (h, w, 3) float64."""
    from cpp_raytracer_amd import _capi
    nbytes = cam.image_h * cam.image_w * 24
    out = np.full(nbytes + tge.TAIL, 0xFF, np.uint8)
    lib = crt.lib()
    if menv is None:
        crt.check(lib.crt_render_lens(scene.handle, 0, C.byref(cam), C.byref(lens), C.c_void_p(out.ctypes.data)),
                  "crt_render_lens")
    else:
        host = np.full(PAD + menv.texels.size + PAD, np.nan)
        host[PAD:PAD + menv.texels.size] = menv.texels.reshape(-1)
        D3 = _capi.D3
        view = _capi.EnvView(host.ctypes.data + 8 * PAD, menv.n, menv.filter, D3(*menv.right), D3(*menv.up), D3(*menv.forward))
        crt.check(lib.crt_render_lens_env(scene.handle, 0, C.byref(cam), C.byref(lens), C.byref(view),
                                          C.c_void_p(out.ctypes.data)), "crt_render_lens_env")
        assert np.array_equal(bits(host[PAD:-PAD]), bits(menv.texels.reshape(-1))) and np.isnan(host[:PAD]).all()
    assert (out[nbytes:] == 0xFF).all(), "the call wrote past its h x w x 3 values"
    return out[:nbytes].copy().view(np.float64).reshape(cam.image_h, cam.image_w, 3)


@pytest.mark.parametrize("kind", ["cube", "fisheye"])
def test_blocking_entry_with_host_texels(crt, kind):
    d, s = resident(crt, "rtow_final")
    w, h = (3, 18) if kind == "cube" else (7, 5)
    lens = tgl.lens_for(crt, d, kind)
    cam = tgl.camera(crt, d, w, h, 4)
    no_env = blocking(crt, s, cam, lens, None)
    assert same(no_env, tge.render(s, cam, lens, None))
    for n in (1, 5, 8):
        for filt in FILTERS:
            menv = em.make(tge.random_map(n, 70 + n), filter=FILTER_ID[filt], **ROTATED)
            want = tge.render(s, cam, lens, tge.device_env(crt, menv))  # test_gpu_env holds it to the model
            assert not same(want, no_env)
            assert same(blocking(crt, s, cam, lens, menv), want), (kind, n, filt)
            assert same(blocking(crt, s, cam, lens, menv), want), (kind, n, filt, "again")
    assert same(blocking(crt, s, cam, lens, None), no_env)  # the uploads left nothing behind


# ---- 7. probes and a lens frame on an HBM-stack world with parallelograms ---------------------------------
def escape_share(d, rays, t_min, bvh, ended):
    """The share of paths that end in a miss after one or more bounces."""
    first_miss = orc.hits(d, rays, t_min, **bvh)["prim"] < 0
    return float(((ended == em.MISS) & ~first_miss).mean())


def test_probes_and_a_cube_frame_on_an_hbm_stack_pm1_world(crt):
    row = ec.BY_LABEL["gstack-u16-pm1"]
    with opened(crt, row) as (s, p):
        menv = em.make(tge.random_map(5, 81), filter=em.BILINEAR, **ROTATED)
        env = tge.device_env(crt, menv)
        # five probes just off surfaces that the row's rays hit
        hit = orc.hits(p.d, p.rays, ec.T_MIN, **p.bvh)
        hit = hit[hit["prim"] >= 0]
        hit = hit[np.linspace(0, len(hit) - 1, 5).astype(int)]
        P, N = np.array(hit["point"], np.float64), np.array(hit["normal"], np.float64)
        P = P + 1e-4 * max(1.0, float(np.abs(P).max())) * N
        S = 65
        rays, states = tgp.generate(s, P, N, S, "sphere")
        L = tge.run(s, rays, states, 50, env)
        model, ended, _, _ = em.ray_color(orc, p.d, rays, states, 50, BG, 1e-5, env=menv, crt=crt, bvh=p.bvh)
        assert same(L, model) and escape_share(p.d, rays, 1e-5, p.bvh, ended) >= ec.MIN_ESCAPE_SHARE
        assert not same(L, tge.run(s, rays, states, 50, None))  # the probes see the map
        want = pm.reduce(rays[:, 3:], L, S, True)
        for batch in (0, 2):
            assert same(tge.bake(s, P, N, S, "sphere", env, batch), want), batch
        assert same(tge.bake(s, P, N, S, "sphere", env, 2, PLAIN), want)
        # a CUBE frame from the first probe: a surface below it, the cluster around it
        n, spp = 3, 4
        lens = tgl.lens_for(crt, p.d, "cube", origin=tuple(P[0].tolist()))
        cam = tgl.camera(crt, p.d, n, 6 * n, spp)
        rays, states = tgl.device_rays(s, cam, lens)
        L = tge.run(s, rays, states, tgl.DEPTH, env, bg=BG, t_min=cam.t_min)
        model, ended, _, _ = em.ray_color(orc, p.d, rays, states, tgl.DEPTH, BG, cam.t_min, env=menv, crt=crt, bvh=p.bvh)
        assert same(L, model) and escape_share(p.d, rays, cam.t_min, p.bvh, ended) >= ec.MIN_ESCAPE_SHARE
        want = lm.frame(L.reshape(6 * n, n, spp, 3), crt.sample_chunk_len(spp))
        assert same(tge.render(s, cam, lens, env), want)
        assert same(tge.render(s, cam, tgl.with_batch(lens, 7, plain=True), env), want)
        assert not same(want, tge.render(s, cam, lens, None))  # the frame sees the map
