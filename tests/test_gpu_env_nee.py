"""Luminance-sampled environments on the GPU: crt_env_sampler_create, crt_radiance_env_sampled_async,
crt_probes_env_sampled_async, crt_render_lens_env_sampled_async and crt_render_lens_env_sampled
through the Python front end, held to tests/env_nee_model.py bit for bit.

  1. tables     Env.tables equals the model's w, c, m and W; maps whose total is 0 or +inf are refused
  2. radiance   the fast route's bytes are the plain route's and both are the model's
  3. capacity   1, 65 and 4097 paths, a side stream, default states, depth 0
  4. refusals   rays the contract refuses among valid ones; shadow rays stopped by glass and by lights
  5. probes     the bake is probe_model's reduction of the sampled radiance query
  6. lens       the frame is lens_model's reduction of the sampled radiance query; the blocking entry
                with host texels gives the async frame
  7. existing   radiance(env=) without importance and without env give the bytes they gave

A call has at most 4097 paths, frames are at most 7 x 5 or 3 x 18 pixels, maps have n in {1, 2, 5, 8, 65}.
Outputs are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact afterwards.
Every scene's parity guard count is 0 after every test (test_gpu_radiance's fixture)."""
import ctypes as C
import math

import numpy as np
import pytest

import env_model as em
import env_nee_model as nm
import lens_model as lm
import probe_model as pm
import probe_sets as ps
import test_gpu_lens as tgl
import test_gpu_probes as tgp
import test_gpu_radiance as tgr
from oracle import crt_oracle_py as orc
from test_env_model import ROTATED
from test_env_nee_model import special_maps
from test_gpu_radiance import bits, guard_stays_zero, resident  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
BG = (0.35, 0.6, 1.25)  # three distinct channels, none of them a scene's own
TAIL = 9
PLAIN = 1
FILTERS = [em.NEAREST, em.BILINEAR]

_MODEL = {}


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def device_env(crt, menv, basis, importance=True):
    """The package's Env of a model Env made with em.make(..., **basis): the same texels on device 0, the
    same basis (make_env builds it with em.basis's numpy lines), the same filter, with a sampler."""
    import torch
    t = torch.from_numpy(np.array(menv.texels)).cuda()
    env = crt.make_env(t, filter=menv.filter, importance=importance, **basis)
    assert (tuple(env.view.right), tuple(env.view.up), tuple(env.view.forward)) == (menv.right, menv.up, menv.forward)
    return env


def run(scene, rays, states, depth, env, bg=BG, t_min=1e-5, flags=0, base_seed=0, stream=None):
    """One crt_radiance_env_sampled_async call on device 0: (n, 3) float64."""
    import torch
    n = len(rays)
    buf = torch.full((n + TAIL, 6), math.nan, dtype=torch.float64, device="cuda")
    buf[:n] = torch.from_numpy(np.array(rays, np.float64))
    st = None
    if states is not None:
        st = torch.full((n + TAIL,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        st[:n] = torch.from_numpy(np.array(states, np.uint32).view(np.int32))
    out = torch.full((n + TAIL, 24), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scene.radiance_async(0, buf.data_ptr(), n, out.data_ptr(), st.data_ptr() if st is not None else 0,
                         max_depth=depth, background=bg, t_min=t_min, base_seed=base_seed, flags=flags,
                         stream=(stream or torch.cuda.current_stream()).cuda_stream, sampler=env.sampler)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[n:] == 0xFF).all(), "the call wrote past its n records"
    return host[:n].copy().view(np.float64).reshape(n, 3)


def random_map(n, seed):
    return np.random.default_rng(seed).random((6 * n, n, 3)) * 4.0


def bright_map(n, row, col):
    t = np.full((6 * n, n, 3), 0.5)
    t[row, col] = 1e4
    return t


def query_rays(crt, name, n_s, n_v):
    s, v = ps.probe(crt, name, "S"), ps.probe(crt, name, "V")
    return np.concatenate([s.rays[:n_s], v.rays[:n_v]]), np.concatenate([s.states[:n_s], v.states[:n_v]])


def model(crt, d, key, rays, states, depth, menv, t_min=1e-5):
    """The model's output and Trace, computed once per key and left unchanged."""
    if key not in _MODEL:
        rgb, ended, tr = nm.ray_color(orc, d, rays, states, depth, BG, t_min, menv, nm.tables(menv), crt=crt)
        rgb.setflags(write=False)
        _MODEL[key] = (rgb, ended, tr)
    return _MODEL[key]


def differing(got, want):
    return np.flatnonzero((bits(got) != bits(want)).any(1))


# ---- 1. tables --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 8, 65])
def test_tables_are_the_models(crt, n):
    import torch
    seen = 0
    for name, texels in special_maps(n, 300 + n).items():
        menv = em.make(texels, **ROTATED)
        tb = nm.tables(menv)
        if not nm.usable(tb):
            continue
        env = device_env(crt, menv, ROTATED)
        got = env.tables
        torch.cuda.synchronize()
        assert got.w.shape == (6 * n, n) and got.c.shape == (6 * n, n) and got.m.shape == (6 * n,)
        assert same(got.w.cpu().numpy(), tb.w), (n, name)
        assert same(got.c.cpu().numpy(), tb.c), (n, name)
        assert same(got.m.cpu().numpy(), tb.m), (n, name)
        assert same(np.array([got.W]), np.array([tb.W])), (n, name)
        seen += 1
    assert seen >= 3  # the random map, the one with -0.0, negatives and NaN, and one with empty parts


def test_maps_without_a_usable_total_are_refused(crt):
    import torch
    n = 4
    big = np.full((6 * n, n, 3), 1.7e308)       # finite texels whose sum overflows
    one_inf = np.full((6 * n, n, 3), 0.5)
    one_inf[7, 2, 1] = math.inf
    for name, texels in (("zeros", np.zeros((6 * n, n, 3))), ("nan", np.full((6 * n, n, 3), math.nan)),
                         ("negative", np.full((6 * n, n, 3), -1.0)), ("overflow", big), ("inf", one_inf)):
        assert not nm.usable(nm.tables(em.make(texels))), name
        with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_env_sampler_create: the map's total weight W"):
            crt.make_env(torch.from_numpy(texels).cuda(), importance=True)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*face_size must be at most 2048"):
        crt.make_env(torch.zeros((6 * 2049, 2049, 3), dtype=torch.float64, device="cuda"), importance=True)


# ---- 2. radiance ------------------------------------------------------------------------------------
def test_the_two_scenes_are_an_lds_scene_and_an_hbm_scene(crt):
    from cpp_raytracer_amd import _capi
    klass = {name: resident(crt, name)[1].launch_plan("radiance").klass for name in ("rtow_final", "christmas_tree")}
    assert klass["rtow_final"] == _capi.CRT_PLAN_LDS_SCENE and klass["christmas_tree"] != _capi.CRT_PLAN_LDS_SCENE, klass


@pytest.mark.parametrize("depth", [1, 2, 3, 50])
@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree"])
def test_both_routes_are_the_model_bit_for_bit(crt, name, depth):
    d, s = resident(crt, name)
    rays, states = query_rays(crt, name, 384, 384)
    for filt in FILTERS:
        n = 5 if filt == em.NEAREST else 8
        menv = em.make(random_map(n, 100 + n), filter=filt, **ROTATED)
        want, _, tr = model(crt, d, (name, depth, filt), rays, states, depth, menv)
        env = device_env(crt, menv, ROTATED)
        fast = run(s, rays, states, depth, env)
        plain = run(s, rays, states, depth, env, flags=PLAIN)
        assert same(fast, plain), (name, depth, filt)
        bad = differing(fast, want)
        assert len(bad) == 0, (name, depth, filt, len(bad), bad[:5], fast[bad[:3]], want[bad[:3]])
        if depth > 1:  # the estimator is exercised: samples that arrive, samples that are stopped, weighted escapes
            assert len(tr.nee_free) >= 5 and len(tr.nee_occluded) >= 5 and len(tr.escapes_weighted) >= 5
        else:          # and with one segment it is the unsampled entry, byte for byte
            import test_gpu_env as tge
            assert same(fast, tge.run(s, rays, states, 1, device_env(crt, menv, ROTATED, importance=False)))


# ---- 3. capacity ------------------------------------------------------------------------------------
def test_one_to_4097_paths_a_side_stream_default_states_and_depth_zero(crt):
    import torch
    d, s = resident(crt, "rtow_final")
    rays, states = query_rays(crt, "rtow_final", 4096, 1)
    assert len(rays) == 4097
    menv = em.make(random_map(4, 9), **ROTATED)
    want, _, _ = model(crt, d, ("capacity",), rays, states, 50, menv)
    env = device_env(crt, menv, ROTATED)
    side = torch.cuda.Stream()
    for n in (1, 65, 4097):
        for flags in (0, PLAIN):
            assert same(run(s, rays[:n], states[:n], 50, env, flags=flags), want[:n]), (n, flags)
        assert same(run(s, rays[:n], states[:n], 50, env, stream=side), want[:n]), n
    base = 77
    want, _, _ = model(crt, d, ("default states",), rays[:65], ps.default_states(base, 65), 50, menv)
    for flags in (0, PLAIN):
        assert same(run(s, rays[:65], None, 50, env, flags=flags, base_seed=base), want), flags
    assert not run(s, rays[:65], states[:65], 0, env).any()  # depth 0: +0, no launch


# ---- 4. refused rays and occlusion ------------------------------------------------------------------
def test_refused_rays_among_valid_ones_and_occluders_of_every_kind(crt):
    name = "rtow_final_lights"
    d = ps.scene_data(crt, name)
    s = crt.GpuScene(d)
    s.upload(0)
    p = ps.probe(crt, name, "S")
    nan, inf = math.nan, math.inf
    refused = np.array([[nan, 0, 0, 0, 1, 0.5], [0, 2e4, 0, 0, 0, 0], [0, 2e4, 0, nan, 1, 0], [0, 2e4, 0, 1, inf, 0],
                        [inf, 0, 0, 1, 0, 0]], np.float64)
    rays, states = np.array(p.rays[:1024]), np.array(p.states[:1024])
    where = np.array([0, 63, 64, 500, 1023])
    rays[where] = refused
    assert not em.traceable(rays)[where].any() and em.traceable(rays).sum() == 1024 - 5
    row, col = 4 * 8 + 3, 3  # a texel of the +Z face at the horizon: the shadow rays skim the ground, where the lights lie
    for filt in FILTERS:
        menv = em.make(bright_map(8, row, col), filter=filt)
        want, ended, tr = model(crt, d, ("refused", filt), rays, states, 50, menv)
        assert (ended[where] == em.MISS).all() and set(where.tolist()) <= set(tr.escapes_plain)
        # a refused ray sees E(its own direction) with f = 1, or the background where it has no major axis
        assert same(want[where[0]], em.lookup(menv, [refused[0, 3:]], BG)[0]) and same(want[where[1]], np.array(BG))
        kinds = {k for _, k in tr.nee_occluded}
        assert {em.LAMBERTIAN, em.DIELECTRIC, em.DIFFUSE_LIGHT} <= kinds, kinds
        env = device_env(crt, menv, {})
        for flags in (0, PLAIN):
            got = run(s, rays, states, 50, env, flags=flags)
            bad = differing(got, want)
            assert len(bad) == 0, (filt, flags, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    assert s.guard(0) == 0


def test_a_sampler_of_another_device_is_refused(crt):
    import torch
    _, s = resident(crt, "rtow_final")
    env = crt.make_env(torch.ones((6, 1, 3), dtype=torch.float64, device="cuda"), importance=True)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_radiance_env_sampled_async: the sampler was built on device 0"):
        s.radiance_async(1, 1 << 20, 4, 1 << 21, max_depth=5, background=BG, sampler=env.sampler)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_probes_env_sampled_async: the sampler was built on device 0"):
        s.probes_async(1, 1 << 20, 0, 4, 1 << 21, samples=4, max_depth=5, background=BG, sampler=env.sampler)


# ---- 5. probes --------------------------------------------------------------------------------------
def bake(scene, P, N, S, mode, env, batch=0, flags=0):
    import torch
    out = scene.probes(tgp.device(P), tgp.device(N) if mode == "hemisphere" else None, samples=S, mode=mode,
                       max_depth=50, background=BG, base_seed=tgp.SEED, batch_probes=batch, plain=bool(flags), env=env)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("mode", ["sphere", "hemisphere"])
def test_bake_is_the_models_reduction_of_the_sampled_radiance_query(crt, mode):
    import test_gpu_env as tge
    _, s = resident(crt, "rtow_final")
    P, N = tgp.probe_points(crt, "rtow_final")
    P, N = P[:5], N[:5]
    S = 65
    menv = em.make(random_map(5, 11), **ROTATED)
    env = device_env(crt, menv, ROTATED)
    rays, states = tgp.generate(s, P, N, S, mode)
    L = run(s, rays, states, 50, env)
    unsampled = device_env(crt, menv, ROTATED, importance=False)
    assert not same(L, tge.run(s, rays, states, 50, unsampled))  # the probes' paths sample the map
    want = pm.reduce(rays[:, 3:], L, S, mode == "sphere")
    for batch in (0, 2, 5):
        assert same(bake(s, P, N, S, mode, env, batch), want), (mode, batch)
    assert same(bake(s, P, N, S, mode, env, 2, PLAIN), want)
    # without importance the call is the one it was
    assert same(bake(s, P, N, S, mode, unsampled), pm.reduce(rays[:, 3:], tge.run(s, rays, states, 50, unsampled), S, mode == "sphere"))


# ---- 6. lens ----------------------------------------------------------------------------------------
def render(scene, cam, lens, env):
    import torch
    out = scene.render_lens(cam, lens, env=env)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["cube", "fisheye"])
def test_frame_is_the_models_reduction_of_the_sampled_radiance_query(crt, kind):
    d, s = resident(crt, "rtow_final")
    w, h = (3, 18) if kind == "cube" else (7, 5)
    lens = tgl.lens_for(crt, d, kind)
    menv = em.make(random_map(8, 13), **ROTATED)
    env = device_env(crt, menv, ROTATED)
    unsampled = device_env(crt, menv, ROTATED, importance=False)
    for spp in (1, 4, 5):
        cam = tgl.camera(crt, d, w, h, spp)
        rays, states = tgl.device_rays(s, cam, lens)
        L = run(s, rays, states, tgl.DEPTH, env, bg=BG, t_min=cam.t_min)
        want = lm.frame(L.reshape(h, w, spp, 3), crt.sample_chunk_len(spp))
        for batch in (0, 2, w * h):
            assert same(render(s, cam, tgl.with_batch(lens, batch), env), want), (kind, spp, batch)
        assert same(render(s, cam, tgl.with_batch(lens, 2, plain=True), env), want), (kind, spp)
        assert not same(want, render(s, cam, lens, unsampled))  # the frame's paths sample the map
    # the blocking entry with host texels: it uploads them, builds a sampler, renders, frees both
    host = np.ascontiguousarray(menv.texels)
    view = type(env.view).from_buffer_copy(bytes(env.view))
    view.texels = host.ctypes.data
    out = np.full((h, w, 3), math.nan)
    crt.check(crt.lib().crt_render_lens_env_sampled(s.handle, 0, C.byref(cam), C.byref(lens), C.byref(view),
                                                    C.c_void_p(out.ctypes.data)), "crt_render_lens_env_sampled")
    assert same(out, want)


# ---- 7. existing entries ------------------------------------------------------------------------------
def test_entries_without_a_sampler_give_the_bytes_they_gave(crt):
    import torch
    d, s = resident(crt, "rtow_final")
    rays, states = query_rays(crt, "rtow_final", 384, 384)
    menv = em.make(random_map(5, 21), **ROTATED)
    flat, ended, last, T = em.ray_color(orc, d, rays, states, 50, BG, 1e-5, crt=crt)
    lit = np.array(flat)
    miss = ended == em.MISS
    lit[miss] = 0.0 + T[miss] * em.lookup(menv, last[miss], BG)
    sampled = device_env(crt, menv, ROTATED)           # a sampler exists next to the plain Env: it changes nothing
    unsampled = device_env(crt, menv, ROTATED, importance=False)
    r = torch.from_numpy(rays).cuda()
    st = torch.from_numpy(states.view(np.int32)).cuda()
    for plain in (False, True):
        got = s.radiance(r, st, 50, BG, plain=plain, env=unsampled)
        none = s.radiance(r, st, 50, BG, plain=plain)
        torch.cuda.synchronize()
        assert same(got.cpu().numpy(), lit) and same(none.cpu().numpy(), flat), plain
    got = s.radiance(r, st, 50, BG, env=sampled)
    torch.cuda.synchronize()
    assert same(got.cpu().numpy(), nm.ray_color(orc, d, rays, states, 50, BG, 1e-5, menv, nm.tables(menv), crt=crt)[0])
    assert unsampled.sampler is None and sampled.sampler
