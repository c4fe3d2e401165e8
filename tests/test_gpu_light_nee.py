"""The scene's own lights sampled on the GPU: crt_light_sampler_create, crt_radiance_lights_async,
crt_probes_lights_async, crt_render_lens_lights_async and crt_render_lens_lights through the Python front
end, held to tests/light_nee_model.py bit for bit.

  1. tables     LightSampler.tables equals the model's prim, w, cdf and W on five worlds; scenes without a
                light or without a usable total are refused, and so is a sampler of another scene or device
  2. radiance   both routes give the model's bytes at depths 1, 2, 3 and 50 on cornell, rtow_final_lights
                (an LDS scene) and christmas_tree (HBM), after the model's trace showed every event the
                scene can produce (light_cases.EVENTS)
  3. capacity   1, 65 and 4097 paths, a side stream, default states, depth 0
  4. identities depth 1 and the paths without a Lambertian bounce are radiance()'s bytes
  5. probes     the bake is probe_model's reduction of the sampled radiance query
  6. lens       a CUBE and a fisheye frame are lens_model's reduction of the sampled radiance query; the
                blocking entry gives the async frame
  7. existing   radiance() without lights gives the bytes it gave

A call has at most 4097 paths and some tens of mirror rays; frames are at most 7 x 5 or 3 x 18 pixels.
Outputs are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact afterwards.
Every scene's parity guard count is 0 after every test (test_gpu_radiance's fixture)."""
import ctypes as C
import math

import numpy as np
import pytest

import env_model as em
import lens_model as lensm
import light_cases as lc
import light_nee_model as lm
import probe_model as pm
import probe_sets as ps
import test_gpu_lens as tgl
import test_gpu_probes as tgp
import test_gpu_radiance as tgr
from oracle import crt_oracle_py as orc
from test_gpu_radiance import bits, guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
BG = (0.35, 0.6, 1.25)  # three distinct channels, none of them a scene's own
TAIL = 9
PLAIN = 1
SCENES = ["cornell", "rtow_final_lights", "christmas_tree"]

_MODEL, _SAMPLER = {}, {}


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def resident(crt, name):
    """test_gpu_radiance.resident for probe_sets' scenes (rtow_final_lights among them), kept in its table:
    its guard fixture covers them too."""
    if name not in tgr._SCENES:
        d = ps.scene_data(crt, name)
        s = crt.GpuScene(d)
        s.upload(0)
        tgr._SCENES[name] = (d, s)
    return tgr._SCENES[name]


def sampler(crt, name):
    """The scene's LightSampler on device 0, built once."""
    if name not in _SAMPLER:
        _SAMPLER[name] = resident(crt, name)[1].light_sampler(0)
    return _SAMPLER[name]


def run(scene, rays, states, depth, lights, bg=BG, t_min=1e-5, flags=0, base_seed=0, stream=None):
    """One crt_radiance_lights_async call on device 0 (crt_radiance_async with lights None): (n, 3) float64."""
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
                         stream=(stream or torch.cuda.current_stream()).cuda_stream,
                         lights=lights.handle if lights is not None else 0)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[n:] == 0xFF).all(), "the call wrote past its n records"
    return host[:n].copy().view(np.float64).reshape(n, 3)


def model(crt, d, key, rays, states, depth, t_min=1e-5, bg=BG):
    """The model's output, endings and Trace, computed once per key and left unchanged."""
    if key not in _MODEL:
        rgb, ended, tr = lm.ray_color(orc, d, rays, states, depth, bg, t_min, lm.tables(d), crt=crt)
        rgb.setflags(write=False)
        _MODEL[key] = (rgb, ended, tr)
    return _MODEL[key]


def differing(got, want):
    return np.flatnonzero((bits(got) != bits(want)).any(1))


# ---- 1. tables --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.WORLDS)
def test_tables_are_the_models(crt, name):
    d, kw = lc.world(crt, name)
    tb = lm.tables(d)
    assert lm.usable(tb)
    s = crt.GpuScene(d, **kw)
    got = s.light_sampler(0).tables
    assert got.prim.dtype == np.uint32 and np.array_equal(got.prim, tb.prim), name
    assert same(got.w, tb.w) and same(got.cdf, tb.cdf) and same(np.array([got.W]), np.array([tb.W])), name
    # picks do not depend on the BVH parameters, nor on where the tree was built
    other = crt.GpuScene(d, num_buckets=8, max_prims_in_node=3, build_device=0).light_sampler(0).tables
    assert np.array_equal(other.prim, tb.prim) and same(other.w, tb.w) and same(other.cdf, tb.cdf)


def test_scenes_without_a_usable_sampler_and_foreign_samplers_are_refused(crt):
    z = lc.odd_lights_world(crt, only_zero=True)
    assert not lm.usable(lm.tables(z))
    with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_light_sampler_create: the lights' total weight W"):
        crt.GpuScene(z).light_sampler(0)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_light_sampler_create: the scene has no light"):
        crt.GpuScene(crt.SceneData.named("config1")).light_sampler(0)
    ok = crt.GpuScene(lc.odd_lights_world(crt))
    smp = ok.light_sampler(0)
    assert same(smp.tables.w, lm.tables(lc.odd_lights_world(crt)).w)
    _, s = resident(crt, "cornell")
    with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_radiance_lights_async: the light sampler was built for another scene"):
        s.radiance_async(0, 1 << 20, 4, 1 << 21, max_depth=5, background=BG, lights=smp.handle)
    with pytest.raises(crt.CrtError, match=r"\(-1\).*crt_probes_lights_async: the light sampler was built on device 0"):
        ok.probes_async(1, 1 << 20, 0, 4, 1 << 21, samples=4, max_depth=5, background=BG, lights=smp.handle)
    import torch
    r = torch.zeros((4, 6), dtype=torch.float64, device="cuda")
    with pytest.raises(crt.CrtError, match="radiance: the LightSampler belongs to another scene or device"):
        s.radiance(r, lights=smp)
    with pytest.raises(ValueError, match="radiance: lights= and env= cannot be combined"):
        ok.radiance(r, lights=smp, env=crt.make_env(torch.ones((6, 1, 3), dtype=torch.float64, device="cuda")))


# ---- 2. radiance ------------------------------------------------------------------------------------
def test_the_scenes_are_two_lds_scenes_and_an_hbm_scene(crt):
    from cpp_raytracer_amd import _capi
    klass = {name: resident(crt, name)[1].launch_plan("radiance").klass for name in SCENES}
    assert klass["rtow_final_lights"] == klass["cornell"] == _capi.CRT_PLAN_LDS_SCENE
    assert klass["christmas_tree"] != _capi.CRT_PLAN_LDS_SCENE, klass


@pytest.mark.parametrize("depth", [1, 2, 3, 50])
@pytest.mark.parametrize("name", SCENES)
def test_both_routes_are_the_model_bit_for_bit(crt, name, depth):
    d, s = resident(crt, name)
    rays, states = lc.query(crt, name)
    want, _, tr = model(crt, d, (name, depth), rays, states, depth)
    if depth == 50:  # the estimator is exercised: every event the scene can show, before any byte is compared
        seen = lc.counts(tr)
        assert all(seen[e] >= 1 for e in lc.EVENTS[name]), (name, seen)
        if name == "rtow_final_lights":
            assert set(lc.EVENTS[name]) == set(lc.ALL_EVENTS)
    smp = sampler(crt, name)
    fast = run(s, rays, states, depth, smp)
    plain = run(s, rays, states, depth, smp, flags=PLAIN)
    assert same(fast, plain), (name, depth)
    bad = differing(fast, want)
    assert len(bad) == 0, (name, depth, len(bad), bad[:5], fast[bad[:3]], want[bad[:3]])
    if depth > 1:
        assert not same(fast, run(s, rays, states, depth, None))  # the paths sample the lights


# ---- 3. capacity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_one_to_4097_paths_a_side_stream_default_states_and_depth_zero(crt, name):
    import torch
    d, s = resident(crt, name)
    rays, states = lc.query(crt, name)
    assert len(rays) >= 4097
    want, _, _ = model(crt, d, (name, 50), rays, states, 50)
    smp = sampler(crt, name)
    side = torch.cuda.Stream()
    for n in (1, 65, 4097):
        for flags in (0, PLAIN):
            assert same(run(s, rays[:n], states[:n], 50, smp, flags=flags), want[:n]), (n, flags)
        assert same(run(s, rays[:n], states[:n], 50, smp, stream=side), want[:n]), n
    base = 77
    want, _, _ = model(crt, d, (name, "default states"), rays[:65], ps.default_states(base, 65), 50)
    for flags in (0, PLAIN):
        assert same(run(s, rays[:65], None, 50, smp, flags=flags, base_seed=base), want), flags
    assert not run(s, rays[:65], states[:65], 0, smp).any()  # depth 0: +0, no launch


def test_refused_rays_stay_first_segment_misses(crt):
    d, s = resident(crt, "rtow_final_lights")
    rays, states = (np.array(a[:1024]) for a in lc.query(crt, "rtow_final_lights"))
    nan, inf = math.nan, math.inf
    where = np.array([0, 63, 64, 500, 1023])
    rays[where] = np.array([[nan, 0, 0, 0, 1, 0.5], [0, 2e4, 0, 0, 0, 0], [0, 2e4, 0, nan, 1, 0], [0, 2e4, 0, 1, inf, 0],
                            [inf, 0, 0, 1, 0, 0]], np.float64)
    assert not em.traceable(rays)[where].any()
    want, ended, _ = model(crt, d, ("refused",), rays, states, 50)
    assert (ended[where] == em.MISS).all() and same(want[where], np.broadcast_to(np.array(BG), (5, 3)))
    for flags in (0, PLAIN):
        assert same(run(s, rays, states, 50, sampler(crt, "rtow_final_lights"), flags=flags), want), flags


# ---- 4. the identities ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_identities_with_radiance(crt, name):
    d, s = resident(crt, name)
    rays, states = lc.query(crt, name)
    smp = sampler(crt, name)
    for flags in (0, PLAIN):
        assert same(run(s, rays, states, 1, smp, flags=flags), run(s, rays, states, 1, None, flags=flags)), flags
    _, _, tr = model(crt, d, (name, 50), rays, states, 50)
    plain = np.ones(len(rays), bool)
    plain[list(tr.lambertian)] = False
    assert plain.sum() >= 50 and (~plain).sum() >= 50
    got, flat = run(s, rays, states, 50, smp), run(s, rays, states, 50, None)
    assert same(got[plain], flat[plain]) and not same(got[~plain], flat[~plain])


# ---- 5. probes --------------------------------------------------------------------------------------
def bake(scene, P, N, S, mode, lights, batch=0, flags=0):
    import torch
    out = scene.probes(tgp.device(P), tgp.device(N) if mode == "hemisphere" else None, samples=S, mode=mode,
                       max_depth=50, background=BG, base_seed=tgp.SEED, batch_probes=batch, plain=bool(flags), lights=lights)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("mode", ["sphere", "hemisphere"])
def test_bake_is_the_models_reduction_of_the_sampled_radiance_query(crt, mode):
    _, s = resident(crt, "cornell")
    P, N = tgp.probe_points(crt, "cornell")
    P, N = P[:5], N[:5]
    S = 65
    smp = sampler(crt, "cornell")
    rays, states = tgp.generate(s, P, N, S, mode)
    L = run(s, rays, states, 50, smp)
    assert not same(L, run(s, rays, states, 50, None))  # the probes' paths sample the light
    want = pm.reduce(rays[:, 3:], L, S, mode == "sphere")
    for batch in (0, 2, 5):
        assert same(bake(s, P, N, S, mode, smp, batch), want), (mode, batch)
    assert same(bake(s, P, N, S, mode, smp, 2, PLAIN), want)
    # without lights the call is the one it was
    assert same(bake(s, P, N, S, mode, None), pm.reduce(rays[:, 3:], run(s, rays, states, 50, None), S, mode == "sphere"))


# ---- 6. lens ----------------------------------------------------------------------------------------
def render(scene, cam, lens, lights):
    import torch
    out = scene.render_lens(cam, lens, lights=lights)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["cube", "fisheye"])
def test_frame_is_the_models_reduction_of_the_sampled_radiance_query(crt, kind):
    d, s = resident(crt, "cornell")
    w, h = (3, 18) if kind == "cube" else (7, 5)
    lens = tgl.lens_for(crt, d, kind, origin=tgl.INSIDE_CORNELL)
    smp = sampler(crt, "cornell")
    for spp in (1, 4, 5):
        cam = tgl.camera(crt, d, w, h, spp)
        rays, states = tgl.device_rays(s, cam, lens)
        L = run(s, rays, states, tgl.DEPTH, smp, bg=tuple(cam.background), t_min=cam.t_min)
        want = lensm.frame(L.reshape(h, w, spp, 3), crt.sample_chunk_len(spp))
        for batch in (0, 2, w * h):
            assert same(render(s, cam, tgl.with_batch(lens, batch), smp), want), (kind, spp, batch)
        assert same(render(s, cam, tgl.with_batch(lens, 2, plain=True), smp), want), (kind, spp)
        assert not same(want, render(s, cam, lens, None))  # the frame's paths sample the light
    # the blocking entry: it builds a sampler of its own, renders, frees it
    out = np.full((h, w, 3), math.nan)
    crt.check(crt.lib().crt_render_lens_lights(s.handle, 0, C.byref(cam), C.byref(lens), C.c_void_p(out.ctypes.data)),
              "crt_render_lens_lights")
    assert same(out, want)


# ---- 7. existing entries ------------------------------------------------------------------------------
def test_radiance_without_lights_gives_the_bytes_it_gave(crt):
    import torch
    d, s = resident(crt, "rtow_final_lights")
    rays, states = (a[:768] for a in lc.query(crt, "rtow_final_lights", 384, 384))
    flat = em.ray_color(orc, d, rays, states, 50, BG, 1e-5, crt=crt)[0]
    smp = sampler(crt, "rtow_final_lights")  # a sampler exists next to the scene: it changes nothing
    r = torch.from_numpy(rays).cuda()
    st = torch.from_numpy(states.view(np.int32)).cuda()
    for plain in (False, True):
        none = s.radiance(r, st, 50, BG, plain=plain)
        torch.cuda.synchronize()
        assert same(none.cpu().numpy(), flat), plain
    got = s.radiance(r, st, 50, BG, lights=smp)
    torch.cuda.synchronize()
    assert same(got.cpu().numpy(), lm.ray_color(orc, d, rays, states, 50, BG, 1e-5, lm.tables(d), crt=crt)[0])
