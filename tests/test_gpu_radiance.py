"""crt_radiance_async and crt_camera_rays_async on the GPU. A camera's own rays are a special case
of a radiance query, so the entry is checked exactly: with the rays and LCG states of
crt_camera_rays_async (themselves equal to tests/radiance_model.py's), the per-path radiance summed
as the render kernel sums it is crt_render_async's frame bit for bit, and it is the oracle's
per-sample radiance. The fast route (radiance_kernel) and the plain route (CRT_RADIANCE_PLAIN) give
the same bits on every instance and under every switch.
Buffers are device tensors: the rays are followed by NaN rays past n, outputs are pre-filled with
0xFF bytes and followed by a sentinel tail that must be intact afterwards. Every scene's parity
guard count is 0 after every test."""
import math

import numpy as np
import pytest

import denoise_model as dm
import radiance_model as rm
import ray_sets as rs
from oracle import crt_oracle_py as orc
from test_gpu_trace import SWITCHES

pytestmark = pytest.mark.gpu
TAIL = 9
PLAIN = 1
W, H = 48, 32
SEED = 21
SCENES = ["rtow_final", "cornell", "mixed", "christmas_tree", "big"]

_SCENES, _JOBS = {}, {}


def resident(crt, name):
    """(SceneData, GpuScene on device 0), built under the default switches and kept for the module."""
    if name not in _SCENES:
        d = rs.scene_data(crt, name)
        s = crt.GpuScene(d)
        s.upload(0)
        _SCENES[name] = (d, s)
    return _SCENES[name]


@pytest.fixture(autouse=True)
def guard_stays_zero():
    yield
    for name, (_, s) in _SCENES.items():
        assert s.guard(0) == 0, name


def camera(crt, d, spp=4, depth=50, w=W, h=H):
    from cpp_raytracer_amd import camera_with
    return crt.resolve_camera(camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp, max_depth=depth), SEED)


def device_rays(scene, cam, **kw):
    import torch
    rays, states = scene.camera_rays(cam, **kw)
    torch.cuda.synchronize()
    return rays.cpu().numpy(), states.cpu().numpy().view(np.uint32)


def run(scene, rays, states=None, depth=50, bg=(0.7, 0.8, 1.0), t_min=1e-5, flags=0, base_seed=0, n=None):
    """One crt_radiance_async call on device 0 and the current stream: (n, 3) float64."""
    import torch
    n = len(rays) if n is None else n
    buf = torch.full((n + TAIL, 6), math.nan, dtype=torch.float64, device="cuda")
    buf[:n] = torch.from_numpy(np.array(rays[:n], np.float64))
    st = None
    if states is not None:
        st = torch.full((n + TAIL,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        st[:n] = torch.from_numpy(np.array(states[:n], np.uint32).view(np.int32))
    out = torch.full((n + TAIL, 24), 0xFF, dtype=torch.uint8, device="cuda")
    scene.radiance_async(0, buf.data_ptr(), n, out.data_ptr(), st.data_ptr() if st is not None else 0,
                         max_depth=depth, background=bg, t_min=t_min, base_seed=base_seed, flags=flags,
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[n:] == 0xFF).all(), "the call wrote past its n records"
    return host[:n].copy().view(np.float64).reshape(n, 3)


def bits(a):
    return dm.bits(np.ascontiguousarray(a))


def job(crt, name):
    """The scene's 12-spp camera job, computed once and left unchanged: the camera, its rays and
    states from the device, the fast route's radiance at depth 50 (H, W, 12, 3)."""
    if name not in _JOBS:
        d, s = resident(crt, name)
        cam = camera(crt, d, 12)
        rays, states = device_rays(s, cam)
        rad = run(s, rays, states, 50, tuple(cam.background), cam.t_min)
        for a in (rays, states, rad):
            a.setflags(write=False)
        _JOBS[name] = (cam, rays, states, rad.reshape(H, W, 12, 3))
    return _JOBS[name]


def first_samples(a, k=4):
    """The records of samples [0, k) out of a 12-spp job's (pixel-major) records."""
    return a.reshape((H * W, 12) + a.shape[1:])[:, :k].reshape((H * W * k,) + a.shape[1:])


# ---- 1. camera rays ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtow_final", "cornell"])
def test_camera_rays_equal_the_model(crt, name):
    """rtow_final draws its origins on the defocus disk, cornell has none. The whole frame, the second of
    three tiles of four-row blocks, and samples [4, 12) of a 12-spp job."""
    from cpp_raytracer_amd import Tiling
    d, s = resident(crt, name)
    cam4, cam12 = camera(crt, d, 4), camera(crt, d, 12)
    for cam, kw in ((cam4, {}), (cam4, dict(tiling=Tiling(4, 3, 1, 0))), (cam12, dict(first_sample=4, num_samples=8))):
        rays, states = device_rays(s, cam, **kw)
        mr, ms = rm.camera_rays(crt, cam, **kw)
        assert rays.shape == mr.shape and len(rays) > 0, kw
        assert np.array_equal(bits(rays), bits(mr)), kw
        assert np.array_equal(states, ms), kw


# ---- 2. the render identity -------------------------------------------------------------------------
def render_frame(scene, cam):
    import torch
    out = torch.full((cam.image_h, cam.image_w, 3), math.nan, dtype=torch.float64, device="cuda")
    scene.render_async(0, cam, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", SCENES)
def test_summed_radiance_is_the_render_bit_for_bit(crt, name):
    """spp 4 is one chunk: ((((0 + c0) + c1) + c2) + c3) * (1 / 4.); spp 12 is three: the chunk sums
    U0, U1, U2 as above, then ((U0 + U1) + U2) * (1 / 12.)."""
    d, s = resident(crt, name)
    cam12, _, _, rad = job(crt, name)
    assert crt.sample_chunk_len(4) == 4 == crt.sample_chunk_len(12)
    assert np.array_equal(bits(rm.frame_from_samples(rad, 4)), bits(render_frame(s, cam12))), "12 spp"
    assert np.array_equal(bits(rm.frame_from_samples(rad[:, :, :4], 4)), bits(render_frame(s, camera(crt, d, 4)))), "4 spp"
    assert np.abs(rad).max() > 0


def test_cornell_at_depth_1000(crt):
    d, s = resident(crt, "cornell")
    cam = camera(crt, d, 4, 1000, 16, 8)
    rays, states = device_rays(s, cam)
    rad = run(s, rays, states, 1000, tuple(cam.background), cam.t_min).reshape(8, 16, 4, 3)
    assert np.array_equal(bits(rm.frame_from_samples(rad, 4)), bits(render_frame(s, cam)))
    assert np.array_equal(bits(rad), bits(run(s, rays, states, 1000, tuple(cam.background), cam.t_min, PLAIN).reshape(rad.shape)))


# ---- 3. the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtow_final", "cornell", "mixed", "christmas_tree"])
def test_per_path_radiance_matches_the_oracle(crt, name):
    """tests/test_gpu_parity.py's bar: 1e-12 relative (the paths are the reference's; only the
    association of the throughput products differs). Depth 0 traces nothing and is exactly zero."""
    from cpp_raytracer_amd import camera_with
    d, s = resident(crt, name)
    cam, rays, states, rad50 = job(crt, name)
    rays, states = first_samples(rays), first_samples(states)
    for depth in (0, 1, 2, 50):
        d.camera = camera_with(d.camera, image_w=W, image_h=H, samples_per_pixel=4, max_depth=depth)
        _, want = orc.render(d, SEED, samples=True)
        for route in (0, PLAIN):
            got = run(s, rays, states, depth, tuple(cam.background), cam.t_min, route).reshape(H, W, 4, 3)
            err = np.abs(got - want).max()
            print(f"{name} depth {depth} route {route}: max |gpu - oracle| = {err:.3g}, max |oracle| = {np.abs(want).max():.3g}")
            assert err <= 1e-12 * max(1.0, np.abs(want).max()), (depth, route, err)
            if depth == 0:
                assert (bits(got) == 0).all()
            if depth == 50 and route == 0:
                assert np.array_equal(bits(got), bits(rad50[:, :, :4]))


# ---- 4. routes and switches -------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_plain_route_gives_the_fast_routes_bits(crt, name):
    """rtow_final: LDS scene, sphere-only. cornell / mixed: LDS scene, the general instance (flat-box
    filter / no filter). christmas_tree: HBM scene, LDS treelet and stack, the pair walk. big: u32
    stack entries."""
    _, s = resident(crt, name)
    cam, rays, states, rad = job(crt, name)
    got = run(s, rays, states, 50, tuple(cam.background), cam.t_min, PLAIN)
    assert np.array_equal(bits(got), bits(rad.reshape(-1, 3)))


MINE = [(n, e) for n, e in SWITCHES if n in SCENES]


@pytest.mark.parametrize("name,env", MINE, ids=[n + "-" + "+".join(k[4:] for k in e) for n, e in MINE])
def test_every_switch_gives_the_same_bytes(crt, monkeypatch, name, env):
    """The scene is built and uploaded under the switch (the upload-time switches are read then); both
    routes then give the default run's bytes."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cam, rays, states, rad = job(crt, name)
    rays, states, want = first_samples(rays), first_samples(states), bits(rad[:, :, :4].reshape(-1, 3))
    s = crt.GpuScene(rs.scene_data(crt, name))
    s.upload(0)
    for route in (0, PLAIN):
        assert np.array_equal(bits(run(s, rays, states, 50, tuple(cam.background), cam.t_min, route)), want), route
    assert s.guard(0) == 0
    s.close()


# ---- 5. queue edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree"])
def test_prefixes_and_permutations(crt, name):
    _, s = resident(crt, name)
    cam, rays, states, rad = job(crt, name)
    full = bits(rad.reshape(-1, 3))
    bg = tuple(cam.background)
    for n in (1, 63, 64, 65, 4097):
        assert np.array_equal(bits(run(s, rays, states, 50, bg, cam.t_min, n=n)), full[:n]), n
    perm = np.random.default_rng(9).permutation(len(rays))
    assert np.array_equal(bits(run(s, rays[perm], states[perm], 50, bg, cam.t_min)), full[perm])


@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree", "cornell"])
@pytest.mark.parametrize("blocks", ["1", "3", "37"])
def test_small_grids_give_the_same_bytes(crt, monkeypatch, name, blocks):
    """18,432 paths on 1, 3 and 37 blocks: every lane takes path after path, from batch after batch."""
    _, s = resident(crt, name)
    cam, rays, states, rad = job(crt, name)
    monkeypatch.setenv("CRT_GRID_BLOCKS", blocks)
    assert np.array_equal(bits(run(s, rays, states, 50, tuple(cam.background), cam.t_min)), bits(rad.reshape(-1, 3)))


# ---- 6. the contract --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree", "mixed"])
def test_rays_outside_the_contract_see_the_background(crt, name):
    _, s = resident(crt, name)
    cam, rays, states, rad = job(crt, name)
    base, bs, want = rays[:1500], states[:1500], rad.reshape(-1, 3)[:1500]
    bad = [r for _, r, tm in rs.invalid_rays() if tm == rs.INF]
    rr, ss, valid = [], [], []
    j = 0
    for i in range(len(base)):
        if i % 23 == 5:  # one in every wave or so, each class many times over
            rr.append(bad[j % len(bad)])
            ss.append(np.uint32(j * 2654435761 & 0xFFFFFFFF))
            valid.append(False)
            j += 1
        rr.append(base[i])
        ss.append(bs[i])
        valid.append(True)
    assert j >= 3 * len(bad)
    rr, ss, valid = np.array(rr), np.array(ss, np.uint32), np.array(valid)
    bg = (0.25, 0.5, 3.0)  # not the job's: the neighbours below are compared where no path saw it
    for route in (0, PLAIN):
        got = run(s, rr, ss, 50, tuple(cam.background), cam.t_min, route)
        assert np.array_equal(bits(got[valid]), bits(want)), f"valid neighbours, route {route}"
        got = run(s, rr, ss, 50, bg, cam.t_min, route)
        assert np.array_equal(bits(got[~valid]), bits(np.tile(np.array(bg), (j, 1)))), f"route {route}"
        got = run(s, rr, ss, 0, bg, cam.t_min, route)
        assert (bits(got) == 0).all(), f"depth 0, route {route}"


@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree", "cornell"])
def test_zero_tiny_and_huge_direction_components(crt, name):
    """Primary rays that take the EXACT walk (a zero, 2^-45 or 2^45 direction component; under the
    pair walk, on plain references beside lanes holding tokens): the plain route's bits. The rays are
    the camera's, so they still meet the scene, with one component replaced in five of every seven."""
    _, s = resident(crt, name)
    rays = np.array(job(crt, name)[1][:8192])
    i = np.arange(len(rays))
    for m, v in ((0, 0.0), (1, 2.0 ** -45), (2, 2.0 ** 45), (3, -0.0), (4, -(2.0 ** -45))):
        sel = i % 7 == m
        rays[sel, 3 + (i[sel] // 7) % 3] = v
    fast = run(s, rays, None, 50, (0.7, 0.8, 1.0), 1e-5, base_seed=77)
    assert np.array_equal(bits(fast), bits(run(s, rays, None, 50, (0.7, 0.8, 1.0), 1e-5, PLAIN, base_seed=77)))
    assert len(np.unique(bits(fast), axis=0)) > 20  # paths of many kinds


def test_default_states_are_sample_seeds(crt):
    _, s = resident(crt, "rtow_final")
    cam, rays, _, _ = job(crt, "rtow_final")
    rays = rays[:5000]
    base = 0xDEADBEEF
    explicit = np.array([crt.sample_seed(base, i, 0) for i in range(len(rays))], np.uint32)
    bg = tuple(cam.background)
    for route in (0, PLAIN):
        a = run(s, rays, None, 50, bg, cam.t_min, route, base_seed=base)
        assert np.array_equal(bits(a), bits(run(s, rays, explicit, 50, bg, cam.t_min, route, base_seed=5)))
    assert not np.array_equal(bits(a), bits(run(s, rays, None, 50, bg, cam.t_min, base_seed=base + 1)))


def test_refused_calls_leave_the_output_untouched(crt):
    import torch
    from cpp_raytracer_amd import CrtError
    _, s = resident(crt, "cornell")
    n = 64
    rays = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    out = torch.full((n, 24), 0xFF, dtype=torch.uint8, device="cuda")
    ok = dict(max_depth=5, background=(0.0, 0.0, 0.0))
    cases = [(dict(ok, flags=2), "unknown flags"), (dict(ok, t_min=-1.0), "t_min must be finite, >= 0"),
             (dict(ok, t_min=math.nan), "t_min must be finite, >= 0"), (dict(ok, t_min=2.0 ** 101), "t_min must be finite, >= 0"),
             (dict(ok, background=(0.0, math.inf, 0.0)), "background must be finite"),
             (dict(max_depth=5, background=(math.nan, 0.0, 0.0)), "background must be finite")]
    for kw, word in cases:
        with pytest.raises(CrtError, match=r"\(-1\).*crt_radiance_async: .*" + word):
            s.radiance_async(0, rays.data_ptr(), n, out.data_ptr(), **kw)
    with pytest.raises(CrtError, match=r"\(-1\).*more than 2\^31-1 rays"):
        s.radiance_async(0, rays.data_ptr(), 1 << 31, out.data_ptr(), **ok)
    with pytest.raises(CrtError, match=r"\(-1\).*d_rays is null"):
        s.radiance_async(0, 0, n, out.data_ptr(), **ok)
    with pytest.raises(CrtError, match=r"\(-1\).*d_rgb is null"):
        s.radiance_async(0, rays.data_ptr(), n, 0, **ok)
    fresh = crt.GpuScene(rs.scene_data(crt, "cornell"))
    with pytest.raises(CrtError, match=r"\(-4\).*not uploaded"):
        fresh.radiance_async(0, rays.data_ptr(), n, out.data_ptr(), **ok)
    fresh.close()
    with pytest.raises(CrtError, match="radiance: states must be"):
        s.radiance(rays, states=torch.zeros((n,), dtype=torch.int64, device="cuda"))
    with pytest.raises(CrtError, match="radiance: states must be"):
        s.radiance(rays, states=torch.zeros((n + 1,), dtype=torch.int32, device="cuda"))
    with pytest.raises(CrtError, match="radiance: states must be"):
        s.radiance(rays, states=torch.zeros((n,), dtype=torch.int32))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xFF).all()
    s.radiance_async(0, 0, 0, 0, **ok)  # n == 0: CRT_OK, no work
    assert s.radiance(rays[:0]).shape == (0, 3)


def test_radiance_follows_the_tensors_stream(crt):
    """Rays made by torch ops on a side stream, GpuScene.camera_rays and .radiance on that stream with
    no synchronisation in between, one synchronise at the end."""
    import torch
    _, s = resident(crt, "rtow_final")
    cam, rays, states, rad = job(crt, "rtow_final")
    host = torch.from_numpy(np.array(rays)).pin_memory()
    st = torch.from_numpy(np.array(states).view(np.int32)).pin_memory()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        half = host.to("cuda", non_blocking=True) * 0.5
        filler = torch.ones((2048, 2048), device="cuda")
        for _ in range(4):  # work queued ahead of the rays' last op
            filler = filler @ filler * 1e-4
        got = s.radiance(half + half, st.to("cuda", non_blocking=True), 50, tuple(cam.background), cam.t_min)
        r2, s2 = s.camera_rays(cam)
        again = s.radiance(r2, s2, cam.max_depth, tuple(cam.background), cam.t_min, plain=True)
    side.synchronize()
    assert got.shape == (len(rays), 3) and got.dtype == torch.float64
    assert np.array_equal(bits(got.cpu().numpy()), bits(rad.reshape(-1, 3)))
    assert np.array_equal(bits(again.cpu().numpy()), bits(rad.reshape(-1, 3)))
