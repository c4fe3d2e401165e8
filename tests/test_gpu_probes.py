"""crt_probes_async, crt_probe_rays_async and crt_sh_eval_async on the GPU, held to
tests/probe_model.py bit for bit and to the oracle's ray_color within the per-path bar carried through
the reduction. Scenes: rtow_final (LDS, spheres), cornell (parallelograms, lights) and christmas_tree
(an HBM scene), at depth 50. Probe points are hit points of the scene camera's centre rays (ray_sets'
set A), lifted off the surface along the normal; at most 8 probes a call.

The bake is a composition: generate, trace, reduce. The generator is checked against the model; the
whole against the model's reduction of crt_radiance_async on the generated rays (so a difference is
the reduction's or the batching's); the result against the oracle on the model's own rays.
Outputs are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact afterwards.
Every scene's parity guard count is 0 after every test (test_gpu_radiance's fixture)."""
import math

import numpy as np
import pytest

import probe_model as pm
import ray_sets as rs
import test_gpu_radiance as tgr
from oracle import crt_oracle_py as orc
from test_gpu_radiance import bits, guard_stays_zero, resident  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
SCENES = ["rtow_final", "cornell", "christmas_tree"]
MODES = ["sphere", "hemisphere"]
BG = (0.35, 0.6, 1.25)  # three distinct channels, none of them a scene's own
SEED = 0xC0FFEE
DEPTH = 50
TAIL = 64
SIZES = (1, 63, 64, 65, 130)

_POINTS = {}


def probe_points(crt, name):
    """(points (8, 3), unit normals (8, 3)): eight hits of set A spread over the frame, each moved off
    its surface by 1e-4 of the scene's scale along the normal. Computed once and left unchanged."""
    if name not in _POINTS:
        d, _ = resident(crt, name)
        h = rs.oracle(d, rs.set_a(crt, d))
        h = h[h["prim"] >= 0]
        h = h[np.linspace(0, len(h) - 1, 8).astype(int)]
        p, n = np.array(h["point"], np.float64), np.array(h["normal"], np.float64)
        p = p + (1e-4 * max(1.0, float(np.abs(p).max()))) * n
        for a in (p, n):
            a.setflags(write=False)
        _POINTS[name] = (p, n)
    return _POINTS[name]


def device(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached points are read-only


def generate(scene, P, N, S, mode, seed=SEED):
    """crt_probe_rays_async through GpuScene.probe_rays: (rays (n S, 6), states (n S,) uint32)."""
    import torch
    rays, states = scene.probe_rays(device(P), device(N) if mode == "hemisphere" else None, samples=S, mode=mode,
                                    base_seed=seed)
    torch.cuda.synchronize()
    return rays.cpu().numpy(), states.cpu().numpy().view(np.uint32)


def bake(scene, P, N, S, mode, depth=DEPTH, bg=BG, t_min=1e-5, seed=SEED, batch=0, flags=0):
    """One crt_probes_async call on device 0 and the current stream: (n, K, 3) float64."""
    import torch
    n, K = len(P), 9 if mode == "sphere" else 1
    pts = device(P)
    nrm = device(N) if mode == "hemisphere" else None
    out = torch.full((n * K * 24 + TAIL,), 0xFF, dtype=torch.uint8, device="cuda")
    scene.probes_async(0, pts.data_ptr(), nrm.data_ptr() if nrm is not None else 0, n, out.data_ptr(), samples=S,
                       mode=mode, max_depth=depth, background=bg, t_min=t_min, base_seed=seed, batch_probes=batch,
                       flags=flags, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[n * K * 24:] == 0xFF).all(), "the call wrote past its n x K x 3 values"
    return host[:n * K * 24].copy().view(np.float64).reshape(n, K, 3)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1. the generator -------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 64, 65])
@pytest.mark.parametrize("mode", MODES)
def test_generated_rays_equal_the_model(crt, mode, S):
    _, s = resident(crt, "rtow_final")
    P, N = probe_points(crt, "rtow_final")
    P, N = P[:5], N[:5]
    rays, states = generate(s, P, N, S, mode)
    want_rays, want_states = pm.rays(crt, P, N if mode == "hemisphere" else None, S, SEED)
    assert rays.shape == (5 * S, 6) and same(rays, want_rays)
    assert np.array_equal(states, want_states)
    if mode == "hemisphere":
        assert ((rays[:, 3:].reshape(5, S, 3) * N[:, None, :]).sum(-1) >= 0).all()


# ---- 2. the composition -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_bake_is_the_models_reduction_of_the_radiance_query(crt, name, mode):
    import torch
    _, s = resident(crt, name)
    P, N = probe_points(crt, name)
    P, N = P[:5], N[:5]
    sphere = mode == "sphere"
    want65 = None
    for S in SIZES:
        rays, states = generate(s, P, N, S, mode)
        L = tgr.run(s, rays, states, DEPTH, BG, 1e-5)
        want = pm.reduce(rays[:, 3:], L, S, sphere)
        assert want.shape == (5, 9 if sphere else 1, 3)
        assert np.abs(want[:, 0]).min() > 0  # every probe sees light: the comparison is not of zeros
        assert same(bake(s, P, N, S, mode), want), (name, mode, S, 5)
        assert same(bake(s, P[:1], N[:1], S, mode), want[:1]), (name, mode, S, 1)
        if S == 65:
            want65 = want
    # batches: one probe each, a ragged last batch (2, 2, 1), exactly n, more than n
    for batch in (0, 1, 2, 5, 7):
        assert same(bake(s, P, N, 65, mode, batch=batch), want65), (name, mode, "batch_probes", batch)
    assert same(bake(s, P, N, 65, mode, batch=2, flags=crt.CRT_RADIANCE_PLAIN), want65), (name, mode, "plain")
    # GpuScene.probes on a stream of the caller's
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = s.probes(device(P), device(N) if not sphere else None, samples=65, mode=mode, max_depth=DEPTH,
                       background=BG, base_seed=SEED, batch_probes=2)
        plain = s.probes(device(P), device(N) if not sphere else None, samples=65, mode=mode, max_depth=DEPTH,
                         background=BG, base_seed=SEED, plain=True)
    side.synchronize()
    assert tuple(got.shape) == want65.shape and got.dtype == torch.float64
    assert same(got.cpu().numpy(), want65) and same(plain.cpu().numpy(), want65)


# ---- 3. against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_bake_against_the_oracle(crt, name, mode):
    """The model's reduction of the oracle's ray_color on the model's own rays and states (no GPU value
    takes part in the expectation). Per coefficient the tolerance is
      (W / S) * sum_s |Y_k(d_s)| * 1e-12 * max(1, max |L_oracle|)  +  64 eps |c_oracle|:
    the project's per-path bar of 1e-12 relative carried through the linear reduction, and the
    reduction's own rounding."""
    d, s = resident(crt, name)
    P, N = probe_points(crt, name)
    sphere = mode == "sphere"
    S = 200
    rays, states = pm.rays(crt, P, None if sphere else N, S, SEED)
    L = orc.radiance(d, rays, states, DEPTH, BG, 1e-5)
    want = pm.reduce(rays[:, 3:], L, S, sphere)
    W = pm.W_SPHERE if sphere else pm.W_HEMISPHERE
    absY = np.abs(pm.basis(rays[:, 3:].reshape(8, S, 3))).sum(1) if sphere else np.full((8, 1), float(S))
    tol = (W / S) * absY[:, :, None] * (1e-12 * max(1.0, float(np.abs(L).max()))) + 64 * np.finfo(np.float64).eps * np.abs(want)
    got = bake(s, P, N, S, mode)
    ratio = float((np.abs(got - want) / tol).max())
    print(f"{name} {mode}: S {S}, max |gpu - oracle| = {np.abs(got - want).max():.3g}, max |c| = {np.abs(want).max():.3g}, "
          f"largest error / tolerance = {ratio:.3g}")
    assert (np.abs(got - want) <= tol).all(), (name, mode, ratio)
    assert np.abs(want[:, 0]).min() > 0


# ---- 4. the exact case ------------------------------------------------------------------------------
def sky_point(crt):
    """A point above every object of rtow_final (one unit over the root box) and the normal that
    points away from the scene: every direction N + u has d.y >= 0 and every path misses."""
    d, _ = resident(crt, "rtow_final")
    lo, hi = rs.root_box(crt, d)
    return np.array([[0.5 * (lo[0] + hi[0]), hi[1] + 1.0, 0.5 * (lo[2] + hi[2])]]), np.array([[0.0, 1.0, 0.0]])


@pytest.mark.parametrize("S", [64, 128, 130])
def test_all_paths_miss(crt, S):
    """Every path is 0.0 + 1 * background. With S = 64 and 128 every lane holds bg or 2 bg and the tree
    only doubles, so the sum is S * bg exactly and the result is RN(bg * pi) after the exact scaling
    by pi / S: the 4 ulp bound is asserted there. S = 130 rounds on the way and is held to the model."""
    _, s = resident(crt, "rtow_final")
    P, N = sky_point(crt)
    L = np.tile([0.0 + 1.0 * b for b in BG], (S, 1))
    got = bake(s, P, N, S, "hemisphere")
    rays, states = generate(s, P, N, S, "hemisphere")
    assert same(tgr.run(s, rays, states, DEPTH, BG, 1e-5), L)  # they do all miss
    assert same(got, pm.reduce(None, L, S, False))
    if S != 130:
        want = np.array([math.pi * b for b in BG])
        assert (np.abs(got[0, 0] - want) <= 4 * np.spacing(want)).all(), (got, want)
    zero = bake(s, P, N, S, "sphere", depth=0)
    assert zero.shape == (1, 9, 3) and (bits(zero) == 0).all()  # 27 values of +0


# ---- 5. sh_eval -------------------------------------------------------------------------------------
@pytest.mark.parametrize("irradiance", [False, True])
def test_sh_eval_equals_the_model(crt, irradiance):
    import torch
    rng = np.random.default_rng(17)
    coeff = rng.normal(size=(5, 9, 3))
    index = rng.integers(0, 6, 1000).astype(np.uint32)  # 5 = num_probes: zeros
    index[7], index[8] = 5, 0xFFFFFFFF
    dirs = rng.normal(size=(1000, 3))
    dirs /= np.sqrt((dirs * dirs).sum(1))[:, None]
    got = crt.sh_eval(device(coeff), device(index.view(np.int32)), device(dirs), irradiance=irradiance)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert same(got, pm.sh_eval(coeff, index, dirs, irradiance))
    assert (bits(got[index >= 5]) == 0).all() and (index >= 5).sum() > 100
    assert (got[index < 5] != 0).all()


def test_sh_eval_follows_a_bake_on_the_stream(crt):
    """probes and sh_eval chained on one stream without a synchronisation between them: the evaluation
    reads the coefficients the bake wrote (the model's evaluation of them, bit for bit)."""
    import torch
    _, s = resident(crt, "cornell")
    P, N = probe_points(crt, "cornell")
    c = s.probes(device(P), samples=130, max_depth=DEPTH, background=BG, base_seed=SEED)
    e = crt.sh_eval(c, torch.arange(8, dtype=torch.int32, device="cuda"), device(N), irradiance=True)
    torch.cuda.synchronize()
    assert tuple(e.shape) == (8, 3) and bool(torch.isfinite(e).all())
    assert same(e.cpu().numpy(), pm.sh_eval(c.cpu().numpy(), np.arange(8, dtype=np.uint32), N, True))


# ---- 6. guard rails ---------------------------------------------------------------------------------
def test_no_probes_is_an_empty_result(crt):
    import torch
    _, s = resident(crt, "cornell")
    empty = torch.empty((0, 3), dtype=torch.float64, device="cuda")
    assert tuple(s.probes(empty, samples=16, background=BG).shape) == (0, 9, 3)
    assert tuple(s.probes(empty, empty, samples=16, mode="hemisphere", background=BG).shape) == (0, 1, 3)
    rays, states = s.probe_rays(empty, samples=16)
    assert tuple(rays.shape) == (0, 6) and tuple(states.shape) == (0,)
    assert tuple(crt.sh_eval(torch.empty((0, 9, 3), dtype=torch.float64, device="cuda"),
                             torch.empty((0,), dtype=torch.int32, device="cuda"), empty).shape) == (0, 3)
    with pytest.raises(crt.CrtError, match="normals are required"):
        s.probes(empty, samples=16, mode="hemisphere")
    with pytest.raises(crt.CrtError, match="float64 tensor on a GPU"):
        s.probes(torch.empty((0, 3), dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["rtow_final", "christmas_tree"])
def test_a_nan_point_sees_the_background(crt, name, mode):
    """A probe whose point has a NaN is outside crt_trace_async's contract in every ray: all of them
    miss, the result is the model's for L = background. Its neighbours in the call are untouched."""
    _, s = resident(crt, name)
    P, N = probe_points(crt, name)
    P = P[:3].copy()
    P[1, 0] = math.nan
    S = 65
    got = bake(s, P, N[:3], S, mode)
    dirs = pm.rays(crt, P[1:2], None if mode == "sphere" else N[1:2], S, SEED, first_probe=1)[0][:, 3:]
    L = np.tile([0.0 + 1.0 * b for b in BG], (S, 1))
    assert same(got[1:2], pm.reduce(dirs, L, S, mode == "sphere"))
    clean = bake(s, np.delete(P, 1, 0)[:1], N[:1], S, mode)
    assert same(got[:1], clean)
