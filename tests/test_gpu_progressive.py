"""Progressive rendering on the GPU: a render cut into passes at chunk boundaries and accumulated
in chunk order makes the additions of the one-shot render, so its final frame is bit-identical to
crt_render_async's on every kernel instance, tiling and band split; previews are the mean of the
samples so far; the noise state matches the oracle's per-sample radiances; checkpoints resume onto
the same bits. Frames are 50 x 30 (no multiple of the 16 x 4 tile: edge tiles take part)."""
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "oracle"))
import crt_oracle_py as orc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4  # tests/test_gpu_vs_oracle.py's bar
W, H = 50, 30


def scene(crt, name, seed=None, **cam):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named(name, seed)
    d.camera = camera_with(d.camera, image_w=cam.pop("image_w", W), image_h=cam.pop("image_h", H), **cam)
    return d


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def one_shot(s, cam, tiling=None, rows=None):
    import torch
    out = torch.full((rows or cam.image_h, cam.image_w, 3), float("nan"), dtype=torch.float64, device="cuda")
    s.render_async(0, cam, out.data_ptr(), stream(), tiling)
    torch.cuda.synchronize()
    return out


def in_passes(s, cam, bounds, tiling=None, rows=None, noise=False):
    """The passes [a, b) of `bounds` through crt_render_pass_async into NaN-filled buffers (the
    first pass must overwrite them). Returns (the preview after each pass, sums, noise state)."""
    import torch
    shape = (rows or cam.image_h, cam.image_w)
    nan = float("nan")
    total = torch.full(shape + (3,), nan, dtype=torch.float64, device="cuda")
    out = torch.full(shape + (3,), nan, dtype=torch.float64, device="cuda")
    nz = torch.full(shape + (2,), nan, dtype=torch.float64, device="cuda") if noise else None
    previews = []
    for a, b in bounds:
        s.render_pass(0, cam, a, b - a, total.data_ptr(), nz.data_ptr() if noise else 0, out.data_ptr(), stream(),
                      tiling)
        previews.append(out.clone())
    torch.cuda.synchronize()
    return previews, total, nz


def splits(spp):
    """Pass boundaries for a job of spp samples (chunk length 4): the issue's three passes, one
    pass, and one pass per chunk."""
    three = [(0, 8), (8, 12), (12, 22)] if spp == 22 else [(0, 4), (4, spp)]
    chunks = [(a, min(a + 4, spp)) for a in range(0, spp, 4)]
    return [three, [(0, spp)], chunks]


# every render_kernel instance: LDS scene five waves sphere-only / flat-quad, LDS scene general
# (four waves), HBM scene with LDS stack, HBM stack, and the linear (always-entered leaf) walk
INSTANCES = [
    ("rtow_final", 42, dict(samples_per_pixel=22), {}, {}),
    ("cornell", None, dict(samples_per_pixel=22, max_depth=50), {}, {}),
    ("rtow_final_lights", None, dict(samples_per_pixel=22), {}, {}),
    ("christmas_tree", None, dict(samples_per_pixel=10), {}, {}),
    ("rtow_final", 42, dict(samples_per_pixel=10), {"CRT_FORCE_GSTACK": "1"}, {}),
    ("cornell", None, dict(samples_per_pixel=22, max_depth=50), {}, dict(linear=True)),
    ("rtow_final", 42, dict(samples_per_pixel=10), {"CRT_FOUR_WAVES": "1"}, {}),
]


@pytest.mark.parametrize("name,seed,cam_kw,env,scene_kw", INSTANCES,
                         ids=["rtow", "cornell", "lights", "tree_hbm", "rtow_gstack", "cornell_linear", "rtow_four_waves"])
def test_final_frame_bit_identical_to_one_shot(crt, monkeypatch, name, seed, cam_kw, env, scene_kw):
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = scene(crt, name, seed, **cam_kw)
    s = crt.GpuScene(d, **scene_kw)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 11)
    spp = cam.samples_per_pixel
    assert crt.sample_chunk_len(spp) == 4
    want = one_shot(s, cam)
    assert torch.isfinite(want).all()
    for bounds in splits(spp):
        previews, _, _ = in_passes(s, cam, bounds)
        assert torch.equal(previews[-1], want), bounds


def test_chunk_length_above_four(crt):
    """spp 1000: L = 6, 166 full chunks and a ragged one of 4 samples."""
    import torch
    d = scene(crt, "rtow_final", 42, image_w=16, image_h=8, samples_per_pixel=1000)
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 12)
    assert crt.sample_chunk_len(1000) == 6
    previews, _, _ = in_passes(s, cam, [(0, 6), (6, 600), (600, 1000)])
    assert torch.equal(previews[-1], one_shot(s, cam))


@pytest.fixture(scope="module")
def rtow22(crt):
    """rtow_final 50 x 30 at 22 spp, base seed 13: the scene, and the oracle's per-sample radiances
    (h, w, 22, 3), computed once and left unchanged."""
    d = scene(crt, "rtow_final", 42, samples_per_pixel=22)
    _, smp = orc.render(d, 13, threads=8, samples=True)
    smp.setflags(write=False)
    return d, smp


def test_previews(crt, rtow22):
    import torch
    from cpp_raytracer_amd import camera_with
    d, smp = rtow22
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 13)
    previews, _, _ = in_passes(s, cam, [(0, 8), (8, 12)])
    # spp 8 has the chunk length of spp 22, and seeds depend on (pixel, sample) only
    cam8 = crt.resolve_camera(camera_with(d.camera, samples_per_pixel=8), 13)
    assert torch.equal(previews[0], one_shot(s, cam8))
    err = np.abs(previews[1].cpu().numpy() - smp[:, :, :12].mean(axis=2)).max()
    print(f"preview after 12 of 22 samples: max |gpu - oracle| = {err:.3g}")
    assert err <= TOL


@pytest.mark.parametrize("mode", ["packed_tiles", "bands"])
def test_tiling_and_bands(crt, monkeypatch, mode):
    import torch
    from cpp_raytracer_amd import Tiling
    from cpp_raytracer_amd.tiles import owned_rows
    bounds = [(0, 8), (8, 12), (12, 22)]
    if mode == "bands":
        # 200 x 134: the first pass's partial sums (2 chunks) take 1.3 MB, so a 1 MB budget bands it
        d = scene(crt, "rtow_final", 42, image_w=200, image_h=134, samples_per_pixel=22, max_depth=20)
        s = crt.GpuScene(d)
        s.upload(0)
        cam = crt.resolve_camera(d.camera, 14)
        want = one_shot(s, cam)
        monkeypatch.setenv("CRT_PARTIAL_MB", "1")
        previews, _, _ = in_passes(s, cam, bounds)
        assert torch.equal(previews[-1], want)
        return
    d = scene(crt, "rtow_final", 42, samples_per_pixel=22)
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 14)
    want = one_shot(s, cam)
    frame = torch.full_like(want, float("nan"))
    for t in range(3):
        rows = owned_rows(H, 4, 3, t)
        previews, _, _ = in_passes(s, cam, bounds, Tiling(4, 3, t, 1), rows=len(rows))
        frame[torch.tensor(rows, device="cuda")] = previews[-1]
    assert torch.equal(frame, want)


@pytest.mark.parametrize("emulate", [None, "3", "16"])
def test_blocking_api(crt, monkeypatch, rtow22, emulate):
    import torch
    d, _ = rtow22
    s = crt.GpuScene(d)
    cam = crt.resolve_camera(d.camera, 13)
    if emulate:
        monkeypatch.setenv("CRT_EMULATE_DEVICES", emulate)
    want, _ = s.render(cam, 1)
    got, done = s.render_progressive(cam)  # no callback
    assert done == 22 and np.array_equal(got, want)
    seen = []
    got, done = s.render_progressive(cam, 8, lambda n, total, noise, frame: seen.append((n, total, noise, frame)))
    assert done == 22 and np.array_equal(got, want)
    assert [x[0] for x in seen] == [8, 16, 22] and all(x[1] == 22 for x in seen)
    assert all(np.isnan(x[2]) and x[3] is None for x in seen)  # neither flag: no noise, no preview
    # samples_per_pass = 0: a tenth of 22 rounded up to one chunk; previews and noise asked for
    seen = []
    got, done = s.render_progressive(cam, 0, lambda n, total, noise, frame: seen.append((n, noise, frame.copy())),
                                     preview=True, noise=True)
    counts = [x[0] for x in seen]
    assert counts == [4, 8, 12, 16, 20, 22] and done == 22
    assert np.array_equal(got, want) and np.array_equal(seen[-1][2], want)
    # one chunk has no variance yet; from two on the figure is a positive number
    assert np.isnan(seen[0][1]) and all(np.isfinite(x[1]) and x[1] > 0 for x in seen[1:])
    # a callback that stops after the second pass: the mean of the 8 samples so far, which is the
    # preview after [0, 8) of the pass API; with and without per-pass previews
    s.upload(0)
    previews, _, _ = in_passes(s, cam, [(0, 8)])
    for preview in (False, True):
        calls = []
        got, done = s.render_progressive(cam, 4, lambda n, *a: calls.append(n) or len(calls) == 2, preview=preview)
        assert done == 2 * 4 and calls == [4, 8]
        assert np.array_equal(got, previews[0].cpu().numpy()), preview


def test_resume(crt, rtow22):
    import torch
    from cpp_raytracer_amd.progressive import ProgressiveRender
    d, _ = rtow22
    s = crt.GpuScene(d)
    cam = crt.resolve_camera(d.camera, 13)
    pr = ProgressiveRender(s, cam)
    pr.step(8)
    pr.step(3)  # rounded up to one chunk
    assert pr.samples_done == 12
    state = pr.state()
    noise12 = pr.noise()
    del pr
    s2 = crt.GpuScene(d)
    pr2 = ProgressiveRender.resume(s2, cam, state)
    assert pr2.samples_done == 12 and pr2.noise() == noise12
    while not pr2.finished:
        frame = pr2.step(8)
    assert pr2.samples_done == 22
    torch.cuda.synchronize()
    s2.upload(0)
    assert torch.equal(frame, one_shot(s2, cam))
    with pytest.raises(crt.CrtError):
        pr2.step(4)


def test_noise_state_and_estimate(crt, rtow22):
    import torch
    d, smp = rtow22
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 13)
    _, _, nz = in_passes(s, cam, [(0, 8), (8, 12), (12, 22)], noise=True)
    nz = nz.cpu().numpy()
    # the oracle's radiances: chunk sums in sample order, y = (r + g) + b, the ragged chunk left out
    K, L = 5, 4
    t = np.zeros((H, W))
    q = np.zeros((H, W))
    for c in range(K):
        S = np.zeros((H, W, 3))
        for i in range(c * L, (c + 1) * L):
            S = S + smp[:, :, i]
        y = (S[..., 0] + S[..., 1]) + S[..., 2]
        t = t + y
        q = q + y * y
    err_t = np.abs(nz[..., 0] / t - 1).max()
    err_q = np.abs(nz[..., 1] / q - 1).max()
    print(f"noise state vs oracle: max relative error t {err_t:.3g}, q {err_q:.3g}")
    np.testing.assert_allclose(nz[..., 0], t, rtol=1e-9, atol=0)
    np.testing.assert_allclose(nz[..., 1], q, rtol=1e-9, atol=0)
    # crt_noise_estimate against its formula on the GPU's own t and q; samples_done = 22 and 20
    # both hold 5 full chunks
    gt, gq = nz[..., 0].reshape(-1), nz[..., 1].reshape(-1)
    m = gt / (K * L)
    se = np.sqrt(np.maximum(0, gq / (L * L) - K * m * m) / (K * (K - 1)))
    dev = torch.from_numpy(nz).cuda()
    a = crt.noise_estimate(0, dev.data_ptr(), H * W, 22, 22)
    b = crt.noise_estimate(0, dev.data_ptr(), H * W, 22, 20)
    print(f"sum se {a[0]!r} (numpy {se.sum()!r}), sum mean {a[1]!r} (numpy {m.sum()!r})")
    np.testing.assert_allclose(a, (se.sum(), m.sum()), rtol=1e-9, atol=0)
    assert a == b and a == crt.noise_estimate(0, dev.data_ptr(), H * W, 22, 22)  # equal bits
    assert all(np.isnan(v) for v in crt.noise_estimate(0, dev.data_ptr(), H * W, 22, 4))  # one chunk


def test_noise_falls_with_samples(crt):
    from cpp_raytracer_amd.progressive import ProgressiveRender
    d = scene(crt, "rtow_final", 42, image_w=16, image_h=8, samples_per_pixel=1000)
    pr = ProgressiveRender(crt.GpuScene(d), crt.resolve_camera(d.camera, 15))
    pr.step(60)
    early = pr.noise()
    pr.step(540)
    assert pr.samples_done == 600
    late = pr.noise()
    print(f"relative noise after 60 samples {early:.4g}, after 600 {late:.4g}")
    assert 0 < late < early


def test_validation(crt, rtow22):
    import torch
    d, _ = rtow22
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 13)
    total = torch.zeros(H, W, 3, dtype=torch.float64, device="cuda")
    for first, count in [(2, 4),    # unaligned start
                         (0, 6),    # unaligned end that is not the job's end
                         (20, 4),   # past the job's end
                         (8, 0)]:   # no samples
        with pytest.raises(crt.CrtError):
            s.render_pass(0, cam, first, count, total.data_ptr(), 0, 0, stream())
    with pytest.raises(crt.CrtError):
        s.render_pass(0, cam, 0, 8, 0)
    previews, _, _ = in_passes(s, cam, [(0, 22)])
    assert torch.equal(previews[-1], one_shot(s, cam))
