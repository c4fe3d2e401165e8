"""The denoiser on the GPU: first-hit features equal the oracle's closest hits of the centre rays,
the per-pixel variance and the filter equal their numpy restatement (tests/denoise_model.py) bit for
bit on every tap route, tilings address features as renders do, the drivers equal the low-level
sequence, and the denoised frame is nearer the converged one than the raw frame. Frames are 50 x 30
(no multiple of the filter's 32 x 8 tile or the 16 x 4 block: edge tiles take part)."""
import ctypes as C
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import crt_oracle_py as orc  # noqa: E402
import denoise_model as dm  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 50, 30
SPP, L = 32, 4
NAN = float("nan")
PRM = (5, 7, 1.0, 0.05)  # iterations, normal squarings, sigma_l, sigma_p


def scene(crt, name, seed=None, **cam):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named(name, seed)
    d.camera = camera_with(d.camera, image_w=cam.pop("image_w", W), image_h=cam.pop("image_h", H), **cam)
    return d


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def gpu_features(s, cam, tiling=None, rows=None):
    """The feature records as a numpy array (rows, w), the buffer pre-filled with 0xff bytes."""
    import torch
    rows = rows or cam.image_h
    buf = torch.full((rows * cam.image_w, 88), 0xFF, dtype=torch.uint8, device="cuda")
    s.render_features(0, cam, buf.data_ptr(), stream(), tiling)
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(s_dtype()).reshape(rows, cam.image_w)


def s_dtype():
    import cpp_raytracer_amd
    return cpp_raytracer_amd.FEATURE_DTYPE


def passes(s, cam, bounds):
    """Plain passes over `bounds`: (sums, noise state, frame) device tensors, NaN-filled first."""
    import torch
    total, nz, out = [torch.full((cam.image_h, cam.image_w, k), NAN, dtype=torch.float64, device="cuda") for k in (3, 2, 3)]
    for a, b in bounds:
        s.render_pass(0, cam, a, b - a, total.data_ptr(), nz.data_ptr(), out.data_ptr(), stream())
    torch.cuda.synchronize()
    return total, nz, out


def gpu_variance(crt, cam, nz, done, blocks=None):
    import torch
    var = torch.full((cam.image_h, cam.image_w), NAN, dtype=torch.float64, device="cuda")
    crt.pixel_variance(0, cam, nz.data_ptr(), var.data_ptr(), done, blocks.data_ptr() if blocks is not None else 0, stream())
    torch.cuda.synchronize()
    return var


def gpu_denoise(crt, rgb, var, feat, prm, want_var=True):
    """crt_denoise_async on device tensors; the outputs are pre-filled with NaN."""
    import torch
    h, w = var.shape
    out = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda")
    vout = torch.full((h, w), NAN, dtype=torch.float64, device="cuda") if want_var else None
    crt.denoise(0, w, h, rgb.data_ptr(), var.data_ptr(), feat.data_ptr(), crt.denoise_params(*prm), out.data_ptr(),
                vout.data_ptr() if want_var else 0, stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), vout.cpu().numpy() if want_var else None


def feat_tensor(feat):
    import torch
    return torch.from_numpy(np.ascontiguousarray(feat).view(np.uint8).reshape(-1, 88).copy()).cuda()


def same_bits(a, b):
    return np.array_equal(dm.bits(a), dm.bits(b))


class Job:
    """A scene at 50 x 30 and 32 spp on the GPU: its frame, noise state, variance and features,
    rendered once and left unchanged."""

    def __init__(self, crt, name, seed, **cam_kw):
        self.d = scene(crt, name, seed, samples_per_pixel=SPP, **cam_kw)
        self.s = crt.GpuScene(self.d)
        self.s.upload(0)
        self.cam = crt.resolve_camera(self.d.camera, 13)
        self.total, self.nz, self.out = passes(self.s, self.cam, [(0, 8), (8, SPP)])
        self.var = gpu_variance(crt, self.cam, self.nz, SPP)
        self.feat = gpu_features(self.s, self.cam)
        self.feat_dev = feat_tensor(self.feat)
        self.feat.setflags(write=False)


@pytest.fixture(scope="module")
def cornell(crt):
    return Job(crt, "cornell", None, max_depth=50)


@pytest.fixture(scope="module")
def rtow(crt):
    return Job(crt, "rtow_final", 42)


@pytest.fixture(params=["cornell", "rtow"])
def job(request):
    return request.getfixturevalue(request.param)


# ---- features ------------------------------------------------------------------------------------
def test_features_equal_the_oracles_hits_of_the_centre_rays(crt, job):
    cam = job.cam
    hits = orc.hits(job.d, dm.centre_rays(cam).reshape(-1, 6), cam.t_min).reshape(H, W)
    want = dm.features_from_hits(hits, job.d.materials, list(cam.background), crt.FEATURE_DTYPE)
    got = job.feat
    hit = want["prim"] >= 0
    kinds = set(job.d.materials["kind"][want["material"][hit]].tolist())
    print(f"{int(hit.sum())} hits, {int((~hit).sum())} misses, material kinds {sorted(kinds)}")
    assert hit.any() and (~hit).any()
    if len(job.d.objects) > 100:  # rtow_final: diffuse, metal and glass spheres, and sky
        assert {crt.CRT_LAMBERTIAN, crt.CRT_METAL, crt.CRT_DIELECTRIC} <= kinds
    for name in ("prim", "material"):
        assert np.array_equal(got[name], want[name]), name
    for name in ("t", "point", "normal", "albedo"):
        assert same_bits(got[name], want[name]), name
    glass = hit & (job.d.materials["kind"][want["material"]] == crt.CRT_DIELECTRIC)
    assert (got["albedo"][glass] == 1.0).all()
    assert (got["albedo"][~hit] == np.array(list(cam.background))).all() and (got["t"][~hit] == 0).all()


def test_features_under_a_tiling(crt, rtow):
    from cpp_raytracer_amd import Tiling
    from cpp_raytracer_amd.tiles import owned_rows
    whole = rtow.feat.view(np.uint8).reshape(H, W * 88)
    rows = owned_rows(H, 4, 3, 1)
    other = [r for r in range(H) if r not in rows]
    plain = gpu_features(rtow.s, rtow.cam, Tiling(4, 3, 1, 0)).view(np.uint8).reshape(H, W * 88)
    assert np.array_equal(plain[rows], whole[rows])
    assert (plain[other] == 0xFF).all()  # rows not owned are left untouched
    packed = gpu_features(rtow.s, rtow.cam, Tiling(4, 3, 1, 1), rows=len(rows)).view(np.uint8).reshape(len(rows), W * 88)
    assert np.array_equal(packed, whole[rows])


# ---- variance ------------------------------------------------------------------------------------
def test_variance_after_plain_passes_equals_the_model(crt, job):
    assert crt.sample_chunk_len(SPP) == L
    nz = job.nz.cpu().numpy()
    want = dm.pixel_variance(nz, SPP, L)
    got = job.var.cpu().numpy()
    assert np.isfinite(got).all() and (got > 0).any()
    assert same_bits(got, want)
    # the frame sum of sqrt(v) is crt_noise_estimate's sum of se, up to the order of the additions
    se, _ = crt.noise_estimate(0, job.nz.data_ptr(), W * H, SPP, SPP, stream())
    mine = float(np.sqrt(got).sum())
    print(f"sum sqrt(v) = {mine!r}, crt_noise_estimate sum_se = {se!r}")
    assert abs(mine - se) <= 1e-12 * abs(se)
    # K = 1 (one chunk) and a count that is no whole number of chunks (22 spp: 5 chunks of 4 and 2 more)
    d = scene(crt, "rtow_final", 42, samples_per_pixel=22)
    cam = crt.resolve_camera(d.camera, 13)
    s = crt.GpuScene(d)
    s.upload(0)
    for done in (4, 22):
        _, nz22, _ = passes(s, cam, [(0, done)])
        assert same_bits(gpu_variance(crt, cam, nz22, done).cpu().numpy(), dm.pixel_variance(nz22.cpu().numpy(), done, 4)), done


def test_variance_of_an_adaptive_render_uses_each_blocks_own_count(crt):
    import torch
    from cpp_raytracer_amd.adaptive import AdaptiveRender
    d = scene(crt, "rtow_final", 42, samples_per_pixel=64)
    cam = crt.resolve_camera(d.camera, 13)
    ar = AdaptiveRender(crt.GpuScene(d), cam, 0.08, 16)
    while not ar.finished:
        ar.step(8)
    torch.cuda.synchronize()
    counts = ar.block_samples()
    print("block samples", counts.tolist())
    assert len(np.unique(counts)) >= 3  # blocks stopped at different counts
    want = dm.pixel_variance(ar._noise.cpu().numpy(), dm.block_counts_to_pixels(ar.block_words(), H, W), 4)
    got = gpu_variance(crt, cam, ar._noise, ar.samples_done, ar._blocks).cpu().numpy()
    assert same_bits(got, want)
    # and the adaptive preview: AdaptiveRender.denoised is the low-level calls on its buffers
    den = ar.denoised(crt.denoise_params(*PRM))
    torch.cuda.synchronize()
    feat = gpu_features(ar.scene, cam)
    want_c, _ = dm.denoise(ar._out.cpu().numpy(), want, feat, *PRM)
    assert same_bits(den.cpu().numpy(), want_c)


# ---- the filter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_filter_equals_the_model(crt, monkeypatch, job, iterations):
    prm = (iterations,) + PRM[1:]
    want_c, want_v = dm.denoise(job.out.cpu().numpy(), job.var.cpu().numpy(), job.feat, *prm)
    got_c, got_v = gpu_denoise(crt, job.out, job.var, job.feat_dev, prm)
    assert np.isfinite(got_c).all() and np.isfinite(got_v).all()
    assert same_bits(got_c, want_c) and same_bits(got_v, want_v)
    assert not same_bits(got_c, job.out.cpu().numpy())  # it filtered
    # every step as gathers: the route changes no bit; and without the variance output
    monkeypatch.setenv("CRT_DENOISE_ROUTE", "gather")
    g_c, g_v = gpu_denoise(crt, job.out, job.var, job.feat_dev, prm)
    assert same_bits(g_c, want_c) and same_bits(g_v, want_v)
    monkeypatch.delenv("CRT_DENOISE_ROUTE")
    only_c, _ = gpu_denoise(crt, job.out, job.var, job.feat_dev, prm, want_var=False)
    assert same_bits(only_c, want_c)


@pytest.mark.parametrize("w,h", [(20, 9), (1, 1), (33, 17)])
def test_filter_on_small_frames(crt, w, h):
    """20 x 9: the step-8 and step-16 taps mostly fall outside; 1 x 1: the centre tap alone;
    33 x 17: one pixel past the 32 x 8 tile both ways."""
    d = scene(crt, "rtow_final", 42, image_w=w, image_h=h, samples_per_pixel=SPP)
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 13)
    _, nz, out = passes(s, cam, [(0, SPP)])
    var = gpu_variance(crt, cam, nz, SPP)
    feat = gpu_features(s, cam)
    want_c, want_v = dm.denoise(out.cpu().numpy(), var.cpu().numpy(), feat, *PRM)
    got_c, got_v = gpu_denoise(crt, out, var, feat_tensor(feat), PRM)
    assert np.isfinite(got_c).all()
    assert same_bits(got_c, want_c) and same_bits(got_v, want_v)


def test_filter_with_an_injected_nan_pixel(crt, cornell):
    rgb = cornell.out.clone()
    rgb[11, 23, 2] = NAN
    var = cornell.var.clone()
    var[20, 5] = float("inf")
    want_c, want_v = dm.denoise(rgb.cpu().numpy(), var.cpu().numpy(), cornell.feat, *PRM)
    got_c, got_v = gpu_denoise(crt, rgb, var, cornell.feat_dev, PRM)
    assert same_bits(got_c, want_c) and same_bits(got_v, want_v)
    bad = ~np.isfinite(got_c).all(-1)
    assert bad[11, 23] and bad.sum() == 1 and np.isinf(got_v[20, 5]) and np.isfinite(got_v).sum() == W * H - 1


# ---- drivers -------------------------------------------------------------------------------------
def test_progressive_render_denoised_is_the_low_level_calls(crt, cornell):
    import torch
    from cpp_raytracer_amd.progressive import ProgressiveRender
    pr = ProgressiveRender(cornell.s, cornell.cam)
    pr.step(8)
    frame = pr.step(8).clone()
    den = pr.denoised(crt.denoise_params(*PRM)).clone()  # mid-run: 16 of 32 samples
    torch.cuda.synchronize()
    _, nz, out = passes(cornell.s, cornell.cam, [(0, 8), (8, 16)])
    assert torch.equal(frame, out)
    var = gpu_variance(crt, cornell.cam, nz, 16)
    want, _ = gpu_denoise(crt, out, var, cornell.feat_dev, PRM)
    assert same_bits(den.cpu().numpy(), want)
    feat_ptr = pr.features().data_ptr()
    pr.step(16)
    den = pr.denoised(crt.denoise_params(*PRM))
    torch.cuda.synchronize()
    assert pr.features().data_ptr() == feat_ptr  # computed once per render object
    want, _ = gpu_denoise(crt, cornell.out, cornell.var, cornell.feat_dev, PRM)
    assert same_bits(den.cpu().numpy(), want)
    with pytest.raises(crt.CrtError, match="noise=False"):
        ProgressiveRender(cornell.s, cornell.cam, noise=False).denoised()


def test_blocking_driver_equals_the_low_level_sequence(crt, job):
    frame, _ = job.s.render_progressive(job.cam)
    den, noisy, rendered = job.s.render_denoised(job.cam, crt.denoise_params(*PRM), noisy=True)
    assert same_bits(noisy, frame) and same_bits(noisy, job.out.cpu().numpy())
    want, _ = gpu_denoise(crt, job.out, job.var, job.feat_dev, PRM)
    assert same_bits(den, want)
    assert rendered == SPP * W * H
    den2, none, _ = job.s.render_denoised(job.cam, crt.denoise_params(*PRM))
    assert none is None and same_bits(den2, den)


def test_blocking_adaptive_driver_equals_the_low_level_sequence(crt):
    import torch
    from cpp_raytracer_amd.adaptive import AdaptiveRender
    d = scene(crt, "rtow_final", 42, samples_per_pixel=64)
    cam = crt.resolve_camera(d.camera, 13)
    s = crt.GpuScene(d)
    frame, counts, total = s.render_adaptive(cam, 0.08, 16, 8)
    den, noisy, rendered = s.render_denoised(cam, crt.denoise_params(*PRM), threshold=0.08, min_samples=16,
                                             samples_per_pass=8, noisy=True)
    assert same_bits(noisy, frame) and rendered == total
    assert len(np.unique(counts)) >= 3
    ar = AdaptiveRender(s, cam, 0.08, 16)
    while not ar.finished:
        ar.step(8)
    want = ar.denoised(crt.denoise_params(*PRM))
    torch.cuda.synchronize()
    assert np.array_equal(ar.block_samples(), counts)
    assert same_bits(den, want.cpu().numpy())


# ---- quality -------------------------------------------------------------------------------------
def test_denoised_is_nearer_the_converged_frame(crt, cornell):
    d = scene(crt, "cornell", None, samples_per_pixel=2048, max_depth=50)
    s = crt.GpuScene(d)
    truth, _ = s.render(crt.resolve_camera(d.camera, 99), 1)
    raw = cornell.out.cpu().numpy()
    den, _ = gpu_denoise(crt, cornell.out, cornell.var, cornell.feat_dev, PRM)
    r_raw, r_den = dm.rmse(raw, truth), dm.rmse(den, truth)
    print(f"cornell 50x30 at 32 spp vs 2048 spp: RMSE raw {r_raw:.5f}, denoised {r_den:.5f}, ratio {r_den / r_raw:.3f}")
    assert r_den < r_raw
