"""Denoised renders over several devices (crt_render_denoised_devices): rows dealt in 4-row blocks
over emulated (CRT_EMULATE_DEVICES) or real devices, variance and filter records packed per device,
gathered to device 0 and filtered there. The unfiltered frame has the bits of render_progressive /
render_adaptive, the denoised frame those of the one-device render_denoised, for every device
count; denoised previews equal AdaptiveRender stepped and denoised. Frames are 50 x 30 (8 row
blocks, the last of 2 rows; no multiple of the filter's 32 x 8 tile or the 16 x 4 block)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H = 50, 30
PRM = (5, 7, 1.0, 0.05)  # iterations, normal squarings, sigma_l, sigma_p
ADAPTIVE = dict(threshold=0.08, min_samples=16, samples_per_pass=8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def job(crt, name, seed, **cam):
    import torch  # noqa: F401  (first: the library then runs on the HIP runtime PyTorch brings along)
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named(name, seed)
    d.camera = camera_with(d.camera, image_w=cam.pop("image_w", W), image_h=cam.pop("image_h", H), **cam)
    return crt.GpuScene(d), crt.resolve_camera(d.camera, 13)


class Plain:
    """cornell 50 x 30 at 32 spp on one device: render_progressive's frame and render_denoised's."""

    def __init__(self, crt):
        self.s, self.cam = job(crt, "cornell", None, samples_per_pixel=32, max_depth=50)
        self.prm = crt.denoise_params(*PRM)
        self.frame, _ = self.s.render_progressive(self.cam)
        self.den, _, self.rendered = self.s.render_denoised(self.cam, self.prm)
        for a in (self.frame, self.den):
            a.setflags(write=False)


class Adaptive:
    """rtow_final 50 x 30, a 64-spp job at threshold 0.08 on one device: render_adaptive's frame and
    counts, render_denoised's frame, and AdaptiveRender's frames step by step."""

    def __init__(self, crt):
        import torch
        from cpp_raytracer_amd.adaptive import AdaptiveRender
        self.s, self.cam = job(crt, "rtow_final", 42, samples_per_pixel=64)
        self.prm = crt.denoise_params(*PRM)
        self.frame, self.counts, self.total = self.s.render_adaptive(self.cam, 0.08, 16, 8)
        self.den, _, _ = self.s.render_denoised(self.cam, self.prm, **ADAPTIVE)
        ar = AdaptiveRender(self.s, self.cam, 0.08, 16)
        self.steps = []  # (samples done, active blocks, unfiltered frame, denoised frame)
        while not ar.finished:
            raw = ar.step(8)
            den = ar.denoised(self.prm)
            torch.cuda.synchronize()
            self.steps.append((ar.samples_done, ar.active_blocks, raw.cpu().numpy().copy(), den.cpu().numpy().copy()))
        for a in (self.frame, self.counts, self.den):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def plain(crt):
    return Plain(crt)


@pytest.fixture(scope="module")
def adaptive(crt):
    return Adaptive(crt)


def check_plain(p, **kw):
    calls = []
    den, noisy, rendered, counts = p.s.render_denoised(p.cam, p.prm, noisy=True, counts=True,
                                                       callback=lambda *a: calls.append(a), **kw)
    assert same_bits(noisy, p.frame)
    assert same_bits(den, p.den)
    assert not same_bits(den, noisy)  # it filtered
    assert rendered == 32 * W * H == p.rendered
    assert counts.shape == (8, 4) and (counts == 32).all()
    assert calls == [(32, 32, 0, 32, None, None)]  # one plain pass: called once, no previews


def check_adaptive(a, **kw):
    den, noisy, rendered, counts = a.s.render_denoised(a.cam, a.prm, noisy=True, counts=True, **ADAPTIVE, **kw)
    assert len(np.unique(a.counts)) >= 3  # blocks stopped at different counts
    assert same_bits(noisy, a.frame)
    assert np.array_equal(counts, a.counts) and rendered == a.total
    assert same_bits(den, a.den)


@pytest.mark.parametrize("n", [2, 3, 8, 16])
def test_plain_render_on_emulated_devices(monkeypatch, plain, n):
    """3: the short last block falls on a lane that also has full blocks; 8: it is a lane's only
    block; 16: eight lanes own nothing. Five iterations reach 62 pixels: every lane's taps cross
    into every other lane's rows."""
    monkeypatch.setenv("CRT_EMULATE_DEVICES", str(n))
    check_plain(plain, num_devices=n)


@pytest.mark.parametrize("n", [3, 16])
def test_adaptive_render_on_emulated_devices(monkeypatch, adaptive, n):
    monkeypatch.setenv("CRT_EMULATE_DEVICES", str(n))
    check_adaptive(adaptive, num_devices=n)
    # without the unfiltered frame or the counts: the same denoised frame
    den, none, rendered = adaptive.s.render_denoised(adaptive.cam, adaptive.prm, **ADAPTIVE, num_devices=n)
    assert none is None and rendered == adaptive.total and same_bits(den, adaptive.den)


def test_previews_equal_adaptive_render_stepped_and_denoised(monkeypatch, adaptive):
    monkeypatch.setenv("CRT_EMULATE_DEVICES", "3")
    seen = []

    def keep(done, total, active, blocks, noisy, den):
        seen.append((done, total, active, blocks, noisy.copy(), den.copy()))

    den, noisy, rendered, counts = adaptive.s.render_denoised(adaptive.cam, adaptive.prm, noisy=True, counts=True,
                                                              callback=keep, preview=True, num_devices=3, **ADAPTIVE)
    assert len(seen) == len(adaptive.steps) >= 3
    for k, (got, want) in enumerate(zip(seen, adaptive.steps)):
        assert got[:4] == (want[0], 64, want[1], 8 * 4), k
        assert same_bits(got[4], want[2]), k
        assert same_bits(got[5], want[3]), k
    assert same_bits(den, seen[-1][5]) and same_bits(noisy, seen[-1][4])  # the last preview is the result
    assert same_bits(den, adaptive.den) and same_bits(noisy, adaptive.frame)
    assert np.array_equal(counts, adaptive.counts) and rendered == adaptive.total
    # preview without the unfiltered frame: the callback gets None for it
    got = []
    den2, none, _ = adaptive.s.render_denoised(adaptive.cam, adaptive.prm, preview=True, num_devices=3, **ADAPTIVE,
                                               callback=lambda d, t, a, b, noisy, den: got.append((noisy, den.copy())))
    assert none is None and len(got) == len(seen) and all(g[0] is None for g in got)
    assert all(same_bits(g[1], s[5]) for g, s in zip(got, seen)) and same_bits(den2, adaptive.den)


def test_callback_stops_the_render_after_the_second_step(monkeypatch, adaptive):
    monkeypatch.setenv("CRT_EMULATE_DEVICES", "3")
    seen = []

    def stop_at_two(done, total, active, blocks, noisy, den):
        seen.append(done)
        return len(seen) == 2

    den, noisy, rendered, counts = adaptive.s.render_denoised(adaptive.cam, adaptive.prm, noisy=True, counts=True,
                                                              callback=stop_at_two, preview=True, num_devices=3,
                                                              **ADAPTIVE)
    done, _, raw2, den2 = adaptive.steps[1]
    assert seen == [8, 16] and done == 16
    assert same_bits(noisy, raw2) and same_bits(den, den2)
    assert (counts == 16).all() and rendered == 16 * W * H
    # stopped without previews: the frames are written once, when the render ends, and are the same
    seen.clear()
    args = []

    def stop_blind(done, total, active, blocks, noisy, den):
        args.append((noisy, den))
        return stop_at_two(done, total, active, blocks, noisy, den)

    den_b, noisy_b, rendered_b = adaptive.s.render_denoised(adaptive.cam, adaptive.prm, noisy=True, callback=stop_blind,
                                                            num_devices=3, **ADAPTIVE)
    assert args == [(None, None)] * 2 and rendered_b == rendered
    assert same_bits(noisy_b, raw2) and same_bits(den_b, den2)


def test_an_exception_in_the_callback_stops_the_render_and_is_raised(monkeypatch, adaptive):
    monkeypatch.setenv("CRT_EMULATE_DEVICES", "3")
    seen = []

    def boom(done, *rest):
        seen.append(done)
        raise KeyError("stop")

    with pytest.raises(KeyError):
        adaptive.s.render_denoised(adaptive.cam, adaptive.prm, callback=boom, num_devices=3, **ADAPTIVE)
    assert seen == [8]


@pytest.mark.parametrize("w,h", [(33, 17), (1, 1)])
def test_tiny_frames(crt, monkeypatch, w, h):
    """33 x 17: one pixel past the filter's 32 x 8 tile both ways, a last row block of one row;
    1 x 1: two of the three lanes own nothing."""
    s, cam = job(crt, "rtow_final", 42, image_w=w, image_h=h, samples_per_pixel=32)
    prm = crt.denoise_params(*PRM)
    want, want_raw, want_n = s.render_denoised(cam, prm, noisy=True)
    want_a, want_a_raw, want_a_n = s.render_denoised(cam, prm, noisy=True, **ADAPTIVE)
    monkeypatch.setenv("CRT_EMULATE_DEVICES", "3")
    den, raw, n = s.render_denoised(cam, prm, noisy=True, num_devices=3)
    assert same_bits(den, want) and same_bits(raw, want_raw) and n == want_n == 32 * w * h
    den, raw, n = s.render_denoised(cam, prm, noisy=True, num_devices=3, **ADAPTIVE)
    assert same_bits(den, want_a) and same_bits(raw, want_a_raw) and n == want_a_n


def test_gather_route_gives_the_default_routes_bits(monkeypatch, plain):
    monkeypatch.setenv("CRT_EMULATE_DEVICES", "3")
    monkeypatch.setenv("CRT_DENOISE_ROUTE", "gather")
    check_plain(plain, num_devices=3)


def test_on_real_devices(crt, monkeypatch, plain, adaptive):
    count = crt.device_count()
    if count < 2:
        pytest.skip(f"{count} device visible: the unemulated multi-device run needs at least 2")
    monkeypatch.delenv("CRT_EMULATE_DEVICES", raising=False)
    n = min(count, 4)
    check_plain(plain, num_devices=n)
    check_adaptive(adaptive, num_devices=n)
