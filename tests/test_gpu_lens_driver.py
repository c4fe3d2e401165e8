"""crt_render_lens_passes and LensRender on the GPU. With PINHOLE the blocking driver is
crt_render_progressive, crt_render_adaptive and crt_render_denoised on one device, bit for bit (frames,
block counts, samples rendered); for fisheye and cube-map frames it equals LensRender stepped by hand
and the composition of the asynchronous entries at every preview, a cube map being filtered one face
at a time. Every comparison is of bits, so a lost pass fails."""
import numpy as np
import pytest

import lens_pass_model as lpm
import test_gpu_lens as tgl
from test_gpu_lens import INSIDE_CORNELL, camera, lens_for, same
from test_gpu_radiance import guard_stays_zero, resident  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
PRM = (3, 7, 1.0, 0.05)  # iterations, normal squarings, sigma_l, sigma_p
NAN = float("nan")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- PINHOLE is the reference camera's drivers ---------------------------------------------------
@pytest.fixture(scope="module")
def rtow(crt):
    import torch  # noqa: F401 (before the first blocking driver of the module)
    d, s = resident(crt, "rtow_final")
    return s, camera(crt, d, 40, 24, 32), crt.make_lens("pinhole", batch_pixels=101)


def test_pinhole_plain_passes_are_render_progressive(crt, rtow):
    s, cam, lens = rtow
    want, done = s.render_progressive(cam)
    calls = []
    got, raw, rendered = s.render_lens_passes(cam, lens, callback=lambda *a: calls.append(a[:4]) and False)
    assert raw is None and same(got, want) and np.abs(want).max() > 0
    assert done == 32 and rendered == 32 * 40 * 24
    # a tenth of the job rounded up to a chunk: passes of 4; every block active until the last pass
    assert [c[0] for c in calls] == list(range(4, 33, 4)) and all(c[1] == 32 for c in calls)
    nb = crt.block_count(40, 24)
    assert [c[2] for c in calls] == [nb] * 7 + [0] and all(c[3] == nb for c in calls)
    assert same(got, tgl.render(s, cam, lens))  # and it is the one-shot lens frame


@pytest.mark.parametrize("preview", [False, True])
def test_pinhole_adaptive_is_render_adaptive(crt, rtow, preview):
    s, cam, lens = rtow
    kw = dict(threshold=0.05, min_samples=8, samples_per_pass=8)
    ref_calls, calls = [], []
    want, want_counts, want_rendered = s.render_adaptive(
        cam, callback=lambda done, total, active, nb, f: ref_calls.append((done, active, None if f is None else f.copy())) and False,
        preview=preview, **kw)
    got, raw, rendered, counts = s.render_lens_passes(
        cam, lens, callback=lambda done, total, active, nb, nz, f: calls.append((done, active, None if f is None else f.copy())) and False,
        preview=preview, counts=True, **kw)
    assert same(got, want) and np.array_equal(counts, want_counts) and rendered == want_rendered
    assert len(set(want_counts.reshape(-1).tolist())) > 1, "some blocks stop early, some do not"
    assert [c[:2] for c in calls] == [c[:2] for c in ref_calls] and len(calls) >= 2
    for a, b in zip(calls, ref_calls):
        assert (a[2] is None) == (b[2] is None) == (not preview)
        assert preview is False or same(a[2], b[2])


@pytest.mark.parametrize("adaptive", [False, True])
def test_pinhole_denoised_is_render_denoised(crt, rtow, adaptive):
    s, cam, lens = rtow
    kw = dict(threshold=0.05, min_samples=8, samples_per_pass=8) if adaptive else {}
    prm = crt.denoise_params(*PRM)
    want, want_raw, want_rendered = s.render_denoised(cam, prm, noisy=True, **kw)
    got, raw, rendered = s.render_lens_passes(cam, lens, params=prm, noisy=True, **kw)
    assert same(got, want) and same(raw, want_raw) and rendered == want_rendered
    assert not same(got, raw)  # the filter did something
    # denoise=True: the default parameters, and no unfiltered frame unless asked for
    only, none, _ = s.render_lens_passes(cam, lens, denoise=True, **kw)
    assert none is None and same(only, s.render_denoised(cam, **kw)[0])


# ---- fisheye and cube: the driver, LensRender and the composition --------------------------------
def compose(crt, s, cam, lens, threshold, per_pass, prm):
    """The asynchronous entries by hand: after every pass and update (noisy frame, denoised frame,
    block words, active blocks). A cube map is filtered one face at a time."""
    import torch
    h, w = cam.image_h, cam.image_w
    total, nz, rgb, den = [torch.full((h, w, k), NAN, dtype=torch.float64, device="cuda") for k in (3, 2, 3, 3)]
    var = torch.full((h, w), NAN, dtype=torch.float64, device="cuda")
    nb = crt.block_count(w, h)
    blocks = torch.zeros(nb, dtype=torch.int32, device="cuda")
    feat = torch.full((h * w, 88), 0xFF, dtype=torch.uint8, device="cuda")
    s.lens_features(0, cam, lens, feat.data_ptr(), stream())
    done, active = 0, nb
    faces = 6 if lens.kind == crt.CRT_LENS_CUBE else 1
    while done < cam.samples_per_pixel and active:
        count = min(per_pass, cam.samples_per_pixel - done)
        s.render_lens_pass(0, cam, lens, done, count, total.data_ptr(), nz.data_ptr(), rgb.data_ptr(), blocks.data_ptr(), active, stream())
        done += count
        active = crt.adaptive_update(0, cam, nz.data_ptr(), blocks.data_ptr(), done, threshold, 0, stream())
        crt.pixel_variance(0, cam, nz.data_ptr(), var.data_ptr(), done, blocks.data_ptr(), stream())
        fh = h // faces
        for f in range(faces):
            px = f * fh * w
            crt.denoise(0, w, fh, rgb.data_ptr() + 24 * px, var.data_ptr() + 8 * px, feat.data_ptr() + 88 * px, prm,
                        den.data_ptr() + 24 * px, 0, stream())
        torch.cuda.synchronize()
        yield rgb.cpu().numpy(), den.cpu().numpy(), blocks.cpu().numpy().view(np.uint32), active


@pytest.mark.parametrize("kind", ["fisheye", "cube"])
def test_driver_equals_lensrender_and_the_composition_at_every_preview(crt, kind):
    import torch
    d, s = resident(crt, "cornell")
    w, h = lpm.SCEN_FRAMES["cube"] if kind == "cube" else lpm.SCEN_FRAMES["equirect"]
    cam = camera(crt, d, w, h, lpm.SCEN_SPP)
    lens = lens_for(crt, d, kind, origin=INSIDE_CORNELL)
    thr = lpm.SCEN_THRESHOLD["cube"]
    prm = crt.denoise_params(*PRM)
    previews = []
    got, raw, rendered, counts = s.render_lens_passes(
        cam, lens, threshold=thr, samples_per_pass=lpm.SCEN_PASS, params=prm, noisy=True, counts=True, preview=True,
        callback=lambda done, total, active, nb, nz, f: previews.append((done, active, nz.copy(), f.copy())) and False)
    hand = list(compose(crt, s, cam, lens, thr, lpm.SCEN_PASS, prm))
    r = crt.LensRender(s, cam, lens, threshold=thr)
    steps = []
    while not r.finished:
        frame = r.step(lpm.SCEN_PASS)
        den = r.denoised(prm)
        torch.cuda.synchronize()
        steps.append((r.samples_done, r.active_blocks, frame.cpu().numpy(), den.cpu().numpy()))
    assert len(previews) == len(hand) == len(steps) >= 2
    for (done, active, nz, f), (h_rgb, h_den, h_words, h_active), (l_done, l_active, l_rgb, l_den) in zip(previews, hand, steps):
        assert done == l_done and active == h_active == l_active
        assert same(nz, h_rgb) and same(nz, l_rgb), (kind, done, "unfiltered")
        assert same(f, h_den) and same(f, l_den), (kind, done, "denoised")
    assert same(got, previews[-1][3]) and same(raw, previews[-1][2])
    assert np.array_equal(counts.reshape(-1), hand[-1][2] & np.uint32(lpm.STOPPED - 1))
    assert np.array_equal(counts, r.block_samples()) and rendered == r.samples_rendered
    assert not same(got, raw) and np.abs(raw).max() > 0
    print(kind, "block counts", counts.reshape(-1).tolist())
    # without previews and without the filter: the same unfiltered frame, once, at the end
    calls = []
    plain, none, rendered2, counts2 = s.render_lens_passes(cam, lens, threshold=thr, samples_per_pass=lpm.SCEN_PASS, counts=True,
                                                          callback=lambda *a: calls.append(a[4:]) and False)
    assert none is None and same(plain, raw) and rendered2 == rendered and np.array_equal(counts2, counts)
    assert all(a == (None, None) for a in calls) and len(calls) == len(previews)


def test_cube_is_filtered_one_face_at_a_time(crt):
    """The driver's denoised cube map is six crt_denoise_async calls on the w x w faces; one call over
    the w x 6w frame lets taps cross the seams between unrelated faces and gives another frame."""
    import torch
    d, s = resident(crt, "cornell")
    w, h, spp = 12, 72, 8
    cam = camera(crt, d, w, h, spp)
    lens = lens_for(crt, d, "cube", origin=INSIDE_CORNELL)
    prm = crt.denoise_params(*PRM)
    got, raw, rendered = s.render_lens_passes(cam, lens, params=prm, noisy=True)
    assert rendered == spp * w * h
    r = crt.LensRender(s, cam, lens)
    while not r.finished:
        r.step(4)
    assert r.noise() == r.noise() and r.samples_rendered == rendered
    feat, var = r.features(), torch.full((h, w), NAN, dtype=torch.float64, device="cuda")
    crt.pixel_variance(0, cam, r._noise.data_ptr(), var.data_ptr(), spp, 0, stream())
    faces = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda")
    whole = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda")
    for f in range(6):
        px = f * w * w
        crt.denoise(0, w, w, r.frame().data_ptr() + 24 * px, var.data_ptr() + 8 * px, feat.data_ptr() + 88 * px, prm,
                    faces.data_ptr() + 24 * px, 0, stream())
    crt.denoise(0, w, h, r.frame().data_ptr(), var.data_ptr(), feat.data_ptr(), prm, whole.data_ptr(), 0, stream())
    torch.cuda.synchronize()
    assert same(raw, r.frame().cpu().numpy()) and same(raw, tgl.render(s, cam, lens))
    assert same(got, faces.cpu().numpy()) and same(got, r.denoised(prm).cpu().numpy())
    assert not same(got, whole.cpu().numpy())


def test_a_callback_that_stops_returns_that_passes_mean(crt):
    import torch
    d, s = resident(crt, "cornell")
    w, h = 33, 9
    cam = camera(crt, d, w, h, 40)  # passes of 4
    lens = lens_for(crt, d, "fisheye", origin=INSIDE_CORNELL)
    seen = []
    got, raw, rendered, counts = s.render_lens_passes(cam, lens, counts=True,
                                                      callback=lambda done, *a: seen.append(done) or done >= 8)
    assert seen == [4, 8] and raw is None and rendered == 8 * w * h and (counts == 8).all()
    r = crt.LensRender(s, cam, lens)
    r.step(4)
    r.step(4)
    torch.cuda.synchronize()
    assert same(got, r.frame().cpu().numpy()) and np.abs(got).max() > 0
    with pytest.raises(ZeroDivisionError):  # an exception in the callback stops the render and is raised
        s.render_lens_passes(cam, lens, callback=lambda *a: 1 // 0)


@pytest.mark.parametrize("threshold", [None, lpm.SCEN_THRESHOLD["cube"]])
def test_state_resume_round_trip(crt, threshold):
    import torch
    d, s = resident(crt, "cornell")
    w, h = lpm.SCEN_FRAMES["cube"]
    cam = camera(crt, d, w, h, lpm.SCEN_SPP)
    lens = lens_for(crt, d, "cube", origin=INSIDE_CORNELL)
    a = crt.LensRender(s, cam, lens, threshold=threshold)
    a.step(8)
    a.step(16)
    st = a.state()
    b = crt.LensRender.resume(s, cam, lens, {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in st.items()})
    assert b.samples_done == 24 and b.active_blocks == a.active_blocks
    for r in (a, b):
        while not r.finished:
            r.step(8)
    torch.cuda.synchronize()
    assert same(a.frame().cpu().numpy(), b.frame().cpu().numpy())
    assert np.array_equal(a.block_words(), b.block_words()) and a.samples_rendered == b.samples_rendered
    if threshold is None:
        assert same(b.frame().cpu().numpy(), tgl.render(s, cam, lens))  # the one-shot frame's bits
    else:
        assert len(set(b.block_samples().reshape(-1).tolist())) > 1
    with pytest.raises(crt.CrtError, match="the state's lens is not `lens`"):
        crt.LensRender.resume(s, cam, lens_for(crt, d, "cube"), st)
