"""Lens renders in passes under a lighting on the GPU: crt_render_lens_pass_lit_async, LensRender(lighting=)
and crt_render_lens_passes_lit through the Python front end.

  1. passes     after every pass the running sums, the noise state and the frame equal
                tests/lens_pass_model.py applied to radiance(lighting=) of the device's own rays, bit for
                bit; the last frame is render_lens(lighting=)'s. EQUIRECT 33 x 9 and CUBE 5 x 30; 9 spp
                (chunks 4, 4, 1) and 24; batch_pixels 1, 7 and w h + 3, and the plain route
  2. adaptive   masked passes with crt_adaptive_update under a lighting follow
                lens_pass_model.run_adaptive after every pass (block words, sums, noise, frame), on a
                scenario that tests/test_lighting_passes_model.py shows to mix blocks that stop early,
                late and never
  3. nothing    Lighting() with nothing set gives render_lens_pass's bytes
  4. drivers    render_lens_passes(lighting=) equals LensRender(lighting=) stepped by hand, with denoise
                the hand composition of features, variance and filter at every preview; resume() with
                the same lighting reaches the one-shot bits

Output buffers are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact
afterwards (test_gpu_lens_passes.Buffers). Every scene's parity guard count is 0 after every test."""
import numpy as np
import pytest

import lens_model as lm
import lens_pass_model as lpm
import lighting_cases as cs
import pass_model as pm
import test_gpu_lens as tgl
import test_gpu_lighting as tgli
from test_gpu_lens import INSIDE_CORNELL, camera, lens_for, same, with_batch
from test_gpu_lens_driver import PRM
from test_gpu_lens_passes import Buffers, same_state, stream
from test_gpu_light_nee import resident
from test_gpu_radiance import guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
NAME = "cornell"
FRAMES = {"equirect": (33, 9), "cube": (5, 30)}


def lens_pass(s, cam, lens, buf, first, count, lit, noise=True, rgb=True, hint=0):
    s.render_lens_pass(0, cam, lens, first, count, buf.ptr("sum"), buf.ptr("noise") if noise else 0,
                       buf.ptr("rgb") if rgb else 0, buf.blocks.data_ptr() if buf.blocks is not None else 0, hint, stream(),
                       lighting=lit)


def device_radiance(crt, s, cam, lens, first, count, lit):
    """(h, w, count, 3): radiance(lighting=) of the device's own rays of samples [first, first + count)."""
    rays, states = tgl.device_rays(s, cam, lens, first_sample=first, num_samples=count)
    return tgli.run(crt, s, rays, states, cam.max_depth, lit, bg=tuple(cam.background),
                    t_min=cam.t_min).reshape(cam.image_h, cam.image_w, count, 3)


def render(s, cam, lens, lit):
    import torch
    out = s.render_lens(cam, lens, lighting=lit)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def setup(crt, kind, spp):
    d, s = resident(crt, NAME)
    w, h = FRAMES[kind]
    cam = camera(crt, d, w, h, spp)
    lens = lens_for(crt, d, kind, origin=INSIDE_CORNELL if kind == "cube" else None)
    return s, cam, lens


# ---- 1. every pass against the model, and the one-shot frame ------------------------------------------
@pytest.mark.parametrize("label", cs.FIRST)
@pytest.mark.parametrize("kind", ["equirect", "cube"])
@pytest.mark.parametrize("spp,per_pass", [(9, 4), (24, 8)])
def test_every_lit_pass_equals_the_model(crt, kind, spp, per_pass, label):
    s, cam, lens = setup(crt, kind, spp)
    w, h = FRAMES[kind]
    lit = tgli.lighting(crt, NAME, label)
    L = crt.sample_chunk_len(spp)
    assert L == 4
    buf, st = Buffers(w, h), lpm.fresh_state(w, h)
    unlit_differs = False
    for first, count in lpm.pass_plan(spp, L, per_pass):
        lens_pass(s, cam, lens, buf, first, count, lit)
        rad = device_radiance(crt, s, cam, lens, first, count, lit)
        unlit_differs |= not same(rad, device_radiance(crt, s, cam, lens, first, count, crt.Lighting()))
        lpm.lens_pass(st, rad, first, L)
        assert same_state(buf.state(), st), (kind, spp, first, label)
    assert np.abs(st["rgb"]).max() > 0 and unlit_differs
    want = render(s, cam, lens, lit)
    assert same(buf.get("rgb"), want), (kind, spp, label)
    for batch, plain in ((1, None), (7, None), (w * h + 3, None), (0, True)):
        b2 = Buffers(w, h)
        for first, count in lpm.pass_plan(spp, L, per_pass):
            lens_pass(s, cam, with_batch(lens, batch, plain), b2, first, count, lit, noise=False)
        assert same(b2.get("rgb"), want) and same(b2.get("sum"), st["sum"]), (kind, spp, batch, plain, label)
        assert (b2.raw("noise") == 0xFF).all()  # not given: not written


# ---- 2. masked passes and the update under a lighting -------------------------------------------------
_SCEN = {}


def scenario(crt, kind):
    if kind not in _SCEN:
        s, cam, lens = setup(crt, kind, lpm.SCEN_SPP)
        assert (cam.image_w, cam.image_h) == lpm.SCEN_FRAMES[kind]
        lit = tgli.lighting(crt, NAME, cs.SCEN_LIGHTING)
        rad = device_radiance(crt, s, cam, lens, 0, lpm.SCEN_SPP, lit)
        rad.setflags(write=False)
        _SCEN[kind] = (s, cam, lens, lit, rad)
    return _SCEN[kind]


@pytest.mark.parametrize("kind", ["equirect", "cube"])
def test_lit_masked_passes_and_updates_follow_the_model(crt, kind):
    s, cam, lens, lit, rad = scenario(crt, kind)
    w, h = cam.image_w, cam.image_h
    thr = cs.SCEN_THRESHOLD[kind]
    steps = lpm.run_adaptive(rad, lpm.SCEN_PASS, thr)
    counts, stopped = lpm.check_mix(steps)  # early, late and never
    print(kind, "counts", counts.tolist(), "stopped", stopped.tolist())
    nb = crt.block_count(w, h)
    buf = Buffers(w, h, np.zeros(nb, np.uint32))
    for first, count, want, active in steps:
        lens_pass(s, cam, lens, buf, first, count, lit, hint=nb)
        got_active = crt.adaptive_update(0, cam, buf.ptr("noise"), buf.blocks.data_ptr(), first + count, thr, 0, stream())
        assert got_active == active, (kind, first)
        assert same_state(buf.state(), want), (kind, first)
    final = buf.state()
    for b, (ys, xs) in enumerate(pm.block_slices(w, h)):  # a stopped block holds the plain passes' bits after its own count
        assert same(final["rgb"][ys, xs], lm.frame(rad[:, :, :int(counts[b])], 4)[ys, xs]), b


# ---- 3. nothing set ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["equirect", "cube"])
def test_a_lighting_with_nothing_set_is_the_unlit_pass(crt, kind):
    s, cam, lens = setup(crt, kind, 9)
    w, h = FRAMES[kind]
    nb = crt.block_count(w, h)
    words = np.zeros(nb, np.uint32)
    words[::2] = pm.STOPPED  # a masked pass too
    for masked in (False, True):
        a, b = (Buffers(w, h, words if masked else None) for _ in range(2))
        for first, count in ((0, 4), (4, 5)) if not masked else ((0, 4),):
            lens_pass(s, cam, lens, a, first, count, crt.Lighting())
            lens_pass(s, cam, lens, b, first, count, None)
        assert same_state(a.state(), b.state()), (kind, masked)
        assert np.abs(a.get("sum")).max() > 0


# ---- 4. the drivers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["equirect", "cube"])
def test_driver_equals_lensrender_and_the_composition_under_a_lighting(crt, kind):
    import torch
    s, cam, lens, lit, rad = scenario(crt, kind)
    thr = cs.SCEN_THRESHOLD[kind]
    prm = crt.denoise_params(*PRM)
    previews = []
    got, raw, rendered, counts = s.render_lens_passes(
        cam, lens, threshold=thr, samples_per_pass=lpm.SCEN_PASS, params=prm, noisy=True, counts=True, preview=True,
        callback=lambda done, total, active, nb, nz, f: previews.append((done, active, nz.copy(), f.copy())) and False, lighting=lit)
    r = crt.LensRender(s, cam, lens, threshold=thr, lighting=lit)
    steps = []
    while not r.finished:
        frame = r.step(lpm.SCEN_PASS)
        den = r.denoised(prm)  # the composition: features, variance, a filter a face
        torch.cuda.synchronize()
        steps.append((r.samples_done, r.active_blocks, frame.cpu().numpy(), den.cpu().numpy()))
    assert len(previews) == len(steps) >= 2
    for (done, active, nz, f), (l_done, l_active, l_rgb, l_den) in zip(previews, steps):
        assert done == l_done and active == l_active
        assert same(nz, l_rgb), (kind, done, "unfiltered")
        assert same(f, l_den), (kind, done, "denoised")
    assert same(got, previews[-1][3]) and same(raw, previews[-1][2])
    assert np.array_equal(counts, r.block_samples()) and rendered == r.samples_rendered
    assert not same(got, raw) and np.abs(raw).max() > 0
    want = lpm.run_adaptive(rad, lpm.SCEN_PASS, thr)[-1][2]
    assert same(raw, want["rgb"])  # the driver's frame is the model's of the lit radiance
    # without the filter, and plain passes: the one-shot frame
    plain, none, rendered2 = s.render_lens_passes(cam, lens, lighting=lit)
    assert none is None and rendered2 == lpm.SCEN_SPP * cam.image_w * cam.image_h
    one_shot = s.render_lens(cam, lens, lighting=lit)
    torch.cuda.synchronize()
    assert same(plain, one_shot.cpu().numpy()) and same(plain, lm.frame(rad, 4))
    # the features do not see the lighting: a miss keeps the background as its albedo
    unlit = crt.LensRender(s, cam, lens)
    assert torch.equal(r.features(), unlit.features())


@pytest.mark.parametrize("threshold", [None, cs.SCEN_THRESHOLD["cube"]])
def test_state_resume_round_trip_under_a_lighting(crt, threshold):
    import torch
    s, cam, lens, lit, rad = scenario(crt, "cube")
    a = crt.LensRender(s, cam, lens, threshold=threshold, lighting=lit)
    a.step(8)
    a.step(16)
    st = a.state()
    assert "lighting" not in st  # not stored: the caller passes the same one again
    b = crt.LensRender.resume(s, cam, lens, {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in st.items()},
                              lighting=lit)
    assert b.samples_done == 24 and b.active_blocks == a.active_blocks
    for r in (a, b):
        while not r.finished:
            r.step(8)
    torch.cuda.synchronize()
    assert same(a.frame().cpu().numpy(), b.frame().cpu().numpy())
    assert np.array_equal(a.block_words(), b.block_words()) and a.samples_rendered == b.samples_rendered
    if threshold is None:
        assert same(b.frame().cpu().numpy(), render(s, cam, lens, lit))  # the one-shot frame's bits
        dark = crt.LensRender.resume(s, cam, lens, st)  # resumed without the lighting: another render
        while not dark.finished:
            dark.step(8)
        torch.cuda.synchronize()
        assert not same(dark.frame().cpu().numpy(), b.frame().cpu().numpy())
    else:
        assert len(set(b.block_samples().reshape(-1).tolist())) > 1
