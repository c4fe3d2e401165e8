"""crt_render_lens_pass_async on the GPU, for every lens kind: after every pass the running sums, the
noise state and the frame equal tests/lens_pass_model.py applied to the radiance query on the device's
own rays, bit for bit; the last frame is crt_render_lens_async's; PINHOLE passes are
crt_render_pass_async's and crt_render_pass_masked_async's; masked passes with crt_adaptive_update
follow the model on a scenario that mixes stopped and active blocks.
Output buffers are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact
afterwards. Every scene's parity guard count is 0 after every test."""
import math

import numpy as np
import pytest

import lens_model as lm
import lens_pass_model as lpm
import pass_model as pm
import ray_sets as rs
import test_gpu_lens as tgl
import test_gpu_radiance as tgr
from test_gpu_lens import BG, DEPTH, INSIDE_CORNELL, KINDS, camera, lens_for, same, with_batch
from test_gpu_radiance import bits, guard_stays_zero, resident  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
TAIL = 64
STOPPED = pm.STOPPED


class Buffers:
    """d_sum, d_noise, d_rgb (and block words) of a w x h frame as 0xFF-filled byte tensors with a
    sentinel tail each."""

    def __init__(self, w, h, words=None):
        import torch
        self.w, self.h = w, h
        self.n = {"sum": w * h * 24, "noise": w * h * 16, "rgb": w * h * 24}
        self.t = {k: torch.full((n + TAIL,), 0xFF, dtype=torch.uint8, device="cuda") for k, n in self.n.items()}
        self.blocks = None
        if words is not None:
            self.nb = len(words)
            self.blocks = torch.full((self.nb + TAIL,), -1, dtype=torch.int32, device="cuda")
            self.blocks[:self.nb] = torch.from_numpy(np.array(words, np.uint32).view(np.int32))

    def ptr(self, k):
        return self.t[k].data_ptr()

    def get(self, k):
        import torch
        torch.cuda.synchronize()
        host = self.t[k].cpu().numpy()
        n = self.n[k]
        assert (host[n:] == 0xFF).all(), f"the call wrote past {k}"
        return host[:n].copy().view(np.float64).reshape(self.h, self.w, -1)

    def raw(self, k):
        import torch
        torch.cuda.synchronize()
        return self.t[k].cpu().numpy()

    def words(self):
        import torch
        torch.cuda.synchronize()
        host = self.blocks.cpu().numpy()
        assert (host[self.nb:] == -1).all(), "the call wrote past the block words"
        return host[:self.nb].copy().view(np.uint32)

    def state(self):
        st = {k: self.get(k) for k in ("sum", "noise", "rgb")}
        if self.blocks is not None:
            st["words"] = self.words()
        return st


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def lens_pass(s, cam, lens, buf, first, count, noise=True, rgb=True, hint=0):
    s.render_lens_pass(0, cam, lens, first, count, buf.ptr("sum"), buf.ptr("noise") if noise else 0,
                       buf.ptr("rgb") if rgb else 0, buf.blocks.data_ptr() if buf.blocks is not None else 0, hint, stream())


def device_radiance(s, cam, lens, first, count):
    """(h, w, count, 3): the radiance query on the device's own rays of samples [first, first + count)."""
    rays, states = tgl.device_rays(s, cam, lens, first_sample=first, num_samples=count)
    return tgr.run(s, rays, states, cam.max_depth, BG, cam.t_min).reshape(cam.image_h, cam.image_w, count, 3)


def same_state(got, want, keys=("sum", "noise", "rgb")):
    return all(same(got[k], want[k]) for k in keys) and ("words" not in want or np.array_equal(got["words"], want["words"]))


# ---- 1, 2. every kind against the model, and the one-shot frame ---------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["rtow_final", "cornell"])
@pytest.mark.parametrize("spp,per_pass", [(9, 4), (24, 8), (136, 64), (136, 68), (769, 385)])
def test_every_pass_equals_the_model(crt, name, kind, spp, per_pass):
    """spp 9: chunks 4, 4, 1 in passes of one chunk; 24: six chunks in passes of two; 136: passes of 64
    samples, the most one thread a pixel accumulates, and of 68, the fewest one wave a pixel does; 769:
    L = 5, 154 chunks, a pass of 77 (every lane of the accumulate holds one or two chunks) and one of
    76 and the ragged chunk of 4 samples."""
    d, s = resident(crt, name)
    w, h = (3, 18) if kind == "cube" else (7, 5)
    cam = camera(crt, d, w, h, spp)
    L = crt.sample_chunk_len(spp)
    assert L == (5 if spp == 769 else 4)
    lens = lens_for(crt, d, kind)
    buf, st = Buffers(w, h), lpm.fresh_state(w, h)
    for first, count in lpm.pass_plan(spp, L, per_pass):
        lens_pass(s, cam, lens, buf, first, count)
        lpm.lens_pass(st, device_radiance(s, cam, lens, first, count), first, L)
        assert same_state(buf.state(), st), (name, kind, spp, first)
    assert np.abs(st["rgb"]).max() > 0  # the comparison is not of zeros
    want = tgl.render(s, cam, lens)
    assert same(buf.get("rgb"), want), (name, kind, spp)
    if spp > 24:
        return
    # the same passes for other batch sizes and the plain route, without the noise state
    for batch, plain in ((1, None), (7, None), (w * h + 3, None), (0, True)):
        b2 = Buffers(w, h)
        for first, count in lpm.pass_plan(spp, L, per_pass):
            lens_pass(s, cam, with_batch(lens, batch, plain), b2, first, count, noise=False)
        assert same(b2.get("rgb"), want) and same(b2.get("sum"), st["sum"]), (name, kind, spp, batch, plain)
        assert (b2.raw("noise") == 0xFF).all()  # not given: not written


# ---- 3, 4. PINHOLE is the reference camera's pass -----------------------------------------------
@pytest.mark.parametrize("name,spp,bounds", [("rtow_final", 24, [(0, 8), (8, 12), (12, 24)]), ("cornell", 9, [(0, 8), (8, 9)])])
def test_pinhole_is_render_pass(crt, name, spp, bounds):
    import torch
    d, s = resident(crt, name)
    w, h = 20, 12
    cam = camera(crt, d, w, h, spp)
    lens = crt.make_lens("pinhole", batch_pixels=11)
    buf = Buffers(w, h)
    ref = [torch.full((h, w, k), math.nan, dtype=torch.float64, device="cuda") for k in (3, 2, 3)]
    for a, b in bounds:
        lens_pass(s, cam, lens, buf, a, b - a)
        s.render_pass(0, cam, a, b - a, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), stream())
        torch.cuda.synchronize()
        got = buf.state()
        for k, r in zip(("sum", "noise", "rgb"), ref):
            assert same(got[k], r.cpu().numpy()), (name, k, a)
    assert np.abs(got["rgb"]).max() > 0


def masked_pair(crt, s, cam, first, count, words):
    """The lens pass and the reference camera's masked pass from the same state: plain passes up to
    `first`, then one masked pass with the block words `words`. Returns (lens state, reference state)."""
    import torch
    w, h = cam.image_w, cam.image_h
    lens = crt.make_lens("pinhole")
    buf = Buffers(w, h, words)
    ref = [torch.full((h, w, k), math.nan, dtype=torch.float64, device="cuda") for k in (3, 2, 3)]
    ref_words = torch.from_numpy(words.view(np.int32).copy()).cuda()
    if first:
        s.render_pass(0, cam, 0, first, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), stream())
        before = Buffers(w, h)
        lens_pass(s, cam, lens, before, 0, first)
        for k in ("sum", "noise", "rgb"):
            buf.t[k].copy_(before.t[k])
    lens_pass(s, cam, lens, buf, first, count, hint=3)
    s.render_pass_masked(0, cam, first, count, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref_words.data_ptr(), 0,
                         stream())
    torch.cuda.synchronize()
    want = {k: r.cpu().numpy() for k, r in zip(("sum", "noise", "rgb"), ref)}
    want["words"] = ref_words.cpu().numpy().view(np.uint32)
    return buf.state(), want


@pytest.mark.parametrize("w,h", [(33, 9), (80, 30)])
@pytest.mark.parametrize("first", [0, 8])
def test_pinhole_masked_is_render_pass_masked(crt, first, w, h):
    """Some blocks pre-set stopped, some at another count: the skipped-block writes (zeroes in a pass
    from sample 0; the frame from the block's own count later) and the words equal the reference
    camera's masked pass. 33 x 9: 9 blocks, one segment of the pixel list; 80 x 30: 40 blocks, 2400
    pixels in three segments, the last one ragged."""
    d, s = resident(crt, "rtow_final")
    cam = camera(crt, d, w, h, 24)
    nb = crt.block_count(w, h)
    words = np.full(nb, first, np.uint32)
    words[1::7] = STOPPED | (first // 2)       # stopped earlier (with 0 or 4 samples)
    words[3::7] = first + 4                     # at another count
    words[5::7] = STOPPED                       # stopped with no samples: its frame is 0
    got, want = masked_pair(crt, s, cam, first, 8, words)
    assert same_state(got, want), (first, w, h)
    active = int((words == first).sum())
    assert 0 < active < nb and got["words"].tolist().count(first + 8) == active and np.abs(got["rgb"]).max() > 0
    if first == 0:
        ys, xs = pm.block_slices(w, h)[5]
        assert all((bits(got[k][ys, xs]) == 0).all() for k in ("sum", "noise", "rgb"))


def test_a_pixel_list_of_more_than_1024_segments(crt):
    """1100 x 1000: 1075 segments of 1024 pixels, so the prefix sum over the segments takes a second
    round; a fault here shows at no smaller size. One chunk a pixel, a third of the blocks stopped."""
    d, s = resident(crt, "rtow_final")
    w, h = 1100, 1000
    cam = camera(crt, d, w, h, 4)
    nb = crt.block_count(w, h)
    words = np.zeros(nb, np.uint32)
    words[np.arange(nb) % 3 == 1] = STOPPED
    got, want = masked_pair(crt, s, cam, 0, 4, words)
    assert same_state(got, want)
    assert (got["words"][words == 0] == 4).all() and np.abs(got["rgb"]).max() > 0


# ---- 5, 6. masked passes and the update on the scenario -----------------------------------------
_SCEN = {}


def scenario(crt, kind):
    """The scenario's camera, lens and the radiance of all 64 samples on the device's own rays, once."""
    if kind not in _SCEN:
        d, s = resident(crt, "cornell")
        w, h = lpm.SCEN_FRAMES[kind]
        cam = camera(crt, d, w, h, lpm.SCEN_SPP)
        lens = lens_for(crt, d, kind, origin=INSIDE_CORNELL if lpm.SCEN_INSIDE[kind] else None)
        rad = device_radiance(s, cam, lens, 0, lpm.SCEN_SPP)
        rad.setflags(write=False)
        _SCEN[kind] = (s, cam, lens, rad)
    return _SCEN[kind]


@pytest.mark.parametrize("kind", ["equirect", "cube"])
def test_masked_passes_and_updates_follow_the_model(crt, kind):
    s, cam, lens, rad = scenario(crt, kind)
    w, h = cam.image_w, cam.image_h
    thr = lpm.SCEN_THRESHOLD[kind]
    steps = lpm.run_adaptive(rad, lpm.SCEN_PASS, thr)
    counts, stopped = lpm.check_mix(steps)  # neither everything nor nothing stops
    print(kind, "counts", counts.tolist(), "stopped", stopped.tolist())
    nb = crt.block_count(w, h)
    runs = {}
    for hint in (0, 1, nb):
        buf = Buffers(w, h, np.zeros(nb, np.uint32))
        for first, count, want, active in steps:
            lens_pass(s, cam, lens, buf, first, count, hint=hint)
            got_active = crt.adaptive_update(0, cam, buf.ptr("noise"), buf.blocks.data_ptr(), first + count, thr, 0, stream())
            assert got_active == active, (kind, hint, first)
            assert same_state(buf.state(), want), (kind, hint, first)
        runs[hint] = buf.state()
    assert same_state(runs[1], runs[0]) and same_state(runs[nb], runs[0])
    # a stopped block holds the plain passes' bits after its own count
    for b, (ys, xs) in enumerate(pm.block_slices(w, h)):
        assert same(runs[0]["rgb"][ys, xs], lm.frame(rad[:, :, :int(counts[b])], 4)[ys, xs]), b


@pytest.mark.parametrize("kind,done", [("equirect", 16), ("cube", 64)])
def test_noise_estimate_on_the_lens_noise_state(crt, kind, done):
    s, cam, lens, rad = scenario(crt, kind)
    w, h = cam.image_w, cam.image_h
    buf = Buffers(w, h)
    lens_pass(s, cam, lens, buf, 0, 8)
    lens_pass(s, cam, lens, buf, 8, done - 8)
    got = crt.noise_estimate(0, buf.ptr("noise"), w * h, lpm.SCEN_SPP, done, stream())
    noise = buf.get("noise")
    assert same(noise, lpm.direct_noise(rad[:, :, :done], 4))
    want = pm.noise_tree(noise.reshape(-1, 2), done // 4, 4)
    assert same(np.array(got), np.array(want)) and want[1] > 0, (got, want)


# ---- 7. edges -----------------------------------------------------------------------------------
def test_a_pass_with_every_block_stopped_writes_the_frame_only(crt):
    """No block is at the pass's first sample: nothing is traced (the guard, which every radiance query
    counts into, is what it was; the sums, the noise state and the words keep their bytes) and the frame
    is every block's sum times 1 / its own count."""
    s, cam, lens, rad = scenario(crt, "cube")
    w, h = cam.image_w, cam.image_h
    nb = crt.block_count(w, h)
    words = np.array([STOPPED | 8] * (nb - 2) + [STOPPED, 24], np.uint32)
    buf = Buffers(w, h, words)
    rng = np.random.default_rng(3)
    total = rng.random((h, w, 3))
    import torch
    buf.t["sum"][:w * h * 24] = torch.from_numpy(total.view(np.uint8).reshape(-1)).cuda()
    before = {k: buf.raw(k).copy() for k in ("sum", "noise")}
    lens_pass(s, cam, lens, buf, 8, 8)
    assert all((buf.raw(k) == before[k]).all() for k in before)
    assert np.array_equal(buf.words(), words)
    want = np.zeros((h, w, 3))
    for b, (ys, xs) in enumerate(pm.block_slices(w, h)):
        n = int(words[b]) & (STOPPED - 1)
        want[ys, xs] = total[ys, xs] * (1 / float(n)) if n else 0.0
    assert same(buf.get("rgb"), want)


@pytest.mark.parametrize("kind", ["pinhole", "fisheye", "cube"])
@pytest.mark.parametrize("masked", [False, True])
def test_depth_zero_adds_plus_zero(crt, kind, masked):
    d, s = resident(crt, "cornell")
    w, h = tgl.dims(kind, 5, 3)
    cam = camera(crt, d, w, h, 9, depth=0)
    lens = lens_for(crt, d, kind)
    nb = crt.block_count(w, h)
    buf = Buffers(w, h, np.zeros(nb, np.uint32) if masked else None)
    for first, count in ((0, 4), (4, 5)):
        lens_pass(s, cam, lens, buf, first, count)
    got = buf.state()
    assert all((bits(got[k]) == 0).all() for k in ("sum", "noise", "rgb"))
    if masked:
        assert (got["words"] == 9).all()


@pytest.mark.parametrize("kind", KINDS[1:])
def test_a_nan_origin_gives_background_sums(crt, kind):
    """Every path is 0.0 + 1 * background: a chunk of 4 is 4 bg exactly, so are the sums, t and q."""
    d, s = resident(crt, "cornell")
    w, h = tgl.dims(kind, 5, 3)
    cam = camera(crt, d, w, h, 8)
    lens = lens_for(crt, d, kind, origin=(1.0, math.nan, 2.0))
    buf = Buffers(w, h)
    lens_pass(s, cam, lens, buf, 0, 4)
    lens_pass(s, cam, lens, buf, 4, 4)
    bg = np.array([0.0 + 1.0 * b for b in BG])
    rad = np.broadcast_to(bg, (h, w, 8, 3))
    want = lpm.lens_pass(lpm.lens_pass(lpm.fresh_state(w, h), rad[:, :, :4], 0, 4), rad[:, :, 4:], 4, 4)
    assert same_state(buf.state(), want)
    assert same(want["sum"], np.broadcast_to(8 * bg, (h, w, 3))) and same(want["rgb"], np.broadcast_to(bg, (h, w, 3)))


def test_refused_calls_leave_the_buffers_untouched(crt):
    from cpp_raytracer_amd import CrtError
    d, s = resident(crt, "cornell")
    cam = camera(crt, d, 4, 4, 24)
    buf = Buffers(4, 4, np.zeros(1, np.uint32))
    eq = crt.make_lens("equirect")
    for first, count, lens, word in ((2, 4, eq, "not a multiple of the chunk length"), (0, 0, eq, "num_samples is 0"),
                                     (20, 8, eq, "exceeds samples_per_pixel"), (4, 6, eq, "the pass ends at sample 10"),
                                     (0, 4, crt.make_lens("cube"), "CUBE needs image_h == 6 \\* image_w"),
                                     (0, 4, crt.make_lens("orthographic"), "ORTHOGRAPHIC extents must be > 0")):
        with pytest.raises(CrtError, match=r"\(-1\).*" + word):
            lens_pass(s, cam, lens, buf, first, count)
    with pytest.raises(CrtError, match=r"\(-1\).*d_sum is null"):
        s.render_lens_pass(0, cam, eq, 0, 4, 0)
    fresh = crt.GpuScene(rs.scene_data(crt, "cornell"))
    with pytest.raises(CrtError, match=r"\(-4\).*not uploaded"):
        lens_pass(fresh, cam, eq, buf, 0, 4)
    fresh.close()
    assert all((buf.raw(k) == 0xFF).all() for k in ("sum", "noise", "rgb"))
    assert (buf.words() == 0).all()
