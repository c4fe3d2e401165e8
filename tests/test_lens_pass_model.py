"""tests/lens_pass_model.py checked on its own, without a GPU, on the oracle's radiance of the lens
model's rays: passes in order end in lens_model.frame's bits, t and q equal a direct evaluation, the
ragged chunk stays out of the noise, the masked skip rules, the centre rays, and the adaptive scenario
the GPU tests run (tests/test_gpu_lens_passes.py) is a real mix of stopped and active blocks."""
import numpy as np
import pytest

import lens_model as lm
import lens_pass_model as lpm
import pass_model as pm
import ray_sets as rs
from oracle import crt_oracle_py as orc

BG = (0.35, 0.6, 1.25)
SEED = 0xC0FFEE
INSIDE_CORNELL = (278.0, 400.0, 120.0)
_RAD = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def setup(crt, name, kind, w, h, spp, inside=False):
    from cpp_raytracer_amd import _capi, camera_with
    d = rs.scene_data(crt, name)
    cam = crt.resolve_camera(camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp, max_depth=50), SEED)
    cam.background = _capi.D3(*BG)
    c = d.camera
    o = np.array(list(c.center))
    f = np.array(list(c.lookat)) - o if c.has_lookat else np.array(list(c.direction))
    kw = dict(extent_x=0.4 * float(np.sqrt(f.dot(f))), extent_y=0.3 * float(np.sqrt(f.dot(f)))) if kind == "orthographic" else {}
    lens = crt.make_lens(kind, origin=INSIDE_CORNELL if inside else tuple(o), forward=tuple(f), up=tuple(c.up), **kw)
    return d, cam, lens


def radiance(crt, name, kind, w, h, spp, inside=False):
    """(h, w, spp, 3): the oracle's ray_color on the model's rays and states, computed once."""
    key = (name, kind, w, h, spp, inside)
    if key not in _RAD:
        d, cam, lens = setup(crt, name, kind, w, h, spp, inside)
        rays, states = lm.lens_rays(crt, cam, lens)
        rad = orc.radiance(d, rays, states, 50, BG, cam.t_min).reshape(h, w, spp, 3)
        rad.setflags(write=False)
        _RAD[key] = rad
    return _RAD[key]


CASES = [("pinhole", 7, 5), ("orthographic", 7, 5), ("cube", 2, 12)]


@pytest.mark.parametrize("kind,w,h", CASES)
@pytest.mark.parametrize("spp,per_pass,chunks", [(9, 4, [4, 4, 1]), (9, 8, [4, 4, 1]), (24, 8, [4] * 6), (24, 4, [4] * 6)])
def test_passes_in_order_are_the_one_shot_frame(crt, kind, w, h, spp, per_pass, chunks):
    L = pm.chunk_len(spp)
    assert L == 4 == crt.sample_chunk_len(spp)
    assert [min(L, spp - c) for c in range(0, spp, L)] == chunks
    rad = radiance(crt, "cornell", kind, w, h, spp)
    assert np.abs(rad).max() > 0
    st = lpm.fresh_state(w, h)
    for first, count in lpm.pass_plan(spp, L, per_pass):
        lpm.lens_pass(st, rad[:, :, first:first + count], first, L)
        done = first + count
        assert same(st["rgb"], st["sum"] * (1 / float(done)))
        assert same(st["noise"], lpm.direct_noise(rad[:, :, :done], L)), (kind, done)
        if done % L == 0:  # a frame of whole chunks is the one-shot frame of a job of that many samples
            assert same(st["rgb"], lm.frame(rad[:, :, :done], L)), (kind, done)
    assert same(st["rgb"], lm.frame(rad, L)), kind


def test_the_ragged_chunk_is_absent_from_the_noise(crt):
    rad = radiance(crt, "cornell", "orthographic", 7, 5, 9)
    st = lpm.fresh_state(7, 5)
    lpm.lens_pass(st, rad, 0, 4)
    assert same(st["noise"], lpm.direct_noise(rad[:, :, :8], 4))       # samples 0..7 only
    assert not same(st["sum"], lpm.accumulate(None, None, rad[:, :, :8], 0, 4)[0])  # the sum does hold sample 8
    one = lpm.fresh_state(7, 5)
    lpm.lens_pass(one, rad[:, :, :3], 0, 4)                                 # a job of 3 samples: one ragged chunk
    assert (bits(one["noise"]) == 0).all()


def test_a_fresh_pass_starts_from_chunk_zero(crt):
    """-0.0 shows the difference: 0.0 + (-0.0) is +0.0, so a chunk sum is never -0.0, and the running
    sum of a fresh pass is chunk 0's sum itself; the stored sums (NaN here) are not read."""
    rad = np.zeros((1, 1, 8, 3))
    rad[..., 0] = -0.0
    st = lpm.fresh_state(1, 1)
    lpm.lens_pass(st, rad, 0, 4)
    assert (bits(st["sum"]) == 0).all() and (bits(st["noise"]) == 0).all() and (bits(st["rgb"]) == 0).all()


def test_masked_skip_rules():
    rng = np.random.default_rng(5)
    w, h = 33, 9
    rad = rng.random((h, w, 8, 3))
    st = lpm.fresh_state(w, h, blocks=True)
    st["words"][[1, 5]] = pm.STOPPED          # pre-set: a region only
    st["words"][7] = 4                        # another count: skipped too
    lpm.lens_pass(st, rad[:, :, :4], 0, 4)
    on, _ = lpm.pixel_mask(np.where(np.isin(np.arange(9), [1, 5, 7]), 1, 0), w, h, 0)
    for k in ("sum", "noise", "rgb"):
        assert (bits(st[k][~on]) == 0).all(), k   # written 0 by a pass from sample 0
    assert same(st["sum"][on], lpm.accumulate(None, None, rad[:, :, :4], 0, 4)[0][on])
    assert st["words"].tolist() == [4, pm.STOPPED, 4, 4, 4, pm.STOPPED, 4, 4, 4]
    before = {k: np.array(v) for k, v in st.items()}
    st["words"][0] |= pm.STOPPED              # stopped after 4 samples
    lpm.lens_pass(st, rad[:, :, 4:], 4, 4)
    ys, xs = pm.block_slices(w, h)[0]
    assert same(st["sum"][ys, xs], before["sum"][ys, xs]) and same(st["noise"][ys, xs], before["noise"][ys, xs])
    assert same(st["rgb"][ys, xs], before["sum"][ys, xs] * (1 / 4.0))
    ys, xs = pm.block_slices(w, h)[1]          # count 0: the frame is 0
    assert (bits(st["rgb"][ys, xs]) == 0).all()
    ys, xs = pm.block_slices(w, h)[2]
    assert same(st["rgb"][ys, xs], lm.frame(rad, 4)[ys, xs])
    assert st["words"].tolist() == [4 | pm.STOPPED, pm.STOPPED, 8, 8, 8, pm.STOPPED, 8, 8, 8]


@pytest.mark.parametrize("kind", ["equirect", "cube"])
def test_the_adaptive_scenario_is_a_mix(crt, kind):
    w, h = lpm.SCEN_FRAMES[kind]
    assert len(pm.block_slices(w, h)) == (9 if kind == "equirect" else 8)
    rad = radiance(crt, "cornell", kind, w, h, lpm.SCEN_SPP, lpm.SCEN_INSIDE[kind])
    # the ratios the thresholds were chosen from: every block after every pass, nothing stopped
    st = lpm.fresh_state(w, h)
    for first, count in lpm.pass_plan(lpm.SCEN_SPP, 4, lpm.SCEN_PASS):
        lpm.lens_pass(st, rad[:, :, first:first + count], first, 4)
        sse, sm = pm.block_sums(st["noise"], w, h, (first + count) // 4, 4)
        with np.errstate(all="ignore"):
            print(kind, first + count, np.array2string(sse / sm, precision=4, max_line_width=200))
    steps = lpm.run_adaptive(rad, lpm.SCEN_PASS, lpm.SCEN_THRESHOLD[kind])
    counts, stopped = lpm.check_mix(steps)
    print(kind, "counts", counts.tolist(), "stopped", stopped.tolist())
    assert len(steps) == lpm.SCEN_SPP // lpm.SCEN_PASS  # a block is active to the end
    # a stopped block holds what plain passes hold after its own count, and its frame is that mean
    final = steps[-1][2]
    for b, (ys, xs) in enumerate(pm.block_slices(w, h)):
        n = int(counts[b])
        assert same(final["rgb"][ys, xs], lm.frame(rad[:, :, :n], 4)[ys, xs]), b
        assert same(final["noise"][ys, xs], lpm.direct_noise(rad[:, :, :n], 4)[ys, xs]), b


@pytest.mark.parametrize("kind", ["pinhole", "orthographic", "equirect", "fisheye", "cube"])
def test_centre_rays(crt, kind):
    """For the kinds other than PINHOLE the jitter-free generator adds +0.0 where the centre rays leave
    the term out: the same bits unless the sum is -0.0, which col + 0.5 never is. PINHOLE: the
    features' ray, centre - origin."""
    w, h = (3, 18) if kind == "cube" else (7, 5)
    _, cam, lens = setup(crt, "rtow_final", kind, w, h, 1)
    got = lpm.centre_rays(cam, lens)
    assert got.shape == (w * h, 6)
    if kind != "pinhole":
        want, _ = lm.lens_rays(crt, cam, lens, jitter=False)
        assert same(got, want)
        return
    O, P0 = np.array(list(cam.origin)), np.array(list(cam.pixel00))
    DX, DY = np.array(list(cam.pixel_delta_x)), np.array(list(cam.pixel_delta_y))
    for row, col in ((0, 0), (2, 5), (4, 6)):
        centre = (P0 + DY * float(row)) + DX * float(col)
        assert same(got[row * w + col], np.concatenate([O, centre - O]))
