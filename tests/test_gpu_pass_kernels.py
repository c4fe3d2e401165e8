"""The pass kernels that never trace a ray, on synthetic state and with no render: crt_noise_estimate
against its tree (tests/pass_model.py) bit for bit up to 131,372 pixels (three trips of the strided
loop), crt_adaptive_update against the block rule on exact ties, NaN, black and clamped blocks in
frames of 1 to 2145 blocks (the tail wave of the last four blocks included), and
crt_pixel_variance_async against tests/denoise_model.py on clamp pixels, signed zeros, NaN, inf and
denormals. Every input has NaN records past its end and every output has sentinels past its end."""
import math
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "tests"))
import denoise_model as dm  # noqa: E402
import pass_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 64  # records past the end of every buffer
STOPPED = pm.STOPPED
BELOW_TIE = float(np.nextafter(pm.TIE_THRESHOLD, 0.0))
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def camera(crt, w, h, spp):
    from cpp_raytracer_amd import camera_with
    return crt.resolve_camera(camera_with(crt.SceneData.named("rtow_final", 42).camera, image_w=w, image_h=h,
                                          samples_per_pixel=spp))


def padded(a, fill=NAN):
    """a's elements on the device followed by PAD * (elements per record) of `fill`."""
    import torch
    a = np.ascontiguousarray(a)
    flat = np.concatenate([a.reshape(-1), np.full(PAD * int(np.prod(a.shape[1:], dtype=np.int64) or 1), fill, a.dtype)])
    return torch.from_numpy(flat).cuda()


def same_bits(a, b):
    return np.array_equal(dm.bits(a), dm.bits(b))


# ---- crt_noise_estimate ------------------------------------------------------------------------------
def gpu_noise(crt, noise, spp, done):
    import torch
    buf = padded(noise)
    got = crt.noise_estimate(0, buf.data_ptr(), len(noise), spp, done, stream())
    again = crt.noise_estimate(0, buf.data_ptr(), len(noise), spp, done, stream())
    torch.cuda.synchronize()
    assert same_bits(got, again)  # a fixed tree: two calls give equal bits
    assert same_bits(buf.cpu().numpy()[:noise.size], noise.reshape(-1))
    return got


@pytest.mark.parametrize("pixels", pm.NOISE_PIXELS)
def test_noise_estimate_equals_the_tree(crt, pixels):
    assert crt.sample_chunk_len(22) == 4 == pm.chunk_len(22)
    noise = pm.noise_state(pixels, 5, seed=pixels)
    got = gpu_noise(crt, noise, 22, 22)  # K = 5 chunks of L = 4 (the two last samples are a ragged chunk)
    want = pm.noise_tree(noise, 5, 4)
    terms = pm.pixel_terms(noise, 5, 4)
    for name, g, wv, t in zip(("sum_se", "sum_mean"), got, want, terms):
        exact, bound = pm.tree_bound(t)
        print(f"{pixels} pixels ({-(-pixels // pm.STRIDE)} trips) {name}: gpu {g!r} model {wv!r} fsum {exact!r} "
              f"relative gap {abs(g - exact) / exact:.3g} bound {bound / exact:.3g}")
        assert abs(g - exact) <= bound
    assert same_bits(got, want)


def test_noise_estimate_with_chunks_of_six(crt):
    assert crt.sample_chunk_len(1000) == 6 == pm.chunk_len(1000)
    pixels = pm.STRIDE + 257
    K = 1000 // 6
    noise = pm.noise_state(pixels, K, seed=6)
    got = gpu_noise(crt, noise, 1000, 1000)
    assert same_bits(got, pm.noise_tree(noise, K, 6))
    assert not same_bits(got, pm.noise_tree(noise, 1000 // 4, 4))  # L matters to the bits compared
    for g, t in zip(got, pm.pixel_terms(noise, K, 6)):
        exact, bound = pm.tree_bound(t)
        assert abs(g - exact) <= bound


@pytest.mark.parametrize("pixels,where", [(300, 17), (pm.STRIDE + 257, pm.STRIDE + 1)])
def test_noise_estimate_with_a_nan_pixel(crt, pixels, where):
    noise = pm.noise_state(pixels, 5, seed=2)
    noise[where] = NAN
    se, mean = gpu_noise(crt, noise, 22, 22)
    want = pm.noise_tree(noise, 5, 4)
    assert math.isfinite(se) and same_bits(se, want[0]) and math.isnan(mean) and math.isnan(want[1])


# ---- crt_adaptive_update -----------------------------------------------------------------------------
def gpu_update(crt, cam, noise, words, done, thr, min_samples=0, tiling=None):
    """(new words, active count); the words are followed by PAD words equal to `done`: a block past
    the end that the kernel took would be counted as active (its noise is NaN)."""
    import torch
    nbuf = noise if isinstance(noise, torch.Tensor) else padded(noise)
    blocks = torch.from_numpy(np.concatenate([words, np.full(PAD, done, np.uint32)]).view(np.int32).copy()).cuda()
    active = crt.adaptive_update(0, cam, nbuf.data_ptr(), blocks.data_ptr(), done, thr, min_samples, stream(), tiling)
    torch.cuda.synchronize()
    out = blocks.cpu().numpy().view(np.uint32)
    assert (out[len(words):] == done).all()
    return out[:len(words)], active


@pytest.mark.parametrize("w,h", pm.UPD_FRAMES)
def test_adaptive_update_equals_the_block_rule(crt, w, h):
    cam = camera(crt, w, h, pm.UPD_N)
    n_blocks = crt.block_count(w, h)
    rotations = range(7) if n_blocks < 100 else (0, 3)
    for rotate in rotations:
        noise, words, kinds = pm.update_state(w, h, rotate, seed=rotate)
        tie, nanb, zero, clamp = (kinds == k for k in (pm.TIE, pm.NANB, pm.ZERO, pm.CLAMP))
        at = words == pm.UPD_DONE
        nbuf = padded(noise)
        for thr in (pm.TIE_THRESHOLD, BELOW_TIE, 0.0, pm.MID_THRESHOLD, sys.float_info.max):
            got, active = gpu_update(crt, cam, nbuf, words, pm.UPD_DONE, thr)
            want, want_active = pm.block_update(noise, words, w, h, pm.UPD_DONE, pm.UPD_N, thr, 0)
            assert np.array_equal(got, want) and active == want_active, (rotate, thr)
            stopped = (got & STOPPED) != 0
            # the header's rules, stated on the GPU's own answer
            assert stopped[tie].all() if thr >= pm.TIE_THRESHOLD else not stopped[tie].any()  # a tie stops; an ulp below does not
            assert not stopped[nanb].any() and stopped[zero | clamp].all()
            assert np.array_equal(got[~at], words[~at])
    print(f"{w} x {h}: {n_blocks} blocks, {(n_blocks + 3) // 4} waves of four, {n_blocks % 4} in the last")
    # an infinite threshold is refused (the header: finite and >= 0), so the largest finite one stands for it
    with pytest.raises(crt.CrtError):
        gpu_update(crt, cam, noise, words, pm.UPD_DONE, float("inf"))


@pytest.mark.parametrize("w,h", [(50, 30), (17, 5), (528, 260)])
def test_adaptive_update_when_no_block_may_stop(crt, w, h):
    cam = camera(crt, w, h, pm.UPD_N)
    noise, words, _ = pm.update_state(w, h, 0, seed=4)
    for done, min_samples in ((pm.UPD_DONE, 16), (pm.UPD_DONE, pm.UPD_N)):  # too early; never
        got, active = gpu_update(crt, cam, noise, words, done, pm.TIE_THRESHOLD, min_samples)
        assert np.array_equal(got, words) and active == int((words == done).sum()) > 0
    noise, words, _ = pm.update_state(w, h, 0, seed=4, samples_done=4)  # K = 1
    got, active = gpu_update(crt, cam, noise, words, 4, pm.TIE_THRESHOLD)
    assert np.array_equal(got, words) and active == int((words == 4).sum()) > 0


@pytest.mark.parametrize("packed", [0, 1])
def test_adaptive_update_under_a_tiling(crt, packed):
    from cpp_raytracer_amd import Tiling
    w, h = 50, 30
    cam = camera(crt, w, h, pm.UPD_N)
    rows = pm.owned_rows(h, 4, 3, 1)
    for rotate in range(7):
        noise, words, kinds = pm.update_state(w, len(rows), rotate, seed=20 + rotate)
        frame = np.full((h, w, 2), NAN)  # NaN in every row not owned
        frame[rows] = noise
        for thr in (pm.TIE_THRESHOLD, BELOW_TIE, pm.MID_THRESHOLD):
            got, active = gpu_update(crt, cam, noise if packed else frame, words, pm.UPD_DONE, thr,
                                     tiling=Tiling(4, 3, 1, packed))
            want, want_active = pm.block_update(noise, words, w, len(rows), pm.UPD_DONE, pm.UPD_N, thr, 0)
            assert np.array_equal(got, want) and active == want_active, (rotate, thr)
            tie = ((got & STOPPED) != 0)[kinds == pm.TIE]
            assert tie.size and (tie.all() if thr == pm.TIE_THRESHOLD else not tie.any())


# ---- crt_pixel_variance_async -------------------------------------------------------------------------
SPECIALS = [0.0, -0.0, NAN, float("inf"), float("-inf"), 5e-324, 2.0 ** -1060, -2.0 ** -1050, 2.2250738585072014e-308]


def variance_state(w, rows, seed):
    """t, q with clamp pixels (a tenth), and a fifth of the records holding signed zeros, NaN,
    infinities and denormals in t, in q or in both."""
    rng = np.random.default_rng(seed)
    noise = pm.update_state(w, rows, 4, seed)[0]  # RANDOM everywhere but the special blocks: ties, NaN, black, clamp
    special = rng.random((rows, w, 2)) < 0.12
    noise[special] = rng.choice(SPECIALS, int(special.sum()))
    # and every special value once in t alone, in q alone (t = 8) and in both, at scattered pixels
    flat = noise.reshape(-1, 2)
    where = rng.permutation(len(flat))[:3 * len(SPECIALS)].reshape(3, -1)
    flat[where[0], 0] = SPECIALS
    flat[where[1]] = np.stack([np.full(len(SPECIALS), 8.0), SPECIALS], -1)
    flat[where[2]] = np.stack([SPECIALS, SPECIALS], -1)
    return noise


def gpu_variance(crt, cam, noise, done, words=None, tiling=None, out_shape=None):
    """The variance buffer as bit patterns, 0xFF-filled before the call, its PAD sentinels checked."""
    import torch
    nbuf = padded(noise)
    rows, w = out_shape
    var = torch.full(((rows * w + PAD) * 8,), 0xFF, dtype=torch.uint8, device="cuda")
    blocks = torch.from_numpy(np.asarray(words, np.uint32).view(np.int32).copy()).cuda() if words is not None else None
    crt.pixel_variance(0, cam, nbuf.data_ptr(), var.data_ptr(), done, blocks.data_ptr() if blocks is not None else 0,
                       stream(), tiling)
    torch.cuda.synchronize()
    out = var.cpu().numpy().view(np.uint64)
    assert (out[rows * w:] == ONES).all()
    return out[:rows * w].reshape(rows, w)


def variance_words(n_blocks):
    return np.array([(0, 4, 8, 64, 8 | STOPPED, 64 | STOPPED, 12)[b % 7] for b in range(n_blocks)], np.uint32)


@pytest.mark.parametrize("w,h", [(50, 30), (17, 5)])
def test_pixel_variance_equals_the_model_on_special_values(crt, w, h):
    cam = camera(crt, w, h, 64)
    noise = variance_state(w, h, seed=w)
    for v in SPECIALS:
        assert (dm.bits(noise) == dm.bits(np.float64(v))).any()
    for done in (0, 4, 8, 64):  # K = 0: every pixel 0, the state is not read; K = 1: m * m; K >= 2
        got = gpu_variance(crt, cam, noise, done, out_shape=(h, w))
        want = dm.pixel_variance(noise, done, 4)
        assert np.array_equal(got, dm.bits(want)), done
    # max0: a negative, -0 or NaN variance gives +0, so K >= 2 never gives a NaN; K = 1 (m * m) does
    v = want
    assert (v == 0).sum() > w * h // 20 and not np.isnan(v).any() and np.isinf(v).any() and not (v < 0).any()
    assert not np.signbit(v[v == 0]).any()
    assert np.isnan(dm.pixel_variance(noise, 4, 4)).any()
    # with block words: each block's own count, the stopped bit ignored
    words = variance_words(crt.block_count(w, h))
    counts = dm.block_counts_to_pixels(words.reshape((h + 3) // 4, (w + 15) // 16), h, w)
    got = gpu_variance(crt, cam, noise, 64, words, out_shape=(h, w))
    want = dm.pixel_variance(noise, counts, 4)
    assert np.array_equal(got, dm.bits(want))
    assert (want[counts == 0] == 0).all() and not np.signbit(want[counts == 0]).any()


@pytest.mark.parametrize("packed", [0, 1])
def test_pixel_variance_under_a_tiling(crt, packed):
    from cpp_raytracer_amd import Tiling
    w, h = 50, 30
    cam = camera(crt, w, h, 64)
    rows = pm.owned_rows(h, 4, 3, 1)
    other = [r for r in range(h) if r not in rows]
    noise = variance_state(w, len(rows), seed=77)
    frame = np.full((h, w, 2), NAN)
    frame[rows] = noise
    words = variance_words(crt.block_count(w, len(rows)))
    counts = dm.block_counts_to_pixels(words.reshape(3, 4), len(rows), w)
    for wd, n in ((None, 8), (words, counts)):
        want = dm.bits(dm.pixel_variance(noise, n, 4))
        if packed:
            got = gpu_variance(crt, cam, noise, 8, wd, Tiling(4, 3, 1, 1), out_shape=(len(rows), w))
            assert np.array_equal(got, want)
        else:
            got = gpu_variance(crt, cam, frame, 8, wd, Tiling(4, 3, 1, 0), out_shape=(h, w))
            assert np.array_equal(got[rows], want)
            assert (got[other] == ONES).all()  # rows not owned keep their fill bytes
