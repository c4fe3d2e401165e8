"""numpy restatements of the pass kernels that never trace a ray: crt_noise_estimate's two-stage tree
(noise_stage1_kernel / noise_stage2_kernel) and crt_adaptive_update's block rule
(adaptive_update_kernel and the host's may_stop), as include/crt_render.h and the comments above the
kernels state them: the same IEEE f64 operations in the same order, so the GPU results are compared
with == (tests/test_gpu_pass_kernels.py). The synthetic states those tests feed the kernels are built
here too, so tests/test_pass_model.py can show on the CPU that they exercise what they claim.
Not a test module."""
import math

import numpy as np

STOPPED = 0x80000000
BW, BH = 16, 4
NOISE_BLOCKS = 256                 # blocks of noise_stage1_kernel, 256 threads each
STRIDE = NOISE_BLOCKS * 256        # pixels one trip of its strided loop covers
U = 2.0 ** -53                     # unit roundoff of f64


def chunk_len(spp):
    """crt_sample_chunk_len: max(4, ceil(spp / 192))."""
    return max(4, -(-int(spp) // 192))


def pixel_terms(noise, K, L):
    """crt_noise_estimate's per-pixel se and m from noise (..., 2) = t, q; K chunks of L samples.
    fmax, not maximum: the kernel's fmax(0, NaN) is 0."""
    t, q = noise[..., 0], noise[..., 1]
    K, L = float(K), float(L)
    with np.errstate(all="ignore"):
        m = t / (K * L)
        var = q / (L * L) - K * m * m
        se = np.sqrt(np.fmax(0.0, var) / (K * (K - 1)))
    return se, m


def _halve(x):
    """Eight halvings of 256 values along the last axis: x[i] = x[i] + x[i + h], h = 128 .. 1."""
    x = np.array(x, np.float64)
    with np.errstate(all="ignore"):
        for h in (128, 64, 32, 16, 8, 4, 2, 1):
            x[..., :h] = x[..., :h] + x[..., h:2 * h]
    return x[..., 0]


def tree_sum(terms):
    """The fixed tree over per-pixel terms: thread j of block b adds pixels b * 256 + j, + 65536, ...
    in order, starting from 0; each block halves its 256 values; stage 2 halves the 256 block
    results. (A thread past the last pixel keeps adding nothing: x + 0 is x for every x the
    accumulator can hold, so the padding zeros change no bit.)"""
    terms = np.asarray(terms, np.float64).reshape(-1)
    trips = max(1, -(-len(terms) // STRIDE))
    padded = np.zeros(trips * STRIDE)
    padded[:len(terms)] = terms
    acc = np.zeros(STRIDE)
    with np.errstate(all="ignore"):
        for k in range(trips):
            acc = acc + padded[k * STRIDE:(k + 1) * STRIDE]
    return float(_halve(_halve(acc.reshape(NOISE_BLOCKS, 256))))


def noise_tree(noise, K, L):
    """crt_noise_estimate: (sum_se, sum_mean) over noise (pixels, 2) with K chunks of L samples."""
    se, m = pixel_terms(np.asarray(noise, np.float64).reshape(-1, 2), K, L)
    return tree_sum(se), tree_sum(m)


def tree_bound(terms):
    """(fsum of the terms, the bound on |tree_sum - fsum|): one rounding for every addition a term
    passes through, ceil(n / 65536) in its thread and 8 + 8 in the two halvings, each at most
    2^-53 of the partial sum's magnitude, which fsum(|terms|) bounds."""
    terms = [float(v) for v in np.asarray(terms, np.float64).reshape(-1)]
    depth = -(-len(terms) // STRIDE) + 16
    return math.fsum(terms), depth * U * math.fsum(abs(v) for v in terms)


def butterfly(v):
    """v (blocks, 64) lane values -> every lane's sum: v = v + v[lane ^ d] for d = 1, 2, ..., 32."""
    v = np.array(v, np.float64)
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for d in (1, 2, 4, 8, 16, 32):
            v = v + v[:, lane ^ d]
    return v


def block_lanes(a, w, rows):
    """a (rows, w) per-pixel values of the owned rows -> (blocks, 64) in lane order (col = lane % 16,
    row = lane / 16), blocks numbered by * ceil(w / 16) + bx; lanes off the image hold 0."""
    nbx, nby = (w + BW - 1) // BW, (rows + BH - 1) // BH
    full = np.zeros((nby * BH, nbx * BW))
    full[:rows, :w] = np.asarray(a, np.float64).reshape(rows, w)
    return full.reshape(nby, BH, nbx, BW).transpose(0, 2, 1, 3).reshape(nby * nbx, BH * BW)


def block_sums(noise, w, rows, K, L):
    """(sum se, sum m) of every block as lane 0 of the butterfly holds them."""
    se, m = pixel_terms(np.asarray(noise, np.float64).reshape(rows, w, 2), K, L)
    return butterfly(block_lanes(se, w, rows))[:, 0], butterfly(block_lanes(m, w, rows))[:, 0]


def block_update(noise, words, w, rows, samples_done, N, threshold, min_samples):
    """crt_adaptive_update over the owned rows' noise (rows, w, 2) and block words (uint32): the
    new words and the number of blocks still at samples_done and not stopped. A block at
    samples_done stops when may_stop (K >= 2, samples_done >= min_samples, min_samples < N) and
    sum se <= threshold * sum m; every other word is returned unchanged."""
    words = np.array(words, np.uint32).reshape(-1)
    L = chunk_len(N)
    K = samples_done // L
    here = words == np.uint32(samples_done)
    stop = np.zeros(len(words), bool)
    if K >= 2 and samples_done >= min_samples and min_samples < N:
        sse, sm = block_sums(noise, w, rows, K, L)
        with np.errstate(all="ignore"):
            stop = here & (sse <= np.float64(threshold) * sm)
    out = np.where(stop, words | np.uint32(STOPPED), words).astype(np.uint32)
    return out, int((here & ~stop).sum())


def block_slices(w, rows):
    nbx = (w + BW - 1) // BW
    return [(slice(BH * (b // nbx), min(rows, BH * (b // nbx) + BH)), slice(BW * (b % nbx), min(w, BW * (b % nbx) + BW)))
            for b in range(nbx * ((rows + BH - 1) // BH))]


# ---- the synthetic states of tests/test_gpu_pass_kernels.py -----------------------------------------
NOISE_PIXELS = (1, 255, 256, 257, 65535, 65536, 65537, 65536 * 2 + 300)


def noise_state(pixels, K, seed):
    """(pixels, 2) t, q of mixed magnitude, t = 2^-40 .. 2^40: q = (t^2 / K) (1 + r) makes the
    variance q / L^2 - K m^2 = r t^2 / (K L^2); about a tenth of the pixels get r < 0 (the
    clamp), about a twentieth are exactly zero. The first and the last pixel are neither and of the
    largest magnitude: a pixel past a boundary that is added twice, or not at all, shows in the sums."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-40, 40, pixels)
    e[[0, -1]] = 39
    t = np.ldexp(1 + rng.random(pixels), e)
    kind = rng.random(pixels)
    kind[[0, -1]] = 0.5
    r = np.where(kind < 0.1, -rng.uniform(0.01, 0.5, pixels), rng.uniform(0.0, 3.0, pixels))
    q = (t * t / K) * (1 + r)
    zero = kind > 0.95
    return np.stack([np.where(zero, 0.0, t), np.where(zero, 0.0, q)], -1)


# crt_adaptive_update: a job of N = 64 samples (L = 4) at samples_done = 8 (K = 2)
UPD_N, UPD_DONE = 64, 8
UPD_FRAMES = ((50, 30), (16, 4), (17, 5), (1, 1), (33, 9), (80, 9), (528, 260))  # 32, 1, 4, 1, 9, 15, 2145 blocks
TIE, NANB, ZERO, CLAMP, RANDOM, OTHER, DONE = range(7)  # what a block of update_state holds
TIE_THRESHOLD = 0.125
MID_THRESHOLD = 0.05  # splits the RANDOM blocks: some stop, some do not


def update_state(w, rows, rotate, seed, samples_done=UPD_DONE):
    """Noise (rows, w, 2), block words and each block's kind ((b + rotate) % 7) for K = 2, L = 4:
      TIE    every pixel t = 8, q = 32.5: m = 1 and se = sqrt((32.5 / 16 - 2) / 2) = 1 / 8 exactly, so
             sum se = n / 8 and sum m = n are exact for any n <= 64 pixels: sum se == 0.125 * sum m
      NANB   one NaN pixel (t and q) among black ones: sum m is NaN
      ZERO   all black: 0 <= threshold * 0
      CLAMP  every pixel t = 8, q = 16: the variance 1 - 2 is negative, se = 0, sum m = n > 0
      RANDOM random t, q (a tenth clamped), the word at samples_done
      OTHER  random t, q, the word at another count (4, 12 or 16)
      DONE   random t, q, a stopped word
    The first five have the word samples_done."""
    rng = np.random.default_rng(seed)
    sl = block_slices(w, rows)
    kinds = (np.arange(len(sl)) + rotate) % 7
    t = np.ldexp(1 + rng.random((rows, w)), rng.integers(-3, 4, (rows, w)))
    # se / m = sqrt(r): a block's ratio is about 0.6 * 10^-(b % 5) / 2, from well above to well below MID_THRESHOLD
    scale = np.zeros((rows, w))
    for b, (ys, xs) in enumerate(sl):
        scale[ys, xs] = 10.0 ** -(b % 5)
    r = np.where(rng.random((rows, w)) < 0.1, -0.25, rng.uniform(0.0, 1.0, (rows, w)) * scale)
    noise = np.stack([t, (t * t / 2) * (1 + r)], -1)
    words = np.full(len(sl), samples_done, np.uint32)
    for b, (ys, xs) in enumerate(sl):
        k = kinds[b]
        if k == TIE:
            noise[ys, xs] = (8.0, 32.5)
        elif k == NANB:
            noise[ys, xs] = 0.0
            n = (ys.stop - ys.start) * (xs.stop - xs.start)
            j = int(rng.integers(n))
            noise[ys.start + j // (xs.stop - xs.start), xs.start + j % (xs.stop - xs.start)] = np.nan
        elif k == ZERO:
            noise[ys, xs] = 0.0
        elif k == CLAMP:
            noise[ys, xs] = (8.0, 16.0)
        elif k == OTHER:
            words[b] = (4, 12, 16)[b % 3]
        elif k == DONE:
            words[b] = (STOPPED | samples_done, STOPPED | 4, STOPPED)[b % 3]
    return noise, words, kinds


def owned_rows(height, row_block, world, rank):
    """The rows crt_tiling{row_block, world, rank} owns."""
    return [r for r in range(height) if (r // row_block) % world == rank]
