"""The numpy restatements of crt_noise_estimate's tree and crt_adaptive_update's block rule
(tests/pass_model.py) checked on their own, and the synthetic states of
tests/test_gpu_pass_kernels.py shown to exercise what they claim before any GPU is involved: the tie
stops and one ulp below it does not, the NaN block stays, the clamp takes part."""
import math
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "tests"))
import denoise_model as dm  # noqa: E402
import pass_model as pm  # noqa: E402

INF = float("inf")
BELOW_TIE = float(np.nextafter(pm.TIE_THRESHOLD, 0.0))


def test_chunk_len_is_the_headers_formula():
    for spp in (1, 4, 22, 64, 768, 769, 1000, 10000):
        assert pm.chunk_len(spp) == max(4, math.ceil(spp / 192))
    assert (pm.chunk_len(22), pm.chunk_len(64), pm.chunk_len(1000)) == (4, 4, 6)


# ---- the tree --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", pm.NOISE_PIXELS)
def test_tree_is_within_one_rounding_per_addition_of_fsum(pixels):
    noise = pm.noise_state(pixels, 5, seed=pixels)
    se, m = pm.pixel_terms(noise, 5, 4)
    assert np.isfinite(se).all() and np.isfinite(m).all()
    got = pm.noise_tree(noise, 5, 4)
    for name, terms, value in (("se", se, got[0]), ("mean", m, got[1])):
        exact, bound = pm.tree_bound(terms)
        print(f"{pixels} pixels, sum {name}: tree {value!r}, fsum {exact!r}, gap {abs(value - exact):.3g}, bound {bound:.3g}")
        assert abs(value - exact) <= bound
    # the state is what it claims: the clamp takes part (but not everywhere), and exact zeros
    if pixels >= 255:
        var = noise[:, 1] / 16 - 5 * m * m
        assert 0.05 < (var < 0).mean() < 0.2 and 0.01 < (noise[:, 0] == 0).mean() < 0.1
        assert (se[var < 0] == 0).all() and (se > 0).any()
        ex = np.frexp(noise[noise[:, 0] > 0, 0])[1]
        assert ex.min() <= -35 and ex.max() >= 36


def test_tree_order_is_the_documented_one():
    # powers of two, one per thread slot and trip: every partial sum is exact, so any order gives
    # the same value; then one term that only the documented order rounds away
    n = pm.STRIDE + 3
    terms = np.zeros(n)
    terms[0] = 1.0
    terms[pm.STRIDE] = 2.0 ** -53      # thread 0's second trip: 1 + 2^-53 rounds to 1 (ties to even)
    terms[1] = 2.0 ** -53              # thread 1, joins thread 0 at the last halving: 1 + 2^-53 again
    assert pm.tree_sum(terms) == 1.0
    assert math.fsum(terms) == 1.0 + 2.0 ** -52
    # a term per block: stage 2 adds block b to block b + 128 first
    terms = np.zeros(pm.STRIDE)
    terms[0], terms[128 * 256], terms[256] = 1.0, 2.0 ** -53, 2.0 ** -53
    # (block 0 + block 128) rounds 2^-53 away; block 1 joins at the last halving and is rounded away too
    assert pm.tree_sum(terms) == 1.0
    terms[129 * 256] = 2.0 ** -53      # block 1 + block 129 = 2^-52 first: now it survives
    assert pm.tree_sum(terms) == 1.0 + 2.0 ** -52
    # a single pixel, and none
    assert pm.tree_sum([3.5]) == 3.5 and pm.tree_sum([]) == 0.0


def test_tree_takes_the_clamp_and_a_nan_pixel_as_the_kernel_does():
    noise = pm.noise_state(300, 5, seed=1)
    noise[17] = np.nan
    se, mean = pm.noise_tree(noise, 5, 4)
    ok = np.delete(noise, 17, axis=0)
    # fmax(0, NaN) = 0: the NaN pixel adds 0 to sum se (x + 0 changes no bit) and NaN to sum m
    assert math.isfinite(se) and math.isnan(mean)
    terms, _ = pm.pixel_terms(noise, 5, 4)
    assert terms[17] == 0 and se == pm.tree_sum(np.where(np.arange(300) == 17, 0.0, terms))
    assert math.isfinite(pm.noise_tree(ok, 5, 4)[1])


# ---- the butterfly and the block rule ----------------------------------------------------------------
def test_butterfly_gives_every_lane_the_same_bits():
    rng = np.random.default_rng(3)
    v = np.ldexp(rng.random((40, 64)), rng.integers(-30, 30, (40, 64)))
    out = pm.butterfly(v)
    assert np.array_equal(dm.bits(out), dm.bits(np.repeat(out[:, :1], 64, axis=1)))
    for row, lanes in zip(out[:, 0], v):
        assert abs(row - math.fsum(lanes)) <= 6 * pm.U * math.fsum(lanes)
    # the order is the xor order: ((l0 + l1) + (l2 + l3)) + ..., not a running sum
    v = np.zeros((1, 64))
    v[0, :4] = (1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53)
    assert pm.butterfly(v)[0, 0] == 1.0 + 2.0 ** -52  # 1 + 2^-53 = 1, 2^-53 + 2^-53 = 2^-52, then exact


def test_block_lanes_are_in_lane_order_and_zero_off_the_image():
    w, rows = 17, 5
    a = np.arange(1, w * rows + 1, dtype=np.float64).reshape(rows, w)
    lanes = pm.block_lanes(a, w, rows)
    assert lanes.shape == (4, 64)
    assert lanes[0, 0] == a[0, 0] and lanes[0, 17] == a[1, 1] and lanes[0, 63] == a[3, 15]
    assert lanes[1, 0] == a[0, 16] and (lanes[1].reshape(4, 16)[:, 1:] == 0).all()   # one pixel wide
    assert lanes[2, 5] == a[4, 5] and (lanes[2].reshape(4, 16)[1:] == 0).all()       # one pixel high
    assert lanes[3, 0] == a[4, 16] and np.count_nonzero(lanes[3]) == 1
    for lane_sum, (ys, xs) in zip(pm.butterfly(lanes)[:, 0], pm.block_slices(w, rows)):
        assert lane_sum == a[ys, xs].sum()  # small integers: exact in any order


@pytest.mark.parametrize("w,rows", pm.UPD_FRAMES)
def test_update_states_exercise_what_they_claim(w, rows):
    n_blocks = len(pm.block_slices(w, rows))
    assert n_blocks == ((w + 15) // 16) * ((rows + 3) // 4)
    seen = set()
    for rotate in range(7):
        noise, words, kinds = pm.update_state(w, rows, rotate, seed=rotate)
        seen |= set(kinds.tolist())
        sse, sm = pm.block_sums(noise, w, rows, 2, 4)
        sizes = np.array([(ys.stop - ys.start) * (xs.stop - xs.start) for ys, xs in pm.block_slices(w, rows)])
        tie, nanb, zero, clamp = (kinds == k for k in (pm.TIE, pm.NANB, pm.ZERO, pm.CLAMP))
        # the tie is exact for every block shape
        assert (sse[tie] == sizes[tie] / 8).all() and (sm[tie] == sizes[tie]).all()
        assert np.isnan(sm[nanb]).all() and (sse[nanb] == 0).all()
        assert (sse[zero] == 0).all() and (sm[zero] == 0).all()
        assert (sse[clamp] == 0).all() and (sm[clamp] == sizes[clamp]).all()
        at = words == pm.UPD_DONE

        def run(thr, min_samples=0, N=pm.UPD_N, done=pm.UPD_DONE):
            return pm.block_update(noise, words, w, rows, done, N, thr, min_samples)

        stopped = lambda out: (out & pm.STOPPED) != 0  # noqa: E731
        out, active = run(pm.TIE_THRESHOLD)
        assert stopped(out)[tie].all()                      # the tie stops
        out_below, _ = run(BELOW_TIE)
        assert not stopped(out_below)[tie].any()            # one ulp below it does not
        for thr in (0.0, pm.TIE_THRESHOLD, 1e300, sys.float_info.max, INF):
            o, a = run(thr)
            assert not stopped(o)[nanb].any()               # the NaN block stays, at any threshold
            assert stopped(o)[zero | clamp].all() or thr == INF  # inf * 0 is NaN: the model's own edge
            assert np.array_equal(o[~at], words[~at])       # everything not at samples_done is unchanged
            assert a == int((at & ~stopped(o)).sum()) and ((o & ~np.uint32(pm.STOPPED)) == (words & ~np.uint32(pm.STOPPED))).all()
        # random blocks: both outcomes occur at a middling threshold
        o, _ = run(pm.MID_THRESHOLD)
        seen |= {("random stopped", bool(v)) for v in stopped(o)[kinds == pm.RANDOM]}
        # may_stop false three ways: nothing changes, the count is the blocks at samples_done
        for kw in (dict(min_samples=16), dict(min_samples=pm.UPD_N)):
            o, a = run(pm.TIE_THRESHOLD, **kw)
            assert np.array_equal(o, words) and a == int(at.sum())
        n4, w4, _ = pm.update_state(w, rows, rotate, seed=rotate, samples_done=4)
        o, a = pm.block_update(n4, w4, w, rows, 4, pm.UPD_N, pm.TIE_THRESHOLD, 0)
        assert np.array_equal(o, w4) and a == int((w4 == 4).sum())
    assert set(range(7)) <= seen  # every block kind occurs in every frame, the one-block frames included
    if n_blocks > 100:
        assert ("random stopped", True) in seen and ("random stopped", False) in seen
    # the frames whose last wave of four blocks is not full
    assert (n_blocks % 4 != 0) == ((w, rows) in ((16, 4), (1, 1), (33, 9), (80, 9), (528, 260)))
    assert {len(pm.block_slices(*f)) for f in pm.UPD_FRAMES} == {32, 1, 4, 9, 15, 2145}


def test_block_update_under_a_tiling_is_the_model_on_the_owned_rows():
    rows = pm.owned_rows(30, 4, 3, 1)
    assert rows == [4, 5, 6, 7, 16, 17, 18, 19, 28, 29]
    noise, words, kinds = pm.update_state(50, len(rows), 0, seed=9)
    assert len(words) == 4 * 3  # the last block row is two rows high
    out, active = pm.block_update(noise, words, 50, len(rows), pm.UPD_DONE, pm.UPD_N, pm.TIE_THRESHOLD, 0)
    assert ((out & pm.STOPPED) != 0)[kinds == pm.TIE].all() and 0 < active < 12
