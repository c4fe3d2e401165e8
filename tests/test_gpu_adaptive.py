"""Adaptive sampling on the GPU: blocks of 16 x 4 pixels stop between passes once their noise is
low enough, and a masked pass renders the others only. A block that stops after n samples holds,
bit for bit, what the plain pass API (crt_render_pass_async) holds after n samples; the stop map
equals the one the stopping rule gives on the oracle's per-sample radiances; tilings, bands, the
hint, caller-set regions, the blocking driver and checkpoints do not change a bit. Frames are
50 x 30 (no multiple of the 16 x 4 block: edge blocks take part)."""
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "oracle"))
import crt_oracle_py as orc  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 50, 30
BW, BH = 16, 4
NBX, NBY = (W + BW - 1) // BW, (H + BH - 1) // BH
STOPPED = 0x80000000
NAN = float("nan")


def scene(crt, name, seed=None, **cam):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named(name, seed)
    d.camera = camera_with(d.camera, image_w=cam.pop("image_w", W), image_h=cam.pop("image_h", H), **cam)
    return d


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def one_shot(s, cam):
    import torch
    out = torch.full((cam.image_h, cam.image_w, 3), NAN, dtype=torch.float64, device="cuda")
    s.render_async(0, cam, out.data_ptr(), stream())
    torch.cuda.synchronize()
    return out


def buffers(rows, w):
    """NaN-filled sums, noise state and frame (the first pass must overwrite them)."""
    import torch
    return [torch.full((rows, w, k), NAN, dtype=torch.float64, device="cuda") for k in (3, 2, 3)]


def words_of(blocks):
    return blocks.cpu().numpy().view(np.uint32)


def adaptive(crt, s, cam, bounds, threshold, min_samples, tiling=None, rows=None, hint=None, words=None):
    """One masked pass and one update per pass of `bounds`. Returns (sums, noise, frame, block
    words as uint32, the active count after each update). hint: the masked passes' active_hint
    (None: the last active count, as a driver passes it on); words: the initial block state."""
    import torch
    rows = rows or cam.image_h
    total, nz, out = buffers(cam.image_h if tiling is None or not tiling.flags & 1 else rows, cam.image_w)
    n = crt.block_count(cam.image_w, rows)
    blocks = torch.zeros(n, dtype=torch.int32, device="cuda")
    if words is not None:
        blocks.copy_(torch.from_numpy(np.asarray(words, np.uint32).view(np.int32).copy()))
    active, seen = 0, []
    for a, b in bounds:
        s.render_pass_masked(0, cam, a, b - a, total.data_ptr(), nz.data_ptr(), out.data_ptr(), blocks.data_ptr(),
                             active if hint is None else hint, stream(), tiling)
        active = crt.adaptive_update(0, cam, nz.data_ptr(), blocks.data_ptr(), b, threshold, min_samples, stream(),
                                     tiling)
        seen.append(active)
    torch.cuda.synchronize()
    return total, nz, out, words_of(blocks), seen


def plain(s, cam, bounds):
    """crt_render_pass_async over the same bounds: {samples done: (sums, noise state, preview)},
    cloned after each pass."""
    import torch
    total, nz, out = buffers(cam.image_h, cam.image_w)
    snaps = {}
    for a, b in bounds:
        s.render_pass(0, cam, a, b - a, total.data_ptr(), nz.data_ptr(), out.data_ptr(), stream())
        snaps[b] = (total.clone(), nz.clone(), out.clone())
    torch.cuda.synchronize()
    return snaps


def block_slices(w=W, h=H):
    nbx = (w + BW - 1) // BW
    return [(slice(BH * (b // nbx), min(h, BH * (b // nbx) + BH)), slice(BW * (b % nbx), min(w, BW * (b % nbx) + BW)))
            for b in range(nbx * ((h + BH - 1) // BH))]


def oracle_stop_map(smp, L, bounds, threshold, min_samples):
    """The stopping rule on per-sample radiances smp (h, w, spp, 3): chunk sums in sample order,
    y = (r + g) + b, crt_noise_estimate's per-pixel formulas, block sums of se and m. Returns (the
    samples each block ends with, the block ratios {samples done: array, NaN where sum m = 0}, the
    smallest |ratio / threshold - 1| among the decisions that were taken)."""
    h, w, spp, _ = smp.shape
    sl = block_slices(w, h)
    t = np.zeros((h, w))
    q = np.zeros((h, w))
    count = np.zeros(len(sl), np.int64)
    live = np.ones(len(sl), bool)
    ratios, margin = {}, np.inf
    for a, b in bounds:
        for c in range(a // L, b // L):
            S = np.zeros((h, w, 3))
            for i in range(c * L, (c + 1) * L):
                S = S + smp[:, :, i]
            y = (S[..., 0] + S[..., 1]) + S[..., 2]
            t = t + y
            q = q + y * y
        count[live] = b
        K = b // L
        if K < 2 or b < min_samples:
            continue
        m = t / (K * L)
        se = np.sqrt(np.maximum(0, q / (L * L) - K * m * m) / (K * (K - 1)))
        r = np.full(len(sl), np.nan)
        for i, (ys, xs) in enumerate(sl):
            sse, sm = se[ys, xs].sum(), m[ys, xs].sum()
            if sm > 0:
                r[i] = sse / sm
            if not live[i]:
                continue
            if sm > 0 and threshold > 0:
                margin = min(margin, abs(r[i] / threshold - 1))
            if sse <= threshold * sm:
                live[i] = False
        ratios[b] = r
    return count, ratios, margin


# every render_kernel instance (tests/test_gpu_progressive.py's list): LDS scene five waves
# sphere-only / flat-quad, LDS scene general (four waves), HBM scene with LDS stack, HBM stack, the
# linear (always-entered leaf) walk, and the four-wave sphere-only instance
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
def test_never_stopping_is_the_one_shot_frame(crt, monkeypatch, name, seed, cam_kw, env, scene_kw):
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = scene(crt, name, seed, **cam_kw)
    s = crt.GpuScene(d, **scene_kw)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 11)
    spp = cam.samples_per_pixel
    bounds = [(0, 8), (8, 12), (12, 22)] if spp == 22 else [(0, 4), (4, spp)]
    want = one_shot(s, cam)
    assert torch.isfinite(want).all()
    _, _, out, words, seen = adaptive(crt, s, cam, bounds, 1e9, spp)  # min_samples = spp: never stop
    assert torch.equal(out, want)
    assert (words == spp).all() and seen == [NBX * NBY] * len(bounds)


SPP, L = 64, 4
BOUNDS = [(a, a + 8) for a in range(0, SPP, 8)]


@pytest.fixture(scope="module")
def rtow64(crt):
    """rtow_final 50 x 30 at 64 spp, base seed 13: the scene and the oracle's per-sample radiances
    (h, w, 64, 3), computed once and left unchanged."""
    d = scene(crt, "rtow_final", 42, samples_per_pixel=SPP)
    _, smp = orc.render(d, 13, threads=8, samples=True)
    smp.setflags(write=False)
    return d, smp


@pytest.fixture(scope="module")
def rtow64_gpu(crt, rtow64):
    """The adaptive render of rtow64 (threshold 0.08, min_samples 16, passes of 8) and the plain
    passes' snapshots, rendered once and left unchanged."""
    d, _ = rtow64
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 13)
    return adaptive(crt, s, cam, BOUNDS, 0.08, 16), plain(s, cam, BOUNDS)


def test_stop_map_equals_the_oracles(crt, rtow64, rtow64_gpu):
    _, smp = rtow64
    assert crt.sample_chunk_len(SPP) == L
    want, _, margin = oracle_stop_map(smp, L, BOUNDS, 0.08, 16)
    hist = {int(v): int((want == v).sum()) for v in np.unique(want)}
    print(f"oracle stop map {hist}, smallest |ratio / threshold - 1| = {margin:.3g}")
    # preconditions on the input: no decision near the threshold, and a map worth testing
    assert margin >= 1e-6
    assert len(hist) >= 4 and 16 in hist and 64 in hist
    (_, _, _, words, seen), _ = rtow64_gpu
    got = words & (STOPPED - 1)
    print("gpu block samples", got.reshape(NBY, NBX).tolist(), "active after each pass", seen)
    assert np.array_equal(got, want)
    # every block that ended before the last pass carries the stopped bit
    assert ((words & STOPPED) != 0)[want < SPP].all()
    assert seen == [int((want > b).sum()) if b < SPP else seen[-1] for _, b in BOUNDS]


def test_a_stopped_block_holds_the_plain_passes_bits(crt, rtow64_gpu):
    import torch
    (total, nz, out, words, _), snaps = rtow64_gpu
    counts = words & (STOPPED - 1)
    assert len(set(counts.tolist())) >= 4
    for (ys, xs), n in zip(block_slices(), counts.tolist()):
        p_sum, p_nz, p_out = snaps[n]
        assert torch.equal(total[ys, xs], p_sum[ys, xs]), (ys, xs, n)
        assert torch.equal(nz[ys, xs], p_nz[ys, xs]), (ys, xs, n)
        assert torch.equal(out[ys, xs], p_out[ys, xs]), (ys, xs, n)


def test_tilings_assemble_to_the_whole_frame(crt, rtow64, rtow64_gpu):
    import torch
    from cpp_raytracer_amd import Tiling
    from cpp_raytracer_amd.tiles import owned_rows
    d, _ = rtow64
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 13)
    (w_total, _, w_out, w_words, _), _ = rtow64_gpu
    for packed in (1, 0):
        frame = torch.full_like(w_out, NAN)
        total = torch.full_like(w_total, NAN)
        words = np.zeros((NBY, NBX), np.uint32)
        for t in range(3):
            rows = owned_rows(H, 4, 3, t)
            r_total, _, r_out, r_words, _ = adaptive(crt, s, cam, BOUNDS, 0.08, 16, Tiling(4, 3, t, packed), rows=len(rows))
            idx = torch.tensor(rows, device="cuda")
            frame[idx] = r_out if packed else r_out[idx]
            total[idx] = r_total if packed else r_total[idx]
            words[t::3] = r_words.reshape(-1, NBX)  # rows dealt in blocks of 4: block row j is frame block row 3 j + t
        assert np.array_equal(words.reshape(-1), w_words), packed
        assert torch.equal(frame, w_out) and torch.equal(total, w_total), packed
    with pytest.raises(crt.CrtError):
        adaptive(crt, s, cam, BOUNDS[:1], 0.08, 16, Tiling(2, 2, 0, 0), rows=16)


def test_bands(crt, monkeypatch):
    """200 x 134: the first pass's partial sums (2 chunks) take 1.3 MB, so a 1 MB budget bands it."""
    import torch
    d = scene(crt, "rtow_final", 42, image_w=200, image_h=134, samples_per_pixel=22, max_depth=20)
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 14)
    bounds = [(0, 8), (8, 12), (12, 22)]
    want = adaptive(crt, s, cam, bounds, 0.12, 8)
    counts = want[3] & (STOPPED - 1)
    print("block samples", {int(v): int((counts == v).sum()) for v in np.unique(counts)})
    assert len(np.unique(counts)) >= 2  # some blocks stop early, some go on
    monkeypatch.setenv("CRT_PARTIAL_MB", "1")
    got = adaptive(crt, s, cam, bounds, 0.12, 8)
    assert np.array_equal(got[3], want[3]) and got[4] == want[4]
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert torch.isfinite(got[2]).all()


def test_caller_set_region(crt):
    import torch
    d = scene(crt, "rtow_final", 42, samples_per_pixel=22)
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 11)
    keep = [5, NBX * NBY - 1]  # an inner block and the corner block (2 columns x 2 rows)
    words = np.full(NBX * NBY, STOPPED, np.uint32)
    words[keep] = 0
    total, nz, out, after, seen = adaptive(crt, s, cam, [(0, 8), (8, 12), (12, 22)], 1e9, 22, words=words)
    want = one_shot(s, cam)
    sl = block_slices()
    inside = torch.zeros(H, W, dtype=torch.bool, device="cuda")
    for b in keep:
        assert torch.equal(out[sl[b]], want[sl[b]])
        inside[sl[b]] = True
    assert torch.isfinite(out).all() and torch.isfinite(total).all() and torch.isfinite(nz).all()
    assert (out[~inside] == 0).all() and (total[~inside] == 0).all() and (nz[~inside] == 0).all()
    assert (total[inside] != 0).any()
    assert (after[keep] == 22).all() and (np.delete(after, keep) == STOPPED).all() and seen == [2, 2, 2]


def test_black_blocks_stop_and_lit_blocks_run_on(crt):
    """cornell at 50 x 30: the blocks beside the box see nothing but the black background."""
    import torch
    d = scene(crt, "cornell", None, samples_per_pixel=SPP, max_depth=50)
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 13)
    total, nz, out, words, _ = adaptive(crt, s, cam, BOUNDS, 0.05, 16)
    snaps = plain(s, cam, BOUNDS[:2])
    assert torch.isfinite(total).all() and torch.isfinite(nz).all() and torch.isfinite(out).all()
    counts = words & (STOPPED - 1)
    sl = block_slices()
    black = [b for b in range(NBX * NBY) if (snaps[16][0][sl[b]] == 0).all()]
    print(f"{len(black)} all-black blocks at 16 samples; block samples {counts.reshape(NBY, NBX).tolist()}")
    assert 0 < len(black) < NBX * NBY
    for b in range(NBX * NBY):
        if b in black:  # 0 <= threshold * 0: stopped at the first decision, nothing in it
            assert words[b] == (16 | STOPPED)
            assert (total[sl[b]] == 0).all() and (out[sl[b]] == 0).all() and (nz[sl[b]] == 0).all()
        else:
            assert counts[b] == SPP, (b, counts[b])


def test_the_hint_changes_no_bit(crt, rtow64, rtow64_gpu):
    import torch
    d, _ = rtow64
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 13)
    (w_total, w_nz, w_out, w_words, w_seen), _ = rtow64_gpu
    for hint in (0, 1, 10 ** 9):
        total, nz, out, words, seen = adaptive(crt, s, cam, BOUNDS, 0.08, 16, hint=hint)
        assert np.array_equal(words, w_words) and seen == w_seen, hint
        assert torch.equal(total, w_total) and torch.equal(nz, w_nz) and torch.equal(out, w_out), hint


@pytest.mark.parametrize("emulate", [None, "3", "16"])
def test_blocking_api(crt, monkeypatch, rtow64, rtow64_gpu, emulate):
    d, smp = rtow64
    s = crt.GpuScene(d)
    cam = crt.resolve_camera(d.camera, 13)
    if emulate:
        monkeypatch.setenv("CRT_EMULATE_DEVICES", emulate)
    (_, _, w_out, w_words, w_seen), snaps = rtow64_gpu
    w_counts = (w_words & (STOPPED - 1)).reshape(NBY, NBX)
    seen = []
    frame, counts, rendered = s.render_adaptive(cam, 0.08, 16, 8, lambda *a: seen.append(a) and False)
    assert np.array_equal(frame, w_out.cpu().numpy())
    assert counts.dtype == np.uint32 and np.array_equal(counts, w_counts)
    pixels = sum(int(w_counts.reshape(-1)[b]) * (ys.stop - ys.start) * (xs.stop - xs.start)
                 for b, (ys, xs) in enumerate(block_slices()))
    assert rendered == pixels
    assert [(a[0], a[1], a[2], a[3], a[4]) for a in seen] == [(b, SPP, n, NBX * NBY, None) for (_, b), n in zip(BOUNDS, w_seen)]
    # previews: the callback's frame is the returned array, the same bits at the end
    last = []
    frame2, counts2, _ = s.render_adaptive(cam, 0.08, 16, 8, lambda *a: last.append(a[4].copy()) and False, preview=True)
    assert np.array_equal(frame2, frame) and np.array_equal(counts2, counts) and np.array_equal(last[-1], frame)
    # threshold 0.2: every block is below it at 16 samples (the margin is asserted on the oracle)
    _, ratios, _ = oracle_stop_map(smp, L, BOUNDS[:2], 0.2, 16)
    worst = float(np.nanmax(ratios[16]))
    print(f"largest block noise at 16 samples: {worst:.4f}")
    assert worst < 0.2 * (1 - 1e-6)
    seen = []
    frame, counts, rendered = s.render_adaptive(cam, 0.2, 16, 8, lambda *a: seen.append(a[:4]) and False)
    assert seen == [(8, SPP, NBX * NBY, NBX * NBY), (16, SPP, 0, NBX * NBY)]
    assert (counts == 16).all() and rendered == 16 * W * H
    assert np.array_equal(frame, snaps[16][2].cpu().numpy())
    # a callback that stops after the first pass: the 8-sample preview
    for preview in (False, True):
        calls = []
        frame, counts, rendered = s.render_adaptive(cam, 0.08, 16, 8, lambda *a: calls.append(a[0]) or True, preview=preview)
        assert calls == [8] and (counts == 8).all() and rendered == 8 * W * H
        assert np.array_equal(frame, snaps[8][2].cpu().numpy()), preview


def test_resume(crt, rtow64, rtow64_gpu):
    import torch
    from cpp_raytracer_amd.adaptive import AdaptiveRender
    d, _ = rtow64
    cam = crt.resolve_camera(d.camera, 13)
    (_, _, w_out, w_words, w_seen), _ = rtow64_gpu
    ar = AdaptiveRender(crt.GpuScene(d), cam, 0.08, 16)
    ar.step(8)
    ar.step(8)
    assert ar.samples_done == 16 and ar.active_blocks == w_seen[1] and not ar.finished
    state = ar.state()
    del ar
    ar2 = AdaptiveRender.resume(crt.GpuScene(d), cam, state)
    assert ar2.samples_done == 16 and ar2.active_blocks == w_seen[1]
    while not ar2.finished:
        frame = ar2.step(8)
    torch.cuda.synchronize()
    assert torch.equal(frame, w_out)
    assert np.array_equal(ar2.block_words().reshape(-1), w_words)
    counts = (w_words & (STOPPED - 1)).reshape(NBY, NBX)
    want_map = np.repeat(np.repeat(counts, BH, axis=0), BW, axis=1)[:H, :W]
    got_map = ar2.sample_map()
    assert got_map.dtype == np.uint32 and got_map.shape == (H, W) and np.array_equal(got_map, want_map)
    assert ar2.samples_rendered == int(want_map.sum())
    with pytest.raises(crt.CrtError):
        ar2.step(8)
    with pytest.raises(crt.CrtError, match="different sample counts"):
        ar2.noise()  # one frame-wide figure at samples_done means nothing here
