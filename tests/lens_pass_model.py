"""A numpy restatement of crt_render_lens_pass_async's accumulation (include/crt_render.h: the running
sum, the noise state, the frame so far and the skip rules of a masked pass) over per-sample radiance,
and of crt_lens_centre_rays_async's records: what the device must write, computed without a GPU (the
feature records are denoise_model.features_from_hits'). The generator is lens_model's, the update rule pass_model.block_update.
Not a test module."""
import numpy as np

import lens_model as lm
import pass_model as pm

STOPPED = pm.STOPPED


def fresh_state(w, h, blocks=False):
    """The buffers before the first pass: sum, noise and frame of the whole frame (a pass from sample 0
    overwrites them, so their content is arbitrary: NaN here), and zeroed block words if asked for."""
    st = {"sum": np.full((h, w, 3), np.nan), "noise": np.full((h, w, 2), np.nan), "rgb": np.full((h, w, 3), np.nan)}
    if blocks:
        st["words"] = np.zeros(len(pm.block_slices(w, h)), np.uint32)
    return st


def accumulate(total, noise, rad, first, L):
    """accumulate_kernel's additions for pixels (..., count, 3) of samples [first, first + count):
    chunk c is the sum of its samples in order from 0.0; a pass from sample 0 starts the running sum
    from chunk 0's sum and t, q from 0, any other from the stored values; the chunk sums are added in
    chunk order; every chunk of L samples adds y = (r + g) + b and y * y to t and q.
    Returns (sum, noise, frame = sum * (1 / (double)(first + count)))."""
    count = rad.shape[-2]
    fresh = first == 0
    r = None if fresh else np.array(total, np.float64)
    t = np.zeros(rad.shape[:-2]) if fresh else np.array(noise[..., 0], np.float64)
    q = np.zeros(rad.shape[:-2]) if fresh else np.array(noise[..., 1], np.float64)
    with np.errstate(all="ignore"):
        for c0 in range(0, count, L):
            c1 = min(count, c0 + L)
            u = np.zeros(rad.shape[:-2] + (3,))
            for s in range(c0, c1):
                u = u + rad[..., s, :]
            r = u if r is None else r + u
            if c1 - c0 == L:
                y = (u[..., 0] + u[..., 1]) + u[..., 2]
                t = t + y
                q = q + y * y
        return r, np.stack([t, q], -1), r * (1 / float(first + count))


def pixel_mask(words, w, h, first):
    """(h, w) bool: the pixels of the blocks whose word equals `first`; and every pixel's block count."""
    on = np.zeros((h, w), bool)
    n = np.zeros((h, w), np.uint32)
    for b, (ys, xs) in enumerate(pm.block_slices(w, h)):
        on[ys, xs] = int(words[b]) == first
        n[ys, xs] = int(words[b]) & (STOPPED - 1)
    return on, n


def lens_pass(st, rad, first, L):
    """One pass on state `st` (fresh_state's keys; updated in place and returned). rad (h, w, count, 3):
    the radiance of samples [first, first + count) of every pixel (a skipped block's is not read).
    With st["words"]: only the blocks at `first` are accumulated and their words become first + count;
    a skipped block is zeroed in a pass from sample 0, else left alone with frame = sum * (1 / n), n its
    own count (0 when n = 0)."""
    h, w = rad.shape[:2]
    count = rad.shape[2]
    total, noise, rgb = accumulate(st["sum"], st["noise"], rad, first, L)
    if "words" not in st:
        st["sum"], st["noise"], st["rgb"] = total, noise, rgb
        return st
    words = st["words"]
    on, n = pixel_mask(words, w, h, first)
    if first == 0:
        skip_sum, skip_noise, skip_rgb = np.zeros((h, w, 3)), np.zeros((h, w, 2)), np.zeros((h, w, 3))
    else:
        skip_sum, skip_noise = st["sum"], st["noise"]
        with np.errstate(all="ignore"):
            inv = 1 / n.astype(np.float64)
            skip_rgb = np.where((n != 0)[..., None], st["sum"] * inv[..., None], 0.0)
    st["sum"] = np.where(on[..., None], total, skip_sum)
    st["noise"] = np.where(on[..., None], noise, skip_noise)
    st["rgb"] = np.where(on[..., None], rgb, skip_rgb)
    st["words"] = np.where(words == np.uint32(first), np.uint32(first + count), words).astype(np.uint32)
    return st


def direct_noise(rad, L):
    """t and q of samples [0, n) evaluated directly: over the full chunks only, in chunk order from 0."""
    n = rad.shape[-2]
    t = np.zeros(rad.shape[:-2])
    q = np.zeros(rad.shape[:-2])
    for c in range(n // L):
        u = np.zeros(rad.shape[:-2] + (3,))
        for s in range(c * L, (c + 1) * L):
            u = u + rad[..., s, :]
        y = (u[..., 0] + u[..., 1]) + u[..., 2]
        t = t + y
        q = q + y * y
    return np.stack([t, q], -1)


def pass_plan(spp, L, per_pass):
    """[(first, count)] of a job cut into passes of per_pass samples (a multiple of L)."""
    assert per_pass % L == 0 and per_pass > 0
    return [(f, min(per_pass, spp - f)) for f in range(0, spp, per_pass)]


def centre_rays(cam, lens):
    """crt_lens_centre_rays_async: (h * w, 6), record row * w + col, no draws. PINHOLE:
    crt_render_features_async's ray; every other kind lens_rays' expressions with fx = col + 0.5 and
    fy = row_in_face + 0.5 (the jitter terms left out, not added as zeros)."""
    w, h = cam.image_w, cam.image_h
    out = np.empty((h * w, 6), np.float64)
    if lens.kind == lm.PINHOLE:
        O, P0 = list(cam.origin), list(cam.pixel00)
        DX, DY = list(cam.pixel_delta_x), list(cam.pixel_delta_y)
        for row in range(h):
            for col in range(w):
                centre = [(P0[k] + DY[k] * float(row)) + DX[k] * float(col) for k in range(3)]
                out[row * w + col] = O + [centre[k] - O[k] for k in range(3)]
        return out
    for row in range(h):
        h_face, face, rf = lm.face_rows(lens, w, h, row)
        for col in range(w):
            fx, fy = float(col) + 0.5, float(rf) + 0.5
            a, b = fx * (2.0 / float(w)) - 1.0, 1.0 - fy * (2.0 / float(h_face))
            o, d = lm.direction(lens, a, b, face)
            out[row * w + col, :3] = o
            out[row * w + col, 3:] = d
    return out


# ---- the adaptive scenario of tests/test_lens_pass_model.py and tests/test_gpu_lens_passes.py ------
# cornell, 64 spp in passes of 8. "equirect": 33 x 9 from the scene camera's own position, outside the
# box: 9 blocks, the edge ones 1 column wide and 1 row high; most of the panorama is the empty
# background (no variance: those blocks stop at the first eligible pass, 8 samples), the blocks on the
# box are noisy. "cube": 5 x 30 from inside the box (test_gpu_lens.INSIDE_CORNELL): 8 blocks of 5 x 4
# (the last 5 x 2); the last block looks out of the open front (background only), the one before it is
# a row of the back wall and three of background, the others are walls.
# The thresholds come from the blocks' ratios sum se / sum m under this model on the oracle's radiance
# (tests/test_lens_pass_model.py prints them). equirect: the four blocks on the box have 0.0027, 0.0051,
# 0.0044, 0.0099 after 8 samples and 0.0012, 0.0041, 0.0023, 0.0099 after 64; 0.0022 lies between the
# first block's 0.0027 (16 samples) and 0.0019 (24), under everything the second and fourth ever
# reach, and above the background's 7e-9. cube: the mixed block has 0.102 after 24 samples and 0.079
# after 32, the walls never less than 0.112: 0.09.
SCEN_SPP, SCEN_PASS = 64, 8
SCEN_FRAMES = {"equirect": (33, 9), "cube": (5, 30)}
SCEN_INSIDE = {"equirect": False, "cube": True}
SCEN_THRESHOLD = {"equirect": 0.0022, "cube": 0.09}


def check_mix(steps, per_pass=SCEN_PASS):
    """The scenario is a real mix: a block stops at the first eligible pass, one never stops, and two
    stop at different counts. Returns (counts, stopped) for the message."""
    counts, stopped = stop_counts(steps)
    spp = int(counts.max())
    assert (stopped & (counts == per_pass)).any(), (counts, stopped)
    assert (~stopped).any() and (counts[~stopped] == spp).all(), (counts, stopped)
    assert len(set(counts[stopped].tolist())) >= 2, (counts, stopped)
    return counts, stopped


def run_adaptive(rad, per_pass, threshold, min_samples=0):
    """The masked passes and updates of a job over rad (h, w, spp, 3), the radiance of every sample of
    every pixel (a sample's radiance does not depend on which blocks are active). Returns the list of
    (first, count, state after the pass and the update (copies), active blocks)."""
    h, w, spp = rad.shape[:3]
    L = pm.chunk_len(spp)
    st = fresh_state(w, h, blocks=True)
    out = []
    for first, count in pass_plan(spp, L, per_pass):
        lens_pass(st, rad[:, :, first:first + count], first, L)
        st["words"], active = pm.block_update(st["noise"], st["words"], w, h, first + count, spp, threshold, min_samples)
        out.append((first, count, {k: np.array(v) for k, v in st.items()}, active))
        if active == 0:
            break
    return out


def stop_counts(steps):
    """Every block's final count, and whether it stopped, from run_adaptive's steps."""
    words = steps[-1][2]["words"]
    return words & np.uint32(STOPPED - 1), (words & np.uint32(STOPPED)) != 0
