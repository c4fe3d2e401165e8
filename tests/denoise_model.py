"""numpy restatement of the denoiser's specification in include/crt_render.h (crt_pixel_variance_async,
crt_denoise_async, the centre rays of crt_render_features_async): the same IEEE f64 operations in the
same order, a whole frame at a time, so the GPU results are compared with == (tests/test_gpu_denoise.py)
and the restatement is checked on its own (tests/test_denoise_model.py). Not a test module."""
import numpy as np

DBL_MIN = float(np.finfo(np.float64).tiny)
G3 = (0.25, 0.5, 0.25)
H5 = (1.0 / 16, 0.25, 3.0 / 8, 0.25, 1.0 / 16)
CRT_DIELECTRIC = 3


def bits(a):
    """The array's f64 bit patterns: equality of these is equality bit for bit (NaNs, zero signs)."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def centre_rays(cam):
    """(h, w, 6) rays of crt_render_features_async: origin, then per component
    d = ((pixel00 + pixel_delta_y * row) + pixel_delta_x * col) - origin."""
    h, w = int(cam.image_h), int(cam.image_w)
    row = np.arange(h, dtype=np.float64)[:, None] * np.ones((1, w))
    col = np.arange(w, dtype=np.float64)[None, :] * np.ones((h, 1))
    rays = np.zeros((h, w, 6))
    for k in range(3):
        center = (cam.pixel00[k] + cam.pixel_delta_y[k] * row) + cam.pixel_delta_x[k] * col
        rays[..., k] = cam.origin[k]
        rays[..., 3 + k] = center - cam.origin[k]
    return rays


def features_from_hits(hits, materials, background, dtype):
    """crt_feature records (dtype = FEATURE_DTYPE) from closest-hit records of the centre rays."""
    f = np.zeros(hits.shape, dtype)
    hit = hits["prim"] >= 0
    f["prim"] = np.where(hit, hits["prim"], -1)
    f["material"] = np.where(hit, hits["material"], 0)
    f["t"] = np.where(hit, hits["t"], 0.0)
    f["normal"] = np.where(hit[..., None], hits["normal"], 0.0)
    f["point"] = np.where(hit[..., None], hits["point"], 0.0)
    mat = materials[np.where(hit, hits["material"], 0)]
    albedo = np.where((mat["kind"] == CRT_DIELECTRIC)[..., None], 1.0, mat["color"])
    f["albedo"] = np.where(hit[..., None], albedo, np.asarray(background, np.float64))
    return f


def pixel_variance(noise, n, L):
    """crt_pixel_variance_async: noise (h, w, 2) = t, q; n = samples per pixel (a number or an
    (h, w) array); L = the chunk length."""
    t, q = noise[..., 0], noise[..., 1]
    Ki = np.broadcast_to(np.asarray(n, np.int64), t.shape) // int(L)
    K, Lf = Ki.astype(np.float64), float(L)
    with np.errstate(all="ignore"):
        m = t / (K * Lf)
        var = q / (Lf * Lf) - K * m * m
        two = np.where(var > 0, var, 0.0) / (K * (K - 1))
        return np.where(Ki >= 2, two, np.where(Ki == 1, m * m, 0.0))


def block_counts_to_pixels(words, h, w):
    """Per-pixel sample counts from block words ((block rows, block columns) uint32)."""
    counts = (np.asarray(words, np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    return np.repeat(np.repeat(counts, 4, axis=0), 16, axis=1)[:h, :w]


def _tap(a, oy, ox, clamp=False):
    """a[y + oy, x + ox] for every pixel (coordinates clamped to the frame) and the mask of the
    pixels whose tap is inside the frame."""
    h, w = a.shape[:2]
    ys, xs = np.arange(h)[:, None] + oy, np.arange(w)[None, :] + ox
    inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    return a[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)], inside


def iterate(c, v, feat, step, squarings, sigma_l, sigma_p):
    """One iteration of crt_denoise_async: (c, v) -> (c', v')."""
    n, P, t, prim = feat["normal"], feat["point"], feat["t"], feat["prim"].astype(np.int64)
    with np.errstate(all="ignore"):
        vbar = np.zeros(v.shape)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, _ = _tap(v, dy, dx)
                vbar = vbar + (G3[dy + 1] * G3[dx + 1]) * vq
        yp = (c[..., 0] + c[..., 1]) + c[..., 2]
        D = (sigma_l * sigma_l) * vbar + (1e-6 * (yp * yp) + DBL_MIN)
        bden = (sigma_p * sigma_p) * (t * t)
        W, V, C = np.zeros(v.shape), np.zeros(v.shape), np.zeros(c.shape)
        geo = prim >= 0
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                cq, inside = _tap(c, step * dy, step * dx)
                vq, _ = _tap(v, step * dy, step * dx)
                nq, _ = _tap(n, step * dy, step * dx)
                Pq, _ = _tap(P, step * dy, step * dx)
                primq, _ = _tap(prim, step * dy, step * dx)
                use = inside & np.isfinite(cq).all(-1) & np.isfinite(vq) & ((prim < 0) == (primq < 0))
                nd = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                N = np.where(nd > 0, nd, 0.0)
                for _ in range(squarings):
                    N = N * N
                e0, e1, e2 = (Pq[..., k] - P[..., k] for k in range(3))
                e = (e0 * n[..., 0] + e1 * n[..., 1]) + e2 * n[..., 2]
                b = (e * e) / bden
                N, b = np.where(geo, N, 1.0), np.where(geo, b, 0.0)
                d = ((cq[..., 0] + cq[..., 1]) + cq[..., 2]) - yp
                a = (d * d) / D
                wt = ((H5[dy + 2] * H5[dx + 2]) * N) / ((1 + a) * (1 + b))
                W = np.where(use, W + wt, W)
                C = np.where(use[..., None], C + wt[..., None] * cq, C)
                V = np.where(use, V + (wt * wt) * vq, V)
        ok = np.isfinite(c).all(-1) & np.isfinite(v) & (W > 0)
        c2 = np.where(ok[..., None], C / W[..., None], c)
        v2 = np.where(ok, V / (W * W), v)
    return c2, v2


def denoise(rgb, var, feat, iterations, squarings, sigma_l, sigma_p):
    """crt_denoise_async: rgb (h, w, 3), var (h, w), feat (h, w) FEATURE_DTYPE records."""
    c, v = np.array(rgb, np.float64), np.array(var, np.float64)
    for i in range(iterations):
        c, v = iterate(c, v, feat, 1 << i, squarings, float(sigma_l), float(sigma_p))
    return c, v


def noise_state(smp, L, n=None):
    """The t, q noise state (h, w, 2) and the running sums (h, w, 3) after the first n samples of
    per-sample radiances smp (h, w, spp, 3): chunk sums in sample order, y = (r + g) + b."""
    h, w, spp, _ = smp.shape
    n = spp if n is None else n
    t, q, total = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
    for c in range((n + L - 1) // L):
        S = np.zeros((h, w, 3))
        for i in range(c * L, min(n, (c + 1) * L)):
            S = S + smp[:, :, i]
        total = total + S
        if (c + 1) * L <= n:
            y = (S[..., 0] + S[..., 1]) + S[..., 2]
            t = t + y
            q = q + y * y
    return np.stack([t, q], -1), total


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))
