"""crt_denoise_async on synthetic guides and signals, with no render: frames with tiles whose whole
halo lies inside the frame (the LDS route's interior), hit and miss pixels interleaved at tap
distance, planes that face each other, hit pixels at t = 0, variances from 0 through denormals to
1e6, a zero-variance patch beside luminance steps (the tolerance D is DBL_MIN there and the colour
term overflows), a NaN colour, an infinite variance and a -0; 0, 7 and 10 normal squarings and up
to 8 iterations (step 128, past both frames). Colour and variance equal tests/denoise_model.py bit
for bit on the default route and with every step as gathers."""
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "tests"))
import denoise_model as dm  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 64
FRAMES = [(100, 40), (65, 17)]  # 4 x 5 tiles of 32 x 8 (columns 1, 2 and rows 1..3 are interior); one pixel past two tiles
PARAMS = [(8, 7, 1.0, 0.05), (1, 0, 1.0, 0.05), (5, 10, 4.0, 0.2), (3, 7, 1e-3, 1e-3)]
# normal, and two tangents spanning the plane, of the three planes: 1 and 2 face each other, 0 and 1 meet at 0.8
PLANES = [((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
          ((0.6, 0.0, 0.8), (0.8, 0.0, -0.6), (0.0, 1.0, 0.0)),
          ((-0.6, 0.0, -0.8), (0.8, 0.0, -0.6), (0.0, 1.0, 0.0))]


class Case:
    """Guide, signal and variance of a w x h frame, built once per frame and left unchanged."""

    def __init__(self, crt, w, h):
        rng = np.random.default_rng(w * 1000 + h)
        ys, xs = np.mgrid[0:h, 0:w]
        # ---- guide: three planes in diagonal bands, so taps cross a border both in x and in y
        region = ((xs + 2 * ys) // 11) % 3
        # the zero-variance patch (below) lies on one plane and has no miss and no t = 0 pixel
        py, px = slice(h // 2 - 4, h // 2 + 3), slice(w // 2 + 17, w // 2 + 31)
        region[py, px] = region[h // 2, w // 2 + 20]
        f = np.zeros((h, w), crt.FEATURE_DTYPE)
        for k, (n, u, v) in enumerate(PLANES):
            m = region == k
            f["prim"][m] = 10 + k
            f["normal"][m] = n
            f["point"][m] = (np.asarray(n) * (k + 1.0))[None, :] + 0.01 * xs[m][:, None] * np.asarray(u) + 0.01 * ys[m][:, None] * np.asarray(v)
            f["t"][m] = 5.0 + 0.01 * xs[m] + 0.003 * ys[m]
            f["material"][m] = k
        f["albedo"] = 0.5
        # checkerboards of miss pixels at periods 1, 2 and 4 in three zones
        self.miss = np.zeros((h, w), bool)
        zones = [(slice(1, h // 3), slice(2, w // 4), 1), (slice(h // 2, h - 1), slice(w // 3, 2 * w // 3 - 2), 2),
                 (slice(2, h - 3), slice(3 * w // 4 - 4, w - 1), 4)]
        for zy, zx, p in zones:
            self.miss[zy, zx] = ((xs[zy, zx] // p + ys[zy, zx] // p) % 2) == 0
        self.miss[py, px] = False
        # hit pixels at t = 0: bden = 0, the centre tap's b is 0 / 0, W is NaN and the pixel comes back unchanged
        self.t0 = np.zeros((h, w), bool)
        self.t0[rng.integers(0, h, 5), rng.integers(0, w, 5)] = True
        self.t0 &= ~self.miss
        self.t0[py, px] = False
        f["t"][self.t0] = 0.0
        for name in ("normal", "point", "t", "material"):
            f[name][self.miss] = 0
        f["prim"][self.miss] = -1
        # ---- signal: a ramp plus noise; variances 0, denormal, small, large
        scales = np.array([0.0, 5e-324, 2.0 ** -1060, 2.0 ** -1030, 1e-300, 1e-12, 1e-4, 1e-2, 1.0, 1e6])
        var = scales[rng.integers(0, len(scales), (h, w))] * rng.integers(1, 8, (h, w))
        rgb = (0.2 + 0.005 * xs + 0.01 * ys)[..., None] * np.array([1.0, 0.7, 0.4]) + \
            np.sqrt(np.minimum(var, 1e-2))[..., None] * rng.standard_normal((h, w, 3))
        # the zero-variance patch: columns in pairs, dark ones with channels (a, -a, 0) whose
        # luminance (a + -a) + 0 is exactly 0, so D = DBL_MIN away from the patch's rim, beside bright
        # ones of luminance 12: d * d / DBL_MIN overflows, the weight is 0
        var[py, px] = 0.0
        a = rng.integers(1, 1024, (h, w)) / 1024.0
        dark = np.stack([a, -a, np.zeros((h, w))], -1)
        self.dark = np.zeros((h, w), bool)
        self.dark[py, px] = (xs[py, px] // 2) % 2 == 0
        bright = np.zeros((h, w), bool)
        bright[py, px] = ~self.dark[py, px]
        rgb[self.dark] = dark[self.dark]
        self.inner = np.zeros((h, w), bool)  # the dark pixels off the rim: their 3 x 3 variance mean is 0
        self.inner[py.start + 1:py.stop - 1, px.start + 1:px.stop - 1] = self.dark[py.start + 1:py.stop - 1, px.start + 1:px.stop - 1]
        rgb[bright] = 4.0
        # one NaN colour, one infinite variance, one -0 colour, away from each other
        self.nan_at, self.inf_at, self.negzero_at = (h // 4, w // 2 - 3), (3 * h // 4, w // 2 - 9), (h // 2 + 1, 7)
        rgb[self.nan_at + (1,)] = NAN
        var[self.inf_at] = np.inf
        rgb[self.negzero_at + (2,)] = -0.0
        for a in (f, rgb, var):
            a.setflags(write=False)
        self.w, self.h, self.feat, self.rgb, self.var, self.region = w, h, f, rgb, var, region
        self.model = {}

    def want(self, prm):
        if prm not in self.model:
            self.model[prm] = dm.denoise(self.rgb, self.var, self.feat, *prm)
        return self.model[prm]


@pytest.fixture(scope="module", params=FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def case(crt, request):
    return Case(crt, *request.param)


def gpu_denoise(crt, c, prm):
    """Colour and variance of crt_denoise_async; inputs have NaN records past their end, outputs are
    NaN-filled and have sentinels past theirs."""
    import torch
    n = c.w * c.h

    def dev(a, per):
        return torch.from_numpy(np.concatenate([a.reshape(-1), np.full(PAD * per, NAN)])).cuda()

    rgb, var = dev(c.rgb, 3), dev(c.var, 1)
    feat = torch.from_numpy(np.concatenate([np.ascontiguousarray(c.feat).view(np.uint8).reshape(-1),
                                            np.full(PAD * 88, 0xFF, np.uint8)])).cuda()
    out = torch.full(((n + PAD) * 3,), NAN, dtype=torch.float64, device="cuda")
    vout = torch.full((n + PAD,), NAN, dtype=torch.float64, device="cuda")
    out[n * 3:] = 123.0
    vout[n:] = 123.0
    crt.denoise(0, c.w, c.h, rgb.data_ptr(), var.data_ptr(), feat.data_ptr(), crt.denoise_params(*prm), out.data_ptr(),
                vout.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, vout = out.cpu().numpy(), vout.cpu().numpy()
    assert (out[n * 3:] == 123.0).all() and (vout[n:] == 123.0).all()
    return out[:n * 3].reshape(c.h, c.w, 3), vout[:n].reshape(c.h, c.w)


def same_bits(a, b):
    return np.array_equal(dm.bits(a), dm.bits(b))


def test_the_inputs_hold_what_they_claim(case):
    c = case
    f, hit = c.feat, ~c.miss
    assert (f["prim"][c.miss] == -1).all() and (f["prim"][hit] >= 10).all() and c.miss.sum() > 50
    # hit pixels with a miss at tap distance 1, 2, 4 and 8 in x, and the other way round
    for step in (1, 2, 4, 8):
        a, b = c.miss[:, :-step], c.miss[:, step:]
        assert (a & ~b).any() and (~a & b).any(), step
    # the planes: unit-ish normals, 1 and 2 face each other, every pair is adjacent somewhere
    n = [np.asarray(p[0]) for p in PLANES]
    assert n[1] @ n[2] < 0 and n[0] @ n[2] < 0 < n[0] @ n[1] < 1
    pairs = {(int(a), int(b)) for a, b in zip(c.region[:, :-1].ravel(), c.region[:, 1:].ravel()) if a != b}
    assert {(0, 1), (1, 2), (2, 0)} <= pairs
    assert c.t0.any() and (f["t"][c.t0] == 0).all() and (f["prim"][c.t0] >= 0).all()
    v = c.var
    denormal = (v > 0) & (v < dm.DBL_MIN)
    assert (v == 0).any() and denormal.sum() > c.w * c.h // 10 and (v >= 1e6).any() and np.isinf(v).sum() == 1
    # the patch: luminance exactly 0 with distinct colours, zero variance around it, steps of 12 beside it
    y = (c.rgb[..., 0] + c.rgb[..., 1]) + c.rgb[..., 2]
    assert c.dark.sum() >= 40 and (y[c.dark] == 0).all() and len(np.unique(c.rgb[c.dark][:, 0])) > 20
    assert c.inner.sum() >= 20 and len({int(k) for k in c.region[c.dark]}) == 1 and not c.miss[c.dark].any()
    vbar = sum(np.roll(np.roll(c.var, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    assert (vbar[c.inner] == 0).all()
    assert (c.var[c.dark] == 0).all()
    with np.errstate(over="ignore"):
        assert np.isinf((12.0 * 12.0) / (0.0 + (1e-6 * 0.0 + dm.DBL_MIN)))
    assert np.isnan(c.rgb).sum() == 1 and np.signbit(c.rgb[c.negzero_at + (2,)]) and c.rgb[c.negzero_at + (2,)] == 0
    # interior tiles: the 32 x 8 tiles whose step-2 halo (4 pixels) is inside the frame
    interior = [(tx, ty) for tx in range(-(-c.w // 32)) for ty in range(-(-c.h // 8))
                if tx * 32 >= 4 and tx * 32 + 36 <= c.w and ty * 8 >= 4 and ty * 8 + 12 <= c.h]
    print(f"{c.w} x {c.h}: {-(-c.w // 32) * -(-c.h // 8)} tiles, {len(interior)} interior, {int(c.miss.sum())} miss pixels, "
          f"{int(denormal.sum())} denormal variances, {int(c.dark.sum())} dark patch pixels")
    assert len(interior) == (6 if (c.w, c.h) == (100, 40) else 0)


@pytest.mark.parametrize("prm", PARAMS, ids=lambda p: f"it{p[0]}_sq{p[1]}")
@pytest.mark.parametrize("route", ["default", "gather"])
def test_filter_equals_the_model_on_synthetic_state(crt, monkeypatch, case, route, prm):
    c = case
    if route == "gather":
        monkeypatch.setenv("CRT_DENOISE_ROUTE", "gather")
    want_c, want_v = c.want(prm)
    got_c, got_v = gpu_denoise(crt, c, prm)
    bad = ~np.isfinite(got_c).all(-1)
    diff = dm.bits(got_c) != dm.bits(want_c)
    print(f"{c.w} x {c.h} {prm} {route}: {int(diff.sum())} colour words differ, first at {np.argwhere(diff)[:4].tolist()}")
    assert same_bits(got_c, want_c) and same_bits(got_v, want_v)
    assert bad[c.nan_at] and bad.sum() == 1                # the injected NaN is the only non-finite colour
    assert not same_bits(got_c, c.rgb)                     # it filtered
    # hit pixels at t = 0 and the infinite-variance pixel come back unchanged
    assert same_bits(got_c[c.t0], c.rgb[c.t0]) and same_bits(got_v[c.t0], c.var[c.t0])
    assert same_bits(got_c[c.inf_at], c.rgb[c.inf_at]) and np.isinf(got_v[c.inf_at])
    # every dark pixel off the patch's rim was filtered: copied through would mean that W was not > 0,
    # as it is when D = 0 (the centre tap's a is then 0 / 0)
    assert (dm.bits(got_c[c.inner]) != dm.bits(c.rgb[c.inner])).any(-1).all()
