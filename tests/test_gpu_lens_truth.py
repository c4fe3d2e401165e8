"""The lens kernels (crt_lens_rays_async, crt_lens_centre_rays_async, crt_render_lens_async) and sh_eval_kernel on
the GPU, held to truth that is no restatement of them (tests/lens_truth.py, tests/test_sh_truth.py).
tests/test_gpu_lens.py holds the same kernels to the model bit for bit; here the device's own records are carried
back into the frame by the inverse of each projection, and whole frames of one lit sphere are held to the share of
each pixel that the sphere covers.

  1. rays      every device record lies in its own pixel (and face) within 1e-9 pixel and at its own two draws, for
               every kind and extent of tests/test_lens_truth.py, make_lens's basis and a sheared one, frames 9 x 7,
               1 x 1, 8 x 1 and 64 x 32 (CUBE 3 x 18, 1 x 6, 16 x 96), first_sample 0 and 3; the centre rays are the
               pixel centres; the same exclusions (11 records of the full panorama's 64 x 32 frames) and the same 1 % cap. The jitter of 2^16 device
               records is uniform and uncorrelated (SEED = 7100, tests/test_lens_truth.py's). In the sheared worlds
               every ray of a certainly covered pixel meets the sphere and none of an untouched one does.
  2. points    the centre ray of an odd FISHEYE frame (psi == 0, the k = 1 branch) and EQUIRECT frame is forward,
               bit for bit, sheared or not. FISHEYE with extent_x = extent_y = pi / sqrt(2) rounded down until
               extent_x^2 + extent_y^2 <= pi^2: the frame's corners are at psi = pi, and the corner pixels' centres at
               psi = pi (1 - 1 / w): their rays are finite and that angle from forward within 1e-9 rad, on 3 x 3
               (pi / 3 from -forward) and 255 x 255 (pi / 255 from it).
  3. frames    render_lens of each world of lens_truth at max_depth 2, spp 1024, 32 x 16 (CUBE 8 x 48): +0 bit for bit
               where the sphere certainly is not, Le bit for bit where it certainly is, and elsewhere within
               5 sqrt(p (1 - p) / spp) + |coverage_g - coverage_g/2| of Le p (p clipped to [0, 1]); batch_pixels = 7
               and plain=True give the same bits; ORTHOGRAPHIC's frame sum is Le pi r^2 w h / (4 ex ey) within five
               standard errors. Every pixel is Le k / 1024 for a whole k: Le = (4, 2, 1) keeps every sum exact.
  4. sh_eval   tests/test_sh_truth.py's comparison with the clamped-cosine integrals on the kernel's output
  5. bake      a SPHERE bake at max_depth 1 under env_truth's `random` world (the point, S and seed of
               tests/test_gpu_env_truth.py), evaluated with irradiance=True at 64 normals, is sum_k I_k(n) m_k within
               5 sum_k |I_k(n)| se_k: I_k the clamped-cosine integrals by quadrature, m_k and se_k from
               env_truth.sphere_moments. The distance to the true irradiance pi sum L F(n) is printed: the band limit's.

Measured on an MI355X: see DESIGN 6p. The largest call is 2^19 paths. Outputs are pre-filled with 0xFF bytes and
followed by a sentinel tail (test_gpu_lens.render; the ray buffers here likewise)."""
import contextlib
import math

import numpy as np
import pytest

import env_truth as et
import lens_truth as lt
import test_gpu_env_nee as tgn
import test_lens_truth as tlt
import test_sh_truth as tst
from test_gpu_env_truth import PROBE_SEED
from test_gpu_lens import render, same, with_batch

pytestmark = pytest.mark.gpu
TAIL = 64
SPP = tlt.SPP
NORMAL_SEED = 7400   # the 64 normals of the bake's evaluation: the first and only seed tried


@contextlib.contextmanager
def opened(crt, d):
    s = crt.GpuScene(d)
    try:
        s.upload(0)
        yield s
        assert s.guard(0) == 0
    finally:
        s.close()


@pytest.fixture(scope="module")
def scene(crt):
    with opened(crt, lt.world(crt, "ortho").d) as s:
        yield s


def black(cam):
    from cpp_raytracer_amd import _capi
    cam.background = _capi.D3(*lt.BG)
    return cam


def device_rays(crt, cam, lens, first, count):
    """crt_lens_rays_async into buffers pre-filled with 0xFF and followed by a sentinel tail: (n, 6) float64."""
    import ctypes as C
    import torch
    n = cam.image_w * cam.image_h * count
    rays = torch.full((n * 48 + TAIL,), 0xFF, dtype=torch.uint8, device="cuda")
    states = torch.full((n * 4 + TAIL,), 0xFF, dtype=torch.uint8, device="cuda")
    crt.check(crt.lib().crt_lens_rays_async(0, C.byref(cam), C.byref(lens), first, count, C.c_void_p(rays.data_ptr()),
                                            C.c_void_p(states.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "crt_lens_rays_async")
    torch.cuda.synchronize()
    r, s = rays.cpu().numpy(), states.cpu().numpy()
    assert (r[n * 48:] == 0xFF).all() and (s[n * 4:] == 0xFF).all(), "the call wrote past its records"
    return r[:n * 48].copy().view(np.float64).reshape(n, 6)


def centre_rays(scene, cam, lens):
    import torch
    rays = scene.lens_centre_rays(cam, lens)
    torch.cuda.synchronize()
    return rays.cpu().numpy()


# ---- 1. the kernel's own rays ----------------------------------------------------------------------------
@pytest.mark.parametrize("shear", [False, True], ids=["orthonormal", "sheared"])
@pytest.mark.parametrize("kind,ex,ey", tlt.CASES)
def test_every_device_record_comes_from_its_own_pixel(crt, scene, kind, ex, ey, shear):
    lens = lt.make(crt, kind, ex, ey)
    if shear:
        lens = lt.sheared(lens)
    worst = left_out = 0
    for w, h, count in [(3, 18, 8), (1, 6, 8), (16, 96, 4)] if kind == "cube" else [(9, 7, 8), (1, 1, 8), (8, 1, 8), (64, 32, 4)]:
        for first in (0, 3):
            cam = tlt.camera(crt, w, h, first + count)
            rays = device_rays(crt, cam, lens, first, count)
            assert np.isfinite(rays).all()
            ux, uy, keep = tlt.recovered(lens, w, h, count, rays)
            wx, wy = tlt.draws(crt, cam, first, count)
            err = max(float(np.abs(ux - wx)[keep].max()), float(np.abs(uy - wy)[keep].max()))
            assert err <= lt.SLACK, (w, h, first, err)
            worst, left_out = max(worst, err), left_out + int((~keep).sum())
        cx, cy, keep = tlt.recovered(lens, w, h, 1, centre_rays(scene, cam, lens))
        err = max(float(np.abs(cx[keep]).max()), float(np.abs(cy[keep]).max()))
        assert err <= lt.SLACK, (w, h, "centre", err)
        worst, left_out = max(worst, err), left_out + int((~keep).sum())
    print(f"{kind} ({ex}, {ey}) sheared={shear}: {left_out} records left out, largest |u - draw| = {worst:.3g} pixels")


@pytest.mark.parametrize("kind,ex,ey", [("fisheye", 0.0, 0.0), ("equirect", 1.0, 0.4)])
def test_device_jitter_is_uniform_and_independent(crt, kind, ex, ey):
    lens = lt.make(crt, kind, ex, ey)
    w, h, spp = 64, 32, 32
    rays = device_rays(crt, tlt.camera(crt, w, h, spp), lens, 0, spp)
    ux, uy, keep = tlt.recovered(lens, w, h, spp, rays)
    assert keep.all() and len(ux) == 1 << 16
    tlt.check_jitter(ux, uy)


def meets(wd, rays):
    """Whether each ray (n, 6), as a half-line, meets the world's sphere."""
    o, d = rays[:, :3], rays[:, 3:]
    oc = np.array(wd.centre) - o
    t = (oc * d).sum(1) / (d * d).sum(1)
    off = oc - t[:, None] * d
    return (t > 0) & ((off * off).sum(1) < wd.radius ** 2)


@pytest.mark.parametrize("name", [n for n in lt.WORLDS if n != "ortho"])
def test_sheared_rays_meet_the_sphere_where_it_certainly_is(crt, name):
    """The sheared variants have no jacobian, but they have a rim: the certain masks need the inverse alone."""
    wd = lt.world(crt, name, shear=True)
    inside, outside = lt.certain(wd.lens, wd.w, wd.h, wd.centre, wd.radius)
    assert inside.any() and outside.any() and (inside.sum() + outside.sum()) >= 0.8 * inside.size
    count = 4
    rays = device_rays(crt, tlt.camera(crt, wd.w, wd.h, count), wd.lens, 0, count)
    hit = meets(wd, rays).reshape(wd.h, wd.w, count)
    print(f"{name} sheared: certainly covered {inside.sum()}, untouched {outside.sum()} of {inside.size}")
    assert hit[inside].all() and not hit[outside].any()


# ---- 2. exact points -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fisheye", "equirect"])
def test_the_centre_of_an_odd_frame_is_forward(crt, scene, kind):
    for shear in (False, True):
        lens = lt.make(crt, kind)
        if shear:
            lens = lt.sheared(lens)
        w, h = 7, 5
        rays = centre_rays(scene, tlt.camera(crt, w, h, 1), lens)
        F = np.array(list(lens.forward))
        assert (F != 0).all()
        assert same(rays[2 * w + 3, 3:], F), (kind, shear)
        assert same(rays[2 * w + 3, :3], np.array(list(lens.origin)))


def widest_fisheye():
    e = math.pi / math.sqrt(2.0)
    while e * e + e * e > math.pi * math.pi:
        e = math.nextafter(e, 0.0)
    return e


@pytest.mark.parametrize("w", [3, 255])
def test_fisheye_corner_pixels_near_the_point_behind(crt, scene, w):
    """The frame's corners are psi = pi; a corner pixel's centre is at a = b = +-(1 - 1 / w), psi = pi (1 - 1 / w):
    no pixel centre reaches pi itself under the header's rule on the extents."""
    e = widest_fisheye()
    assert math.pi * math.pi - 2 * e * e < 1e-14
    lens = lt.make(crt, "fisheye", e, e)
    rays = centre_rays(scene, tlt.camera(crt, w, w, 1), lens).reshape(w, w, 6)
    B = lt.basis(lens)
    for row, col in ((0, 0), (0, w - 1), (w - 1, 0), (w - 1, w - 1)):
        d = rays[row, col, 3:]
        assert np.isfinite(rays[row, col]).all()
        q = B.T @ d
        behind = math.atan2(math.hypot(q[0], q[1]), -q[2])   # the angle from -forward
        assert abs(behind - math.pi / w) <= 1e-9, (row, col, behind)
        assert (q[0] > 0) == (col > 0) and (q[1] > 0) == (row == 0)   # right of forward on the right, above it on top
        assert abs(float(d @ d) - 1) <= 1e-12


# ---- 3. frames against coverage --------------------------------------------------------------------------
def differing(a, b, most=8):
    """The first pixels at which two frames differ: (row, col, hits of a, hits of b), hits out of SPP."""
    at = np.argwhere((a.view(np.uint64) != b.view(np.uint64)).any(2))
    return len(at), [(int(r), int(c), float(a[r, c, 0] * SPP / lt.LE[0]), float(b[r, c, 0] * SPP / lt.LE[0])) for r, c in at[:most]]


@pytest.mark.parametrize("name", list(lt.WORLDS))
def test_a_frame_of_one_lit_sphere_is_its_coverage(crt, name):
    wd = lt.world(crt, name)
    p, p2, inside, outside = lt.truth(name)
    noise = 5 * math.sqrt(0.25 / SPP)
    assert np.abs(p - p2).max() <= noise / 10   # the quadrature's own error is a tenth of the noise at p = 0.5
    share = (inside.sum() + outside.sum()) / p.size
    assert inside.any() and outside.any() and share >= tlt.SHARE
    cam = black(tlt.camera(crt, wd.w, wd.h, SPP))
    assert cam.max_depth == 2 and SPP * wd.w * wd.h <= 1 << 21
    with opened(crt, wd.d) as s:
        got = render(s, cam, wd.lens)
        for label, lens in (("batch_pixels = 7", with_batch(wd.lens, 7)), ("plain", with_batch(wd.lens, 7, plain=True))):
            other = render(s, cam, lens)
            assert same(other, got), (label, differing(got, other))
    Le = np.array(lt.LE)
    assert (got.view(np.uint64)[outside] == 0).all(), "a pixel the sphere cannot reach is not +0"
    assert same(got[inside], np.broadcast_to(Le, got[inside].shape)), "a pixel the sphere fills is not Le"
    k = got[:, :, 0] * (SPP / Le[0])
    assert (k == np.round(k)).all() and same(got, k[:, :, None] * (Le / SPP)[None, None, :])  # whole counts, every channel
    pc, pc2 = np.clip(p, 0.0, 1.0), np.clip(p2, 0.0, 1.0)
    tol = 5 * np.sqrt(pc * (1 - pc) / SPP) + np.abs(pc - pc2)
    frac = k / SPP
    doubtful = ~(inside | outside)
    z = (frac - pc)[doubtful] / np.maximum(np.sqrt(pc * (1 - pc) / SPP)[doubtful], 1e-300)
    print(f"{name}: {int(doubtful.sum())} doubtful pixels, certain share {share:.3f}, largest |share - p| / tolerance = "
          f"{float((np.abs(frac - pc) / np.maximum(tol, 1e-300))[doubtful].max()):.3g}, largest |z| = {float(np.abs(z[np.isfinite(z)]).max()):.3g}")
    assert (np.abs(frac - pc) <= tol).all()
    if name == "ortho":
        want = math.pi * wd.radius ** 2 * wd.w * wd.h / (4 * wd.lens.extent_x * wd.lens.extent_y)
        se = math.sqrt(float((pc * (1 - pc))[doubtful].sum()) / SPP)
        print(f"ortho: the frame's share sum {frac.sum():.6f} against {want:.6f}, z = {(frac.sum() - want) / se:.3g}")
        assert abs(frac.sum() - want) <= 5 * se
        assert same(got.sum((0, 1)), Le * frac.sum())


# ---- 4. sh_eval_kernel -----------------------------------------------------------------------------------
def device_sh_eval(crt):
    def run(coeff, index, dirs, irradiance):
        import torch
        out = crt.sh_eval(torch.from_numpy(np.ascontiguousarray(coeff, np.float64)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(dirs, np.float64)).cuda(), irradiance=irradiance)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    return run


def test_the_kernels_irradiance_is_the_clamped_cosine_integral(crt):
    tst.check(device_sh_eval(crt), "kernel: ")


# ---- 5. bake, then evaluate ------------------------------------------------------------------------------
def test_a_baked_probes_irradiance_is_the_band_limited_fields(crt):
    import torch
    w = et.world(crt, "random")
    log2s = et.PROBE_LOG2_S["sphere"]
    m, sd = et.sphere_moments(w.env)
    se = sd / math.sqrt(1 << log2s)
    n = tst.normals(64, NORMAL_SEED)
    I = tst.clamped_cosine_integrals(n)   # (64, 9)
    with opened(crt, w.d) as s:
        P = torch.tensor([(200.0, 0.0, 0.0)], dtype=torch.float64, device="cuda")
        coeff = s.probes(P, None, samples=1 << log2s, mode="sphere", max_depth=1, background=et.BG, t_min=et.T_MIN,
                         base_seed=PROBE_SEED, env=tgn.device_env(crt, w.env, w.basis))
        got = crt.sh_eval(coeff, torch.zeros(len(n), dtype=torch.int32, device="cuda"), torch.from_numpy(n).cuda(), irradiance=True)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
    want = I @ m
    tol = 5 * (np.abs(I) @ se)
    true = math.pi * np.array([(w.env.texels * et.factors(w.env, tuple(nn.tolist()))[:, :, None]).sum((0, 1)) for nn in n[:8]])
    print(f"bake then evaluate: largest |got - want| / tolerance = {float((np.abs(got - want) / tol).max()):.3g}; the band limit's error "
          f"at the first 8 normals, relative to pi sum L F: {float((np.abs(want[:8] - true) / true).max()):.3g}")
    assert got.shape == (64, 3) and (np.abs(got - want) <= tol).all()
