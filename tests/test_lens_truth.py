"""tests/lens_truth.py held on its own, and tests/lens_model.py held to it, without a GPU. The truth is
the inverse of each projection; the model is the header's text. What agrees here is a meaning, not a restatement.

  1. round trip   every record of lens_model.lens_rays, carried back into the frame by lens_truth.inverse, lies in
                  its own pixel (and face) within SLACK = 1e-9 pixel, and the position inside the pixel is the
                  record's own two draws: the second along the row, the first down the column. With make_lens's
                  basis and with a scaled, sheared one. Records that the truth's own conditioning marks (an
                  EQUIRECT latitude within 1e-3 of a pole, a FISHEYE angle within 1e-3 of pi) are left out, counted,
                  printed and capped at 1 % of a case.
  2. jitter       the recovered (ux, uy) of 2^16 records are uniform on [-1/2, 1/2] and uncorrelated, five standard
                  errors each. SEED = 7100, the first and only one tried.
  3. jacobians    integrate to 4 pi (EQUIRECT), 4 pi / 6 (a CUBE face) and the equidistant square's solid angle
                  2 pi - 8 * integral over [0, pi / 4] of cos(e / cos(phi)) (FISHEYE), tolerance the difference of
                  two midpoint grids
  4. coverage     sums to pi r^2 / (ex ey) of (a, b) area (ORTHOGRAPHIC) and to the area of the cone's section by
                  the face's plane (CUBE, one face) and, for the EQUIRECT and FISHEYE worlds, to the cone's (a, b) area by a
                  Gauss-Legendre rule, within the difference from the grid of half the size; and agrees, pixel
                  by pixel, with the model's forward map on a sub-pixel grid. The certain masks hold no pixel that
                  the sub-pixel grid contradicts, and hold SHARE of every frame.
  5. mutations    each listed change to a copy of the model's text fails the check named beside it
"""
import math
import types
from pathlib import Path

import numpy as np
import pytest

import lens_model as lm
import lens_truth as lt

SEED = 7100
SHARE = 0.9   # of a world's frame is certain, and both certain sets are non-empty
SPP = 1024    # the GPU frames' samples: the quadrature's error is held against their noise
CASES = [("orthographic", 0.0, 0.0), ("equirect", 0.0, 0.0), ("fisheye", 0.0, 0.0), ("cube", 0.0, 0.0),
         ("equirect", 1.0, 0.4), ("fisheye", 2.2, 2.2), ("fisheye", 0.3, 0.2)]
FRAMES = [(9, 7), (1, 1), (1, 5), (8, 1)]
CUBE_FRAMES = [(3, 18), (1, 6)]


_SETTINGS = []


def camera(crt, w, h, spp, seed=SEED):
    """A resolved camera of w x h at spp samples and max_depth 2; the lens kinds here read nothing else of it."""
    from cpp_raytracer_amd import camera_with
    if not _SETTINGS:
        _SETTINGS.append(crt.SceneData.named("cornell").camera)
    return crt.resolve_camera(camera_with(_SETTINGS[0], image_w=w, image_h=h, samples_per_pixel=spp, max_depth=2), seed)


def draws(crt, cam, first, count):
    """(ux, uy) of every record in record order, from the generator's contract: the state is sample_seed(base,
    pixel, s), the first draw is the one down the column, the second the one along the row."""
    ux, uy = [], []
    for pixel in range(cam.image_w * cam.image_h):
        for s in range(first, first + count):
            st = crt.sample_seed(cam.base_seed, pixel, s)
            st, v = crt.rand_double(st, -0.5, 0.5)
            st, u = crt.rand_double(st, -0.5, 0.5)
            ux.append(u)
            uy.append(v)
    return np.array(ux), np.array(uy)


def recovered(lens, w, h, count, rays):
    """(ux, uy, kept) of records in lens_rays' order: where inverse puts each inside its own pixel; asserts the
    containment and the exclusion cap."""
    hf = lt.h_face(lens, w, h)
    r = np.arange(len(rays)) // count
    row, col = r // w, r % w
    bad = lt.conditioning(lens, rays[:, 3:])
    assert bad.sum() <= 0.01 * len(rays), (int(bad.sum()), len(rays))
    a, b, face = lt.inverse(lens, rays[:, :3], rays[:, 3:])
    fx, fy = lt.frame_xy(w, hf, a, b)
    keep = ~bad
    assert (face[keep] == (row // hf)[keep]).all(), "a record is on another face than its row's"
    ux, uy = fx - col - 0.5, fy - row % hf - 0.5
    worst = max(float(np.abs(ux[keep]).max()), float(np.abs(uy[keep]).max())) - 0.5
    assert worst <= lt.SLACK, f"a record lies {worst:.3g} pixels outside its own pixel"
    return ux, uy, keep


def check_round_trip(crt, model, kind, ex, ey, w, h, shear, first=0, count=8, jitter=True):
    lens = lt.make(crt, kind, ex, ey)
    if shear:
        lens = lt.sheared(lens)
    cam = camera(crt, w, h, first + count)
    rays, _ = model.lens_rays(crt, cam, lens, first, count, jitter=jitter)
    ux, uy, keep = recovered(lens, w, h, count, rays)
    wx, wy = draws(crt, cam, first, count) if jitter else (np.zeros(len(rays)), np.zeros(len(rays)))
    err = max(float(np.abs(ux - wx)[keep].max()), float(np.abs(uy - wy)[keep].max()))
    assert err <= lt.SLACK, f"the place in the pixel is not the record's own draws: {err:.3g} pixels"
    return int((~keep).sum()), err


def check_jitter(ux, uy):
    """Uniform on [-1/2, 1/2]: mean 0, variance 1 / 12, fourth moment 1 / 80; independent: correlation 0."""
    n = len(ux)
    z = []
    for u in (ux, uy):
        z.append(u.mean() / math.sqrt(1 / (12 * n)))
        z.append(((u * u).mean() - 1 / 12) / math.sqrt((1 / 80 - 1 / 144) / n))
    z.append(float(np.corrcoef(ux, uy)[0, 1]) * math.sqrt(n))
    print("z of mean ux, var ux, mean uy, var uy, correlation:", np.round(z, 2).tolist())
    assert (np.abs(z) <= 5).all(), z
    return z


def model_jitter(crt, model, kind, ex, ey):
    lens = lt.make(crt, kind, ex, ey)
    w, h, spp = 64, 32, 32
    rays, _ = model.lens_rays(crt, camera(crt, w, h, spp), lens)
    ux, uy, keep = recovered(lens, w, h, spp, rays)
    assert keep.all() and len(ux) == 1 << 16
    return ux, uy


# ---- 1. round trip ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shear", [False, True], ids=["orthonormal", "sheared"])
@pytest.mark.parametrize("kind,ex,ey", CASES)
def test_every_record_comes_from_its_own_pixel(crt, kind, ex, ey, shear):
    for w, h in CUBE_FRAMES if kind == "cube" else FRAMES:
        left_out, err = check_round_trip(crt, lm, kind, ex, ey, w, h, shear)
        print(f"{kind} ({ex}, {ey}) {w} x {h} sheared={shear}: {left_out} records left out, largest |u - draw| = {err:.3g} pixels")


@pytest.mark.parametrize("kind", ["orthographic", "equirect", "fisheye", "cube"])
def test_centre_records_are_pixel_centres(crt, kind):
    w, h = (3, 18) if kind == "cube" else (9, 7)
    for shear in (False, True):
        check_round_trip(crt, lm, kind, 0.0, 0.0, w, h, shear, count=1, jitter=False)


def test_the_exclusions_are_the_truths_own(crt):
    """conditioning reads the ray alone: the poles of a panorama and the point behind a fisheye, nothing else."""
    l = crt.make_lens("equirect", forward=(0.0, 0.0, 1.0))   # right = -x, up = y
    d = np.array([[0.0, 1.0, 0.0], [0.0, math.cos(2e-3), math.sin(2e-3)], [0.0, -1.0, 1e-4], [1.0, 0.0, 0.0]])
    assert lt.conditioning(l, d).tolist() == [True, False, True, False]
    f = crt.make_lens("fisheye", forward=(0.0, 0.0, 1.0))
    d = np.array([[0.0, 0.0, -1.0], [1e-4, 0.0, -1.0], [2e-3, 0.0, -1.0], [0.0, 0.0, 1.0]])
    assert lt.conditioning(f, d).tolist() == [True, True, False, False]
    assert not lt.conditioning(crt.make_lens("cube"), d).any()


def test_the_inverse_at_points_anyone_can_name(crt):
    """Looking along +z with up = y, right is -x (right-handed with forward = -z of the viewer's frame). A ray to
    the right of forward is in the right half of a panorama and of a fisheye frame, one above it in the upper
    half; on a fisheye a ray 0.5 rad off the axis is 0.5 / extent from the centre, whatever its azimuth."""
    for kind in ("equirect", "fisheye"):
        l = crt.make_lens(kind, forward=(0.0, 0.0, 1.0))
        R, U, F, O = (np.array(list(v)) for v in (l.right, l.up, l.forward, l.origin))
        assert R.tolist() == [-1.0, 0.0, 0.0] and U.tolist() == [0.0, 1.0, 0.0]
        a, b, _ = lt.inverse(l, O, F * math.cos(0.5) + R * math.sin(0.5))
        assert a[0] > 0 and abs(b[0]) < 1e-12 and abs(a[0] * l.extent_x - 0.5) < 1e-12
        a, b, _ = lt.inverse(l, O, F * math.cos(0.5) + U * math.sin(0.5))
        assert b[0] > 0 and abs(a[0]) < 1e-12 and abs(b[0] * l.extent_y - 0.5) < 1e-12
        fx, fy = lt.frame_xy(8, 4, a, b)
        assert abs(fx[0] - 4.0) < 1e-12 and fy[0] < 2.0   # up is towards row 0
    f = crt.make_lens("fisheye", forward=(0.0, 0.0, 1.0), extent_x=1.0, extent_y=1.0)
    for az in (0.3, 2.0, 4.4):
        d = np.array([-math.sin(0.5) * math.cos(az), math.sin(0.5) * math.sin(az), math.cos(0.5)])
        a, b, _ = lt.inverse(f, (0.0, 0.0, 0.0), d)
        assert abs(math.hypot(a[0], b[0]) - 0.5) < 1e-12 and abs(math.atan2(b[0], a[0]) % (2 * math.pi) - az) < 1e-12
    c = crt.make_lens("cube", forward=(0.0, 0.0, 1.0))
    # the usual layout: on +Z (face 4) right is along the row and up towards row 0; +X is the face to the right
    a, b, face = lt.inverse(c, (0.0, 0.0, 0.0), np.array([[-0.5, 0.25, 1.0], [-1.0, 0.0, 0.2], [0.0, 2.0, 0.2]]))
    assert face.tolist() == [4, 0, 2] and (a[0], b[0]) == (0.5, 0.25)


# ---- 2. jitter -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ex,ey", [("fisheye", 0.0, 0.0), ("equirect", 1.0, 0.4)])
def test_jitter_is_uniform_and_independent(crt, kind, ex, ey):
    check_jitter(*model_jitter(crt, lm, kind, ex, ey))


# ---- 3. jacobians ----------------------------------------------------------------------------------------
def jacobian_integral(lens, n):
    t = -1.0 + (np.arange(n) + 0.5) * (2.0 / n)
    a, b = np.meshgrid(t, t, indexing="ij")
    return float(lt.jacobian(lens, a, b).sum() * (2.0 / n) ** 2)


def fisheye_square(e):
    """The solid angle of the square |px|, |py| <= e of an equidistant fisheye, e <= pi / sqrt(2): in polar
    coordinates (psi, phi) about the axis the square reaches psi = e / cos(phi) for |phi| <= pi / 4, eight times
    over, and d omega = sin(psi) d psi d phi: 2 pi - 8 * integral over [0, pi / 4] of cos(e / cos(phi))."""
    x, wgt = np.polynomial.legendre.leggauss(64)
    phi = (x + 1) * (math.pi / 8)
    return 2 * math.pi - 8 * float((wgt * np.cos(e / np.cos(phi))).sum() * (math.pi / 8))


@pytest.mark.parametrize("kind,e", [("equirect", 0.0), ("cube", 0.0), ("fisheye", math.pi / 2), ("fisheye", 0.7), ("fisheye", 2.2)])
def test_jacobians_integrate_to_the_projections_solid_angles(crt, kind, e):
    lens = lt.make(crt, kind, e, e)
    want = {"equirect": 4 * math.pi, "cube": 4 * math.pi / 6}.get(kind) or fisheye_square(e)
    coarse, fine = jacobian_integral(lens, 256), jacobian_integral(lens, 512)
    print(f"{kind} {e}: {fine} against {want}, the grids differ by {abs(fine - coarse):.3g}")
    assert abs(fine - want) <= abs(fine - coarse) and abs(fine - coarse) <= 1e-4 * want


def test_the_fisheye_squares_solid_angle(crt):
    """The one-dimensional form against a grid finer than the test above uses, and at a size with a closed form
    of its own: a square that the circle psi = pi just holds is not needed; a small one tends to 4 e^2."""
    lens = lt.make(crt, "fisheye", 1.3, 1.3)
    fine, finer = jacobian_integral(lens, 1024), jacobian_integral(lens, 2048)
    assert abs(finer - fisheye_square(1.3)) <= abs(finer - fine)
    assert abs(fisheye_square(1e-3) / 4e-6 - 1) < 1e-6


# ---- 4. coverage -----------------------------------------------------------------------------------------
def model_share(crt, wd, row, col, n):
    """The share of an n x n sub-pixel grid of pixel (row, col) whose ray, by the model's forward map, meets the
    world's sphere."""
    hf, face, rf = lm.face_rows(wd.lens, wd.w, wd.h, row)
    c, hits = np.array(wd.centre), 0
    for i in range(n):
        for j in range(n):
            a, b = lm.pixel_ab(wd.w, hf, col, rf, (i + 0.5) / n - 0.5, (j + 0.5) / n - 0.5)
            o, d = (np.array(v) for v in lm.direction(wd.lens, a, b, face))
            oc = c - o
            t = float(oc @ d) / float(d @ d)
            hits += t > 0 and float((oc - t * d) @ (oc - t * d)) < wd.radius ** 2
    return hits / (n * n)


@pytest.mark.parametrize("name", list(lt.WORLDS))
def test_coverage_and_certainty_of_each_world(crt, name):
    wd = lt.world(crt, name)
    p, p2, inside, outside = lt.truth(name)
    err = np.abs(p - p2)
    noise = 5 * math.sqrt(0.25 / SPP)
    share = (inside.sum() + outside.sum()) / p.size
    print(f"{name}: sum {p.sum():.6f}, largest |coverage_g - coverage_g/2| = {err.max():.3g} (a tenth of the noise at p = 0.5: "
          f"{noise / 10:.3g}), certainly covered {inside.sum()}, untouched {outside.sum()} of {p.size} ({share:.3f})")
    assert err.max() <= noise / 10
    assert inside.any() and outside.any() and share >= SHARE
    # a covered pixel is 1 to the accuracy asked of the quadrature; no node lands in an untouched pixel
    assert np.abs(p[inside] - 1).max() <= noise / 10 and (p[outside] == 0).all()
    if name in ("seam", "pole", "fisheye"):
        # the frame holds the whole image: the sum is the cone's (a, b) area, by a rule that shares nothing with the
        # grid (Gauss-Legendre, 192 x 192); the grid's own error is a third of its difference from the half grid.
        # `corner` has no such value: 1 / jacobian has kinks along the cube's edges and the rule does not converge
        pixel = 4.0 / (wd.w * lt.h_face(wd.lens, wd.w, wd.h))
        want = lt.cone_area(wd.lens, wd.centre, wd.radius, 192)
        print(f"{name}: the cone's (a, b) area {p.sum() * pixel!r} against {want!r}, the grids differ by {abs(p.sum() - p2.sum()) * pixel:.3g}")
        assert abs(p.sum() * pixel - want) <= abs(p.sum() - p2.sum()) * pixel
    if name == "ortho":
        want = math.pi * wd.radius ** 2 / (4 * wd.lens.extent_x * wd.lens.extent_y) * wd.w * wd.h
        assert abs(p.sum() - want) <= 1e-12 * want
    # the model's forward map, pixel by pixel: every doubtful pixel, and every eighth certain one
    doubtful = ~(inside | outside)
    n = 16
    worst = 0.0
    for row, col in zip(*np.nonzero(doubtful)):
        worst = max(worst, abs(model_share(crt, wd, row, col, n) - min(p[row, col], 1.0)))
    # a smooth rim crosses at most about 2 n of the n^2 cells, each worth 1 / n^2
    print(f"{name}: {int(doubtful.sum())} doubtful pixels, largest |model's share - coverage| = {worst:.3g}")
    assert worst <= 2 / n
    for k, (row, col) in enumerate(zip(*np.nonzero(~doubtful))):
        if k % 8 == 0:
            assert model_share(crt, wd, row, col, 4) == (1.0 if inside[row, col] else 0.0), (row, col)


def test_coverage_on_one_cube_face_is_the_cones_section(crt):
    """A cone of half-angle alpha whose axis is theta off a face's normal cuts the face's plane (at distance 1,
    where (a, b) are lengths) in an ellipse: with the normal along z and the axis (sin theta, 0, cos theta), (x sin theta + cos theta)^2 =
    cos^2(alpha) (x^2 + y^2 + 1) has semi-axes sin(alpha) cos(alpha) / A and sin(alpha) / sqrt(A), A = cos^2(alpha) - sin^2(theta):
    the area is pi sin^2(alpha) cos(alpha) / A^1.5."""
    lens = lt.make(crt, "cube")
    c = np.array([0.2, -0.3, 1.0]) * 4.0   # on +Z
    centre, radius = np.array(lt.ORIGIN) + lt.basis(lens) @ c, 1.0
    sa = radius / math.sqrt(float(c @ c))
    ct = c[2] / math.sqrt(float(c @ c))
    ca = math.sqrt(1 - sa * sa)
    want = math.pi * sa * sa * ca / (ca * ca - (1 - ct * ct)) ** 1.5
    p, p2 = lt.coverage(lens, 8, 48, centre, radius, 512)
    got, got2 = p.sum() * 4 / 64, p2.sum() * 4 / 64
    print(f"one face: {got} and {got2} against {want}")
    assert (p[:32] == 0).all() and (p[40:] == 0).all()
    assert abs(got - want) <= max(abs(got - got2), 1e-9 * want)


# ---- 5. mutations ----------------------------------------------------------------------------------------
UNIT = "\n\ndef _unit(v):\n    v = list(v)\n    n = math.sqrt(sum(c * c for c in v))\n    return [c / n for c in v]\n"
MUTATIONS = {
    "equirect x negated": ("x, y, z = ct * math.sin(phi), st,", "x, y, z = -(ct * math.sin(phi)), st,", "round trip"),
    "fisheye y negated": ("x, y, z = px * k, py * k,", "x, y, z = px * k, -(py * k),", "round trip"),
    "fisheye x and y swapped": ("x, y, z = px * k, py * k,", "x, y, z = py * k, px * k,", "round trip"),
    "fisheye equisolid": ("else math.sin(psi) / psi", "else 2.0 * math.sin(psi / 2.0) / psi", "round trip"),
    # the same with directions of unit length, as a lens that really were equisolid (r = 2 sin(angle / 2)) would give
    "fisheye equisolid, unit length": ("        x, y, z = px * k, py * k, math.cos(psi)",
                                       "        q = 2.0 * math.asin(min(1.0, psi / 2.0))\n        k = 1.0 if psi == 0 else math.sin(q) / psi\n"
                                       "        x, y, z = px * k, py * k, math.cos(q)", "round trip"),
    "equirect theta by extent_x": ("phi, theta = a * ex, b * ey", "phi, theta = a * ex, b * ex", "round trip"),
    "ux and uy swapped": ("    fx = (float(col) + 0.5) + ux\n    fy = (float(row_in_face) + 0.5) + uy",
                          "    fx = (float(col) + 0.5) + uy\n    fy = (float(row_in_face) + 0.5) + ux", "round trip"),
    "uy for both": ("    fx = (float(col) + 0.5) + ux", "    fx = (float(col) + 0.5) + uy", "jitter"),
    "orthographic a and b swapped": ("ax, by = a * ex, b * ey", "ax, by = b * ex, a * ey", "round trip"),
    "basis normalised": ("R, U, F, O = list(lens.right), list(lens.up), list(lens.forward), list(lens.origin)",
                         "R, U, F, O = _unit(lens.right), _unit(lens.up), _unit(lens.forward), list(lens.origin)", "sheared round trip"),
}


def mutant(name):
    old, new, _ = MUTATIONS[name]
    src = Path(lm.__file__).read_text()
    assert src.count(old) == 1, name
    mod = types.ModuleType("lens_model_mutant")
    exec(compile(src.replace(old, new) + UNIT, "lens_model_mutant", "exec"), mod.__dict__)
    return mod


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_each_mutation_of_the_model_is_caught(crt, name):
    """The check named in MUTATIONS, the one the tests above run on the model itself, fails on the mutant. The
    kind is the mutation's own; the frame 9 x 7 at the default extents (ORTHOGRAPHIC (3, 1.5))."""
    m = mutant(name)
    kind = name.split()[0] if name.split()[0] in lt.KIND else "fisheye"
    check_round_trip(crt, lm, kind, 0.0, 0.0, 9, 7, name == "basis normalised")   # the model itself passes
    with pytest.raises(AssertionError):
        if MUTATIONS[name][2] == "jitter":
            check_jitter(*model_jitter(crt, m, kind, 0.0, 0.0))
        else:
            check_round_trip(crt, m, kind, 0.0, 0.0, 9, 7, name == "basis normalised")
    if name == "uy for both":   # the round trip catches it as well, through the draws
        with pytest.raises(AssertionError, match="own draws"):
            check_round_trip(crt, m, kind, 0.0, 0.0, 9, 7, False)
    if name == "ux and uy swapped":   # every sample is still inside its pixel: only the draws tell
        with pytest.raises(AssertionError, match="own draws"):
            check_round_trip(crt, m, kind, 0.0, 0.0, 9, 7, False)
