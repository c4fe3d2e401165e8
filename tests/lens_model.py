"""A numpy and Python-float restatement of the lens render's generator (include/crt_render.h,
crt_lens_rays_async) over the package's sample_seed / rand_double: what the device must write,
computed without a GPU. The reduction is radiance_model.frame_from_samples, crt_render_async's own.
Not a test module.

Python floats are IEEE doubles, math.sqrt is the IEEE square root and nothing here is fused, so the
values are the kernel's bits for PINHOLE, ORTHOGRAPHIC and CUBE. EQUIRECT and FISHEYE go through
math.sin / math.cos (libm), which the device library's functions match only to a few ulp.
"""
import math

import numpy as np

import radiance_model as rm

PINHOLE, ORTHOGRAPHIC, EQUIRECT, FISHEYE, CUBE = range(5)
frame = rm.frame_from_samples

# face -> the local direction (x, y, z) from (u, v), v pointing down the image
CUBE_FACES = (
    lambda u, v: (1.0, -v, -u),   # +X
    lambda u, v: (-1.0, -v, u),   # -X
    lambda u, v: (u, 1.0, v),     # +Y
    lambda u, v: (u, -1.0, -v),   # -Y
    lambda u, v: (u, -v, 1.0),    # +Z
    lambda u, v: (-u, -v, -1.0),  # -Z
)


def face_rows(lens, w, h, row):
    """(h_face, face, row_in_face) of frame row `row`."""
    if lens.kind == CUBE:
        return w, row // w, row % w
    return h, 0, row


def direction(lens, a, b, face=0):
    """(origin, direction) of the point (a, b) of the frame (of `face` for CUBE), lists of 3 floats."""
    R, U, F, O = list(lens.right), list(lens.up), list(lens.forward), list(lens.origin)
    ex, ey = lens.extent_x, lens.extent_y
    if lens.kind == ORTHOGRAPHIC:
        ax, by = a * ex, b * ey
        return [(O[k] + R[k] * ax) + U[k] * by for k in range(3)], F
    if lens.kind == EQUIRECT:
        phi, theta = a * ex, b * ey
        ct, st = math.cos(theta), math.sin(theta)
        x, y, z = ct * math.sin(phi), st, ct * math.cos(phi)
    elif lens.kind == FISHEYE:
        px, py = a * ex, b * ey
        psi = math.sqrt(px * px + py * py)
        k = 1.0 if psi == 0 else math.sin(psi) / psi
        x, y, z = px * k, py * k, math.cos(psi)
    elif lens.kind == CUBE:
        x, y, z = CUBE_FACES[face](a, -b)
    else:
        raise ValueError("direction: not for PINHOLE")
    return O, [(R[k] * x + U[k] * y) + F[k] * z for k in range(3)]


def pixel_ab(w, h_face, col, row_in_face, ux=0.0, uy=0.0):
    fx = (float(col) + 0.5) + ux
    fy = (float(row_in_face) + 0.5) + uy
    return fx * (2.0 / float(w)) - 1.0, 1.0 - fy * (2.0 / float(h_face))


def pinhole_rays(crt, cam, first_sample, num_samples):
    """PINHOLE as the header states it (start_path): the defocus loop, the two jitter draws, then
    centre = (p00 + pdy * row) + pdx * col, sample = (centre + pdx * ux) + pdy * uy, d = sample - o."""
    w, h = cam.image_w, cam.image_h
    O, P0 = list(cam.origin), list(cam.pixel00)
    DX, DY = list(cam.pixel_delta_x), list(cam.pixel_delta_y)
    KX, KY = list(cam.defocus_disk_x), list(cam.defocus_disk_y)
    out = []
    states = []
    for pixel in range(w * h):
        row, col = divmod(pixel, w)
        for s in range(first_sample, first_sample + num_samples):
            rng = crt.sample_seed(cam.base_seed, pixel, s)
            o = O
            if cam.defocus_angle > 0:
                while True:
                    rng, vx = crt.rand_double(rng, -1.0, 1.0)
                    rng, vy = crt.rand_double(rng, -1.0, 1.0)
                    if vx * vx + vy * vy + 0.0 * 0.0 < 1:
                        break
                o = [(O[k] + KX[k] * vx) + KY[k] * vy for k in range(3)]
            rng, uy = crt.rand_double(rng, -0.5, 0.5)
            rng, ux = crt.rand_double(rng, -0.5, 0.5)
            d = []
            for k in range(3):
                centre = (P0[k] + DY[k] * float(row)) + DX[k] * float(col)
                d.append(((centre + DX[k] * ux) + DY[k] * uy) - o[k])
            out.append(list(o) + d)
            states.append(rng)
    return np.array(out, np.float64).reshape(-1, 6), np.array(states, np.uint32)


def lens_rays(crt, cam, lens, first_sample=0, num_samples=None, jitter=True):
    """(rays (n, 6) float64, states (n,) uint32) in crt_lens_rays_async's record order: record
    (row * w + col) * num_samples + (s - first_sample). jitter=False replaces the two draws' values
    by 0 (the states still advance): the pixel centres."""
    if num_samples is None:
        num_samples = cam.samples_per_pixel - first_sample
    if lens.kind == PINHOLE:
        return pinhole_rays(crt, cam, first_sample, num_samples)
    w, h = cam.image_w, cam.image_h
    n = w * h * num_samples
    rays = np.empty((n, 6), np.float64)
    states = np.empty(n, np.uint32)
    r = 0
    for row in range(h):
        h_face, face, rf = face_rows(lens, w, h, row)
        for col in range(w):
            for s in range(first_sample, first_sample + num_samples):
                rng = crt.sample_seed(cam.base_seed, row * w + col, s)
                rng, uy = crt.rand_double(rng, -0.5, 0.5)
                rng, ux = crt.rand_double(rng, -0.5, 0.5)
                if not jitter:
                    ux = uy = 0.0
                a, b = pixel_ab(w, h_face, col, rf, ux, uy)
                o, d = direction(lens, a, b, face)
                rays[r, :3] = o
                rays[r, 3:] = d
                states[r] = rng
                r += 1
    return rays, states
