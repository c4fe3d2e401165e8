"""A numpy restatement of the render kernel's start_path (random_ray_through_pixel, camera.h:184-200,
with the defocus disk of :160-168), over the package's sample_seed / rand_double: what
crt_camera_rays_async must write, computed without a GPU. Not a test module.

Per record, in the kernel's order: the defocus rejection loop (pairs of draws over (-1, 1) until
vx*vx + vy*vy + 0*0 < 1), the two jitter draws over (-0.5, 0.5) with the pixel_delta_y one first (a
g++ build of the reference evaluates it first), then per axis
  centre = (p00 + pdy * row) + pdx * col,  sample = (centre + pdx * ux) + pdy * uy,  d = sample - o.
Python floats are IEEE doubles and nothing here is fused, so the values are the kernel's bits.
"""
import numpy as np


def owned_rows(cam, tiling):
    if tiling is None:
        return list(range(cam.image_h))
    return [r for r in range(cam.image_h) if (r // tiling.row_block) % tiling.tile_count == tiling.tile_index]


def camera_rays(crt, cam, first_sample=0, num_samples=None, tiling=None):
    """(rays (n, 6) float64, states (n,) uint32) in crt_camera_rays_async's record order: owned pixel
    j (owned rows in order, packed), sample s -> record j * num_samples + (s - first_sample)."""
    if num_samples is None:
        num_samples = cam.samples_per_pixel - first_sample
    o0, p00 = list(cam.origin), list(cam.pixel00)
    pdx, pdy = list(cam.pixel_delta_x), list(cam.pixel_delta_y)
    ddx, ddy = list(cam.defocus_disk_x), list(cam.defocus_disk_y)
    rows = owned_rows(cam, tiling)
    n = len(rows) * cam.image_w * num_samples
    rays = np.empty((n, 6), np.float64)
    states = np.empty(n, np.uint32)
    r = 0
    for row in rows:
        fr = float(row)
        for col in range(cam.image_w):
            fc = float(col)
            centre = [(p00[k] + pdy[k] * fr) + pdx[k] * fc for k in range(3)]
            for s in range(first_sample, first_sample + num_samples):
                rng = crt.sample_seed(cam.base_seed, row * cam.image_w + col, s)
                if cam.defocus_angle <= 0:
                    o = o0
                else:
                    while True:
                        rng, vx = crt.rand_double(rng, -1.0, 1.0)
                        rng, vy = crt.rand_double(rng, -1.0, 1.0)
                        if vx * vx + vy * vy + 0.0 * 0.0 < 1:
                            break
                    o = [(o0[k] + ddx[k] * vx) + ddy[k] * vy for k in range(3)]
                rng, uy = crt.rand_double(rng, -0.5, 0.5)
                rng, ux = crt.rand_double(rng, -0.5, 0.5)
                for k in range(3):
                    sample = (centre[k] + pdx[k] * ux) + pdy[k] * uy
                    rays[r, k] = o[k]
                    rays[r, 3 + k] = sample - o[k]
                states[r] = rng
                r += 1
    return rays, states


def frame_from_samples(smp, chunk):
    """crt_render_async's frame from per-sample radiance smp (..., spp, 3): per chunk of `chunk`
    samples the sum in sample order from 0, the chunk sums added in order, times 1 / spp."""
    spp = smp.shape[-2]
    total = None
    for c0 in range(0, spp, chunk):
        u = np.zeros(smp.shape[:-2] + (3,))
        for s in range(c0, min(spp, c0 + chunk)):
            u = u + smp[..., s, :]
        total = u if total is None else total + u
    return total * (1 / float(spp))
