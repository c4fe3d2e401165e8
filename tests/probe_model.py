"""A numpy restatement of the probe bake's own stages (include/crt_render.h, crt_probes_async): the
generator of crt_probe_rays_async over the package's sample_seed / rand_double, the spherical-harmonic
basis, the lane-strided tree reduction and crt_sh_eval_async. What the device must write, computed
without a GPU, given the per-path radiance. Not a test module.

Python floats and numpy float64 arrays are IEEE doubles, np.sqrt is the IEEE square root and nothing
here is fused, so the values are the kernels' bits.
"""
import numpy as np

W_SPHERE, W_HEMISPHERE = 12.566370614359172, 3.141592653589793
A_IRRADIANCE = (3.141592653589793,) + (2.0943951023931953,) * 3 + (0.7853981633974483,) * 5
C0, C1, C2, C6, C8 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396


def unit_vector(crt, state):
    """Vec3D::random_unit_vector on an LCG state: (the state after the draws, [x, y, z])."""
    while True:
        state, x = crt.rand_double(state, -1.0, 1.0)
        state, y = crt.rand_double(state, -1.0, 1.0)
        state, z = crt.rand_double(state, -1.0, 1.0)
        if x * x + y * y + z * z < 1:
            break
    inv = 1 / float(np.sqrt(np.float64(x * x + y * y + z * z)))
    return state, [x * inv, y * inv, z * inv]


def rays(crt, points, normals, samples, base_seed=0, first_probe=0):
    """(rays (n * samples, 6) float64, states (n * samples,) uint32), record p * samples + s; normals
    None: SPHERE (d = u), else HEMISPHERE (d = N + u). Probe p is seeded as probe first_probe + p."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(points)
    out = np.empty((n * samples, 6), np.float64)
    states = np.empty(n * samples, np.uint32)
    for p in range(n):
        for s in range(samples):
            st, u = unit_vector(crt, crt.sample_seed(base_seed, first_probe + p, s))
            r = p * samples + s
            out[r, :3] = points[p]
            out[r, 3:] = u if normals is None else [float(normals[p][k]) + u[k] for k in range(3)]
            states[r] = st
    return out, states


def basis(d):
    """The nine basis functions at directions d (..., 3): (..., 9)."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full(x.shape, C0), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z),
                     C6 * ((3.0 * z) * z - 1.0), C2 * (x * z), C8 * (x * x - y * y)], -1)


def reduce_terms(terms, weight):
    """The fixed-order sum of terms (n, S, ...) over the S samples, times weight / S: lane l (0..63)
    adds the terms of samples l, l + 64, ... in order from 0.0, then the tree over steps 32 .. 1."""
    terms = np.asarray(terms, np.float64)
    n, S = terms.shape[:2]
    lanes = np.zeros((n, 64) + terms.shape[2:])
    for s0 in range(0, S, 64):
        c = min(64, S - s0)
        lanes[:, :c] = lanes[:, :c] + terms[:, s0:s0 + c]
    step = 32
    while step >= 1:
        lanes[:, :step] = lanes[:, :step] + lanes[:, step:2 * step]
        step //= 2
    return lanes[:, 0] * (weight / float(S))


def terms(dirs, L, samples, sphere):
    """The per-sample terms (n, S, K, 3): Y_k(d_s) * L_s[j], or L_s[j] itself (K = 1) for HEMISPHERE."""
    L = np.asarray(L, np.float64).reshape(-1, samples, 3)
    if not sphere:
        return L[:, :, None, :].copy()
    Y = basis(np.asarray(dirs, np.float64).reshape(-1, samples, 3))
    return Y[:, :, :, None] * L[:, :, None, :]


def reduce(dirs, L, samples, sphere):
    """crt_probes_async's coefficients (n, K, 3) from the generated directions (n * S, 3) and the
    per-path radiance (n * S, 3)."""
    return reduce_terms(terms(dirs, L, samples, sphere), W_SPHERE if sphere else W_HEMISPHERE)


def sh_eval(coeff, index, dirs, irradiance=False):
    """crt_sh_eval_async: (m, 3)."""
    coeff = np.asarray(coeff, np.float64).reshape(-1, 9, 3)
    index = np.asarray(index).astype(np.int64)
    Y = basis(dirs)
    ok = index < len(coeff)
    c = coeff[np.where(ok, index, 0)] if len(coeff) else np.zeros((len(index), 9, 3))
    out = np.zeros((len(index), 3))
    for k in range(9):
        a = A_IRRADIANCE[k] if irradiance else 1.0
        out = out + a * (c[:, k, :] * Y[:, k, None])
    out[~ok] = 0.0
    return out
