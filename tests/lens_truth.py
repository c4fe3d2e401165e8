"""Truth for the lens kinds that is never the forward map: the inverse of each projection, written
from the textbook meaning of the projection, its solid-angle jacobian, the share of a pixel that a sphere
covers, and the worlds these hold in. tests/test_lens_truth.py uses it without a GPU, tests/test_gpu_lens_truth.py
on one. Not a test module. Nothing here comes from lens_model's direction, CUBE_FACES or pixel_ab, and nothing
here maps a frame position to a ray.

  inverse    (a, b, face) of the frame position a ray (o, d) must have come from. The local coordinates are
             (x, y, z) = B^-1 d with B = [right | up | forward], a 3 x 3 solve: any basis that can be inverted.
               ORTHOGRAPHIC  B^-1 (o - origin), components 0 and 1 over the extents; d is forward
               EQUIRECT      longitude atan2(x, z), positive towards right; latitude asin(y / |xyz|), positive
                             towards up; each over its own extent
               FISHEYE       equidistant: psi = atan2(hypot(x, y), z) from the axis, position psi * (x, y) /
                             hypot(x, y), over the extents
               CUBE          the major axis picks the face, (sc, tc) from the usual cube-map table over |major|;
                             sc runs along the row, tc down the column
  frame_xy   fx = (a + 1) w / 2 along the row, fy = (1 - b) h_face / 2 down the column (of the face)
  jacobian   solid angle per unit (a, b) area, for an orthonormal basis: EQUIRECT ex ey cos(b ey), FISHEYE
             ex ey sin(psi) / psi, CUBE (1 + a^2 + b^2)^-1.5
  coverage   each pixel's share of its own (a, b) area whose rays meet a sphere: quadrature nodes on the cone the
             sphere subtends (equal solid angles, polar about the cone's axis), each worth d omega / jacobian
             of (a, b) area, binned by inverse; for ORTHOGRAPHIC equal-area nodes on the silhouette disk
  certain    the pixels that are certainly covered whole and certainly untouched: the rim of the cone (of the
             disk), sampled densely and carried into the frame by inverse, stays MARGIN pixels away from them

A World is one DiffuseLight sphere of Le = (4, 2, 1) under a black background, the lens outside it.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np

from light_truth import _scene

ORTHOGRAPHIC, EQUIRECT, FISHEYE, CUBE = 1, 2, 3, 4
KIND = {"orthographic": ORTHOGRAPHIC, "equirect": EQUIRECT, "fisheye": FISHEYE, "cube": CUBE}
LIGHT = 4
COLOR, PARAM = (1.0, 0.5, 0.25), 4.0
LE = (4.0, 2.0, 1.0)
BG = (0.0, 0.0, 0.0)
MARGIN = 0.05       # pixels: how far the rim must stay from a certain pixel
RIM = 1 << 16       # rim samples
SLACK = 1e-9        # pixels: what a record may lie outside its own pixel (a jitter draw of exactly -0.5, rounding)
POLE, ANTIPODE = 1e-3, 1e-3  # rad: EQUIRECT records nearer a pole, FISHEYE records nearer -forward are ill-conditioned

# the usual cube-map table: face -> (sc, tc) of (x, y, z), faces in the order +X -X +Y -Y +Z -Z
_SC_TC = (lambda x, y, z: (-z, -y), lambda x, y, z: (z, -y), lambda x, y, z: (x, z), lambda x, y, z: (x, -z),
          lambda x, y, z: (x, -y), lambda x, y, z: (-x, -y))


def _a(x):
    return np.asarray(x, np.float64)


def basis(lens):
    """B = [right | up | forward], columns."""
    return np.array([list(lens.right), list(lens.up), list(lens.forward)], np.float64).T


def h_face(lens, w, h):
    return w if lens.kind == CUBE else h


# ---- the inverse maps -----------------------------------------------------------------------------------
def local(lens, d):
    """(x, y, z) (n, 3) with d = right x + up y + forward z."""
    return np.linalg.solve(basis(lens), _a(d).reshape(-1, 3).T).T


def conditioning(lens, d):
    """(n,) bool: the records whose inverse is ill-conditioned, decided from the ray alone."""
    q = local(lens, d)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    if lens.kind == EQUIRECT:
        return np.abs(np.arctan2(y, np.hypot(x, z))) > math.pi / 2 - POLE
    if lens.kind == FISHEYE:
        return np.arctan2(np.hypot(x, y), z) > math.pi - ANTIPODE
    return np.zeros(len(q), bool)


def inverse(lens, o, d):
    """(a (n,), b (n,), face (n,) int) of rays o, d (n, 3)."""
    o, d = _a(o).reshape(-1, 3), _a(d).reshape(-1, 3)
    O = _a(list(lens.origin))
    face = np.zeros(len(d), np.int64)
    if lens.kind == ORTHOGRAPHIC:
        assert (d == _a(list(lens.forward))).all(), "an orthographic ray runs along forward"
        q = local(lens, o - O)
        assert np.abs(q[:, 2]).max() <= 1e-9 * (1 + np.abs(q).max()), "an orthographic ray starts in the lens's plane"
        return q[:, 0] / lens.extent_x, q[:, 1] / lens.extent_y, face
    assert (o == O).all(), "a ray of an angular lens starts at the origin"
    q = local(lens, d)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    if lens.kind == EQUIRECT:
        lon = np.arctan2(x, z)
        lat = np.arcsin(np.clip(y / np.sqrt(x * x + y * y + z * z), -1.0, 1.0))
        return lon / lens.extent_x, lat / lens.extent_y, face
    if lens.kind == FISHEYE:
        rho = np.hypot(x, y)
        psi = np.arctan2(rho, z)
        safe = np.where(rho > 0, rho, 1.0)
        return psi * (x / safe) / lens.extent_x, psi * (y / safe) / lens.extent_y, face
    assert lens.kind == CUBE
    m = np.abs(q)
    axis = np.argmax(m, 1)
    face = 2 * axis + (q[np.arange(len(q)), axis] < 0)
    ma = m[np.arange(len(q)), axis]
    sc, tc = np.empty(len(q)), np.empty(len(q))
    for f in range(6):
        k = face == f
        sc[k], tc[k] = _SC_TC[f](x[k], y[k], z[k])
    return sc / ma, -(tc / ma), face   # tc points down the image, b up


def frame_xy(w, hf, a, b):
    """(fx along the row, fy down the column of the face)."""
    return (a + 1.0) * (w / 2.0), (1.0 - b) * (hf / 2.0)


def jacobian(lens, a, b):
    """Solid angle per unit (a, b) area; an orthonormal basis is assumed."""
    a, b = _a(a), _a(b)
    ex, ey = lens.extent_x, lens.extent_y
    if lens.kind == EQUIRECT:
        return ex * ey * np.cos(b * ey) + 0.0 * a
    if lens.kind == FISHEYE:
        psi = np.hypot(a * ex, b * ey)
        return ex * ey * np.where(psi > 0, np.sin(psi) / np.where(psi > 0, psi, 1.0), 1.0)
    if lens.kind == CUBE:
        return (1.0 + a * a + b * b) ** -1.5
    raise ValueError("jacobian: angular kinds only")


def is_orthonormal(lens):
    B = basis(lens)
    return bool(np.abs(B.T @ B - np.eye(3)).max() <= 1e-12)


# ---- a sphere in the frame ------------------------------------------------------------------------------
def _frame_of(v):
    """Two unit vectors that complete unit v to an orthonormal frame."""
    e1 = np.cross(v, [1.0, 0.0, 0.0] if abs(v[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= math.sqrt(float(e1 @ e1))
    return e1, np.cross(v, e1)


def _cone(lens, centre, radius):
    """(unit axis, cos of the half-angle) of the cone a sphere subtends from the lens's origin."""
    to = _a(centre) - _a(list(lens.origin))
    dist = math.sqrt(float(to @ to))
    assert dist > radius > 0, "the lens is outside the sphere"
    return to / dist, math.sqrt(1.0 - (radius / dist) ** 2)


def _polar(radial, g):
    """The nodes of a polar grid, flat: g rings of g nodes each, ring i turned by the fraction frac(i * golden
    ratio) of a node's spacing, so that no radial line (a pixel's edge through the axis) meets every ring alike."""
    turn = np.modf(np.arange(g) * 0.6180339887498949)[0]
    phi = 2 * math.pi * ((np.arange(g) + 0.5)[None, :] + turn[:, None]) / g
    return np.repeat(radial, g), phi.reshape(-1)


def _bin(lens, w, h, a, b, face, weight):
    hf = h_face(lens, w, h)
    fx, fy = frame_xy(w, hf, a, b)
    col, row = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    ok = (col >= 0) & (col < w) & (row >= 0) & (row < hf)   # the rest of the sphere is outside the frame
    flat = (face[ok] * hf + row[ok]) * w + col[ok]
    return np.bincount(flat, weight[ok] if np.ndim(weight) else None, minlength=w * h)[:w * h].reshape(h, w)


def _nodes(lens, centre, radius, g):
    """(a, b, face, the solid angle or, for ORTHOGRAPHIC, the (right, up) area of a node) of g * g quadrature
    nodes inside the cone the sphere subtends (inside its silhouette's disk), by inverse."""
    O = _a(list(lens.origin))
    t = (np.arange(g) + 0.5) / g
    if lens.kind == ORTHOGRAPHIC:
        B = basis(lens)
        q = np.linalg.solve(B, _a(centre) - O)
        assert is_orthonormal(lens) and q[2] > radius, "the sphere is in front of the lens's plane"
        rr, phi = _polar(radius * np.sqrt(t), g)   # equal areas
        p = O[None, :] + np.outer(q[0] + rr * np.cos(phi), B[:, 0]) + np.outer(q[1] + rr * np.sin(phi), B[:, 1])
        return inverse(lens, p, np.broadcast_to(B[:, 2], p.shape)) + (math.pi * radius ** 2 / (g * g),)
    axis, c0 = _cone(lens, centre, radius)
    e1, e2 = _frame_of(axis)
    z, phi = _polar(c0 + (1 - c0) * t, g)   # equal solid angles
    s = np.sqrt(1 - z * z)
    d = np.outer(z, axis) + np.outer(s * np.cos(phi), e1) + np.outer(s * np.sin(phi), e2)
    return inverse(lens, np.broadcast_to(O, d.shape), d) + (2 * math.pi * (1 - c0) / (g * g),)


def _coverage(lens, w, h, centre, radius, g):
    assert is_orthonormal(lens), "the jacobian is defined for an orthonormal basis only"
    a, b, face, each = _nodes(lens, centre, radius, g)
    pixel = 4.0 / (w * h_face(lens, w, h))
    if lens.kind == ORTHOGRAPHIC:
        area = np.full(len(a), each / (lens.extent_x * lens.extent_y))   # of (a, b) a node
    else:
        area = each / jacobian(lens, a, b)
    return _bin(lens, w, h, a, b, face, area) / pixel


def cone_area(lens, centre, radius, n=96):
    """The (a, b) area of the whole cone, the integral of d omega / jacobian over it, by a rule that shares nothing
    with coverage's grid: Gauss-Legendre in cos(angle from the axis) times Gauss-Legendre in azimuth, n nodes each."""
    assert is_orthonormal(lens)
    axis, c0 = _cone(lens, centre, radius)
    e1, e2 = _frame_of(axis)
    x, wt = np.polynomial.legendre.leggauss(n)
    z, phi = (v.reshape(-1) for v in np.meshgrid(c0 + (1 - c0) * 0.5 * (x + 1), math.pi * (x + 1), indexing="ij"))
    wz, wp = (v.reshape(-1) for v in np.meshgrid(0.5 * (1 - c0) * wt, math.pi * wt, indexing="ij"))
    s = np.sqrt(1 - z * z)
    d = np.outer(z, axis) + np.outer(s * np.cos(phi), e1) + np.outer(s * np.sin(phi), e2)
    a, b, _ = inverse(lens, np.broadcast_to(_a(list(lens.origin)), d.shape), d)
    return float((wz * wp / jacobian(lens, a, b)).sum())


def coverage(lens, w, h, centre, radius, g):
    """((h, w) the covered share of each pixel's (a, b) area, the same from a grid of g / 2): their
    difference is the quadrature's own error."""
    return _coverage(lens, w, h, centre, radius, g), _coverage(lens, w, h, centre, radius, g // 2)


def rim(lens, w, h, centre, radius, m=RIM):
    """(fx, fy, face) of m points of the cone's rim (the silhouette's circle), by inverse."""
    O = _a(list(lens.origin))
    phi = 2 * math.pi * np.arange(m) / m
    if lens.kind == ORTHOGRAPHIC:
        B = basis(lens)
        q = B.T @ (_a(centre) - O)
        p = O[None, :] + np.outer(q[0] + radius * np.cos(phi), B[:, 0]) + np.outer(q[1] + radius * np.sin(phi), B[:, 1])
        a, b, face = inverse(lens, p, np.broadcast_to(B[:, 2], p.shape))
    else:
        axis, c0 = _cone(lens, centre, radius)
        e1, e2 = _frame_of(axis)
        s0 = math.sqrt(1 - c0 * c0)
        d = c0 * axis[None, :] + np.outer(s0 * np.cos(phi), e1) + np.outer(s0 * np.sin(phi), e2)
        a, b, face = inverse(lens, np.broadcast_to(O, d.shape), d)
    fx, fy = frame_xy(w, h_face(lens, w, h), a, b)
    return fx, fy, face


def certain(lens, w, h, centre, radius):
    """((h, w) bool certainly covered whole, (h, w) bool certainly untouched). A pixel is certain when no rim
    sample, carried into the frame by inverse, lies within MARGIN pixels of its rectangle; consecutive rim
    samples are at most MARGIN / 4 apart (asserted; the few pairs that step over the seam, an edge of the
    frame or of a cube face aside), so no stretch of the rim passes between them unseen. A certain pixel is
    all inside or all outside; it is inside when nodes of the cone's interior (256 x 256 of them, hundreds a
    pixel) land in it: that needs no jacobian, so any basis will do. A doubtful pixel is in neither mask."""
    hf = h_face(lens, w, h)
    fx, fy, face = rim(lens, w, h, centre, radius)
    dx, dy = np.diff(fx, append=fx[:1]), np.diff(fy, append=fy[:1])
    jump = (np.diff(face, append=face[:1]) != 0) | (np.abs(dx) > w / 2)
    # a step that leaves the frame need not be short: only what lies in or beside the frame matters
    inside = (fx > -1) & (fx < w + 1) & (fy > -1) & (fy < hf + 1)
    step = np.hypot(dx, dy)[~jump & inside & np.roll(inside, -1)]
    longest = float(step.max()) if len(step) else 0.0
    assert jump.sum() <= 16 and longest <= MARGIN / 4, (int(jump.sum()), longest)
    near = np.zeros((h, w), bool)
    reach = MARGIN + MARGIN / 4
    for ox in (-reach, 0.0, reach):
        for oy in (-reach, 0.0, reach):
            col, row = np.floor(fx + ox).astype(np.int64), np.floor(fy + oy).astype(np.int64)
            ok = (col >= 0) & (col < w) & (row >= 0) & (row < hf)
            near.reshape(-1)[(face[ok] * hf + row[ok]) * w + col[ok]] = True
    a, b, nface, _ = _nodes(lens, centre, radius, 256)
    hit = _bin(lens, w, h, a, b, nface, np.ones(len(a))) > 0
    return ~near & hit, ~near & ~hit


# ---- worlds ---------------------------------------------------------------------------------------------
ORIGIN, FORWARD, UP = (1.0, 2.0, 3.0), (0.3, -0.2, -1.0), (0.0, 1.0, 0.2)
SHEAR = ((1.5, 0.2, 0.0), (-0.1, 0.8, 0.3), (0.25, 0.0, 2.0))  # right', up', forward' in (right, up, forward)
ORTHO_EXTENTS = (3.0, 1.5)


def make(crt, kind, ex=0.0, ey=0.0, **kw):
    if kind == "orthographic" and ex == 0 and ey == 0:
        ex, ey = ORTHO_EXTENTS
    return crt.make_lens(kind, origin=ORIGIN, forward=FORWARD, up=UP, extent_x=ex, extent_y=ey, **kw)


def sheared(lens):
    """A copy of the lens (a raw Lens) with a scaled, sheared basis: no two vectors orthogonal, none of unit
    length. The library uses it as given."""
    from cpp_raytracer_amd import Lens, _capi
    B = basis(lens) @ _a(SHEAR).T
    l = Lens.from_buffer_copy(bytes(lens))
    l.right, l.up, l.forward = (_capi.D3(*B[:, k].tolist()) for k in range(3))
    return l


@dataclass
class World:
    name: str
    kind: str
    d: object       # SceneData: the one sphere
    lens: object
    centre: tuple
    radius: float
    w: int
    h: int


# name -> (kind, the centre in (right, up, forward) coordinates from the origin, radius, (ex, ey))
#   seam     directly behind: the sphere's image is cut in two by the panorama's left and right edges
#   pole     reaches up to latitude 1.46, within a row (pi / 16) of the upper pole, and does not hold it
#   fisheye  psi = 1.2 from the axis at azimuth 45 degrees: a mirroring in x, in y, or a swap of the two moves it
#            (the extents differ, so the swap moves it although it is on the diagonal of the local frame)
#   corner   about the (1, 1, 1) corner of the cube: +X, +Y and +Z each hold a part
#   ortho    off centre in both axes, whole inside the frame
_S = math.sin(1.2) * math.sqrt(0.5)
_POLE_LAT, _POLE_LON = 1.46 - math.asin(0.4), 0.6   # the centre of a cone of half-angle asin(1.6 / 4)
WORLDS = {
    "seam": ("equirect", (0.0, 0.5, -5.0), 2.0, (0.0, 0.0)),
    "pole": ("equirect", (4.0 * math.cos(_POLE_LAT) * math.sin(_POLE_LON), 4.0 * math.sin(_POLE_LAT),
                          4.0 * math.cos(_POLE_LAT) * math.cos(_POLE_LON)), 1.6, (0.0, 0.0)),
    "fisheye": ("fisheye", (4.0 * _S, 4.0 * _S, 4.0 * math.cos(1.2)), 1.4, (1.8, 1.5)),
    "corner": ("cube", (2.0, 2.0, 2.0), 1.8, (0.0, 0.0)),
    "ortho": ("orthographic", (1.1, -0.4, 6.0), 0.9, ORTHO_EXTENTS),
}
FRAME = {"equirect": (32, 16), "fisheye": (32, 16), "cube": (8, 48), "orthographic": (32, 16)}
G = 2048   # coverage's grid: tests/test_lens_truth.py holds its error to a tenth of the sampling noise


def world(crt, name, shear=False):
    kind, c, r, (ex, ey) = WORLDS[name]
    lens = make(crt, kind, ex, ey)
    if shear:   # the centre keeps its coordinates in the lens's own basis, and so its place in the frame
        lens = sheared(lens)
    centre = _a(ORIGIN) + basis(lens) @ _a(c)
    d = _scene(crt, [(LIGHT, COLOR, PARAM)], [(1, 0, tuple(centre.tolist()) + (r,))])
    w, h = FRAME[kind]
    return World(name, kind, d, lens, tuple(centre.tolist()), r, w, h)


@functools.lru_cache(maxsize=None)
def _truth(name):
    import cpp_raytracer_amd as crt
    wd = world(crt, name)
    p, p2 = coverage(wd.lens, wd.w, wd.h, wd.centre, wd.radius, G)
    inside, outside = certain(wd.lens, wd.w, wd.h, wd.centre, wd.radius)
    for x in (p, p2, inside, outside):
        x.setflags(write=False)
    return p, p2, inside, outside


def truth(name):
    """(coverage at G, coverage at G / 2, certainly covered, certainly untouched) of a world's frame, computed
    once and left unchanged."""
    return _truth(name)
