"""tests/lens_model.py checked on its own, without a GPU: the pinhole records against
radiance_model.camera_rays, unit directions, the frame's centre and seam, the cube map's face table
and the orthographic span. tests/test_gpu_lens.py then holds the kernels to this model."""
import itertools
import math

import numpy as np
import pytest

import lens_model as lm
import radiance_model as rm

EPS = 2.0 ** -52


def lens(crt, kind, **kw):
    return crt.make_lens(kind, **kw)


def camera(crt, name, w, h, spp=3, seed=21):
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named(name, 42) if name == "rtow_final" else crt.SceneData.named(name)
    return crt.resolve_camera(camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp, max_depth=50), seed)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", ["rtow_final", "cornell"])
def test_pinhole_records_are_the_camera_rays(crt, name):
    """rtow_final's camera draws on its defocus disk, cornell's does not."""
    cam = camera(crt, name, 6, 4, 8)
    assert (cam.defocus_angle > 0) == (name == "rtow_final")
    for first, count in ((0, 1), (3, 5)):
        got = lm.lens_rays(crt, cam, lens(crt, "pinhole"), first, count)
        want = rm.camera_rays(crt, cam, first, count)
        assert got[0].shape == (6 * 4 * count, 6)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])


def test_make_lens_basis_and_default_extents(crt):
    l = lens(crt, "equirect", forward=(1.0, 2.0, -0.5), up=(0.1, 1.0, 0.0))
    R, U, F = (np.array(list(v)) for v in (l.right, l.up, l.forward))
    gram = np.array([[a.dot(b) for b in (R, U, F)] for a in (R, U, F)])
    assert np.abs(gram - np.eye(3)).max() <= 4 * EPS
    assert np.abs(np.cross(R, U) - -F).max() <= 4 * EPS  # right-handed with forward = -z
    assert (l.kind, l.extent_x, l.extent_y) == (crt.CRT_LENS_EQUIRECT, math.pi, math.pi / 2)
    f = lens(crt, crt.CRT_LENS_FISHEYE)
    assert (f.kind, f.extent_x, f.extent_y, f.flags) == (3, math.pi / 2, math.pi / 2, 0)
    o = lens(crt, "orthographic", extent_x=2.0, extent_y=1.0, batch_pixels=7, plain=True)
    assert (o.extent_x, o.extent_y, o.batch_pixels, o.flags) == (2.0, 1.0, 7, crt.CRT_RADIANCE_PLAIN)
    assert (lens(crt, "cube").extent_x, lens(crt, "pinhole").extent_y) == (0.0, 0.0)
    with pytest.raises(crt.CrtError):
        lens(crt, "telephoto")
    assert [lm.PINHOLE, lm.ORTHOGRAPHIC, lm.EQUIRECT, lm.FISHEYE, lm.CUBE] == [
        crt.CRT_LENS_PINHOLE, crt.CRT_LENS_ORTHOGRAPHIC, crt.CRT_LENS_EQUIRECT, crt.CRT_LENS_FISHEYE, crt.CRT_LENS_CUBE]


@pytest.mark.parametrize("kind,ex,ey", [("equirect", 0.0, 0.0), ("equirect", 1.0, 0.4), ("fisheye", 0.0, 0.0),
                                        ("fisheye", 2.2, 2.2), ("fisheye", 0.3, 0.2)])
def test_directions_have_unit_length(crt, kind, ex, ey):
    """With an orthonormal basis the three coefficients are a point of the unit sphere."""
    l = lens(crt, kind, origin=(1.0, 2.0, 3.0), forward=(0.3, -0.2, -1.0), up=(0.0, 1.0, 0.2), extent_x=ex, extent_y=ey)
    cam = camera(crt, "cornell", 9, 7, 4)
    rays, _ = lm.lens_rays(crt, cam, l)
    assert np.abs(np.sqrt((rays[:, 3:] ** 2).sum(1)) - 1).max() <= 8 * EPS
    assert (rays[:, :3] == [1.0, 2.0, 3.0]).all()


@pytest.mark.parametrize("kind", ["equirect", "fisheye"])
def test_centre_of_an_odd_frame_is_forward(crt, kind):
    l = lens(crt, kind, forward=(0.0, 0.0, -1.0))
    cam = camera(crt, "cornell", 7, 5, 1)
    rays, _ = lm.lens_rays(crt, cam, l, jitter=False)
    a, b = lm.pixel_ab(7, 5, 3, 2)
    assert (a, b) == (0.0, 0.0)
    assert list(rays[2 * 7 + 3, 3:]) == [0.0, 0.0, -1.0]


def test_equirect_seam_is_backward(crt):
    """a = +-1 at full extent: phi = +-pi, the direction -F (sin(pi) is 1.2e-16, not 0)."""
    l = lens(crt, "equirect")
    for a in (-1.0, 1.0):
        _, d = lm.direction(l, a, 0.0)
        assert np.abs(np.array(d) - [0.0, 0.0, 1.0]).max() <= 2 * EPS, d
    _, d = lm.direction(l, 0.3, 1.0)  # the top row's edge: straight up
    assert np.abs(np.array(d) - [0.0, 1.0, 0.0]).max() <= 2 * EPS, d


# ---- the cube map -----------------------------------------------------------------------------------
AXES = [(0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, 1.0), (2, -1.0)]


def local(face, u, v):
    """The table's (x, y, z) in the basis right = x, up = y, forward = z."""
    return tuple(float(c) + 0.0 for c in lm.CUBE_FACES[face](u, v))


def test_cube_face_centres_are_the_axes():
    for face, (axis, sign) in enumerate(AXES):
        want = [0.0, 0.0, 0.0]
        want[axis] = sign
        assert list(local(face, 0.0, 0.0)) == want, face


def test_cube_faces_meet_exactly_on_the_12_edges():
    """Each of the 24 face edges (u or v = +-1) is the same set of directions, exactly, as one edge of
    another face; a wrong sign in a row of the table tears an edge open."""
    T = [-1.0, -0.75, -0.25, 0.0, 0.25, 0.75, 1.0]
    edges = {}
    for face in range(6):
        for fixed, val in itertools.product("uv", (-1.0, 1.0)):
            pts = frozenset(local(face, val, t) if fixed == "u" else local(face, t, val) for t in T)
            assert len(pts) == len(T)
            edges.setdefault(pts, []).append(face)
    assert len(edges) == 12
    for faces in edges.values():
        assert len(faces) == 2 and faces[0] != faces[1], faces


def test_cube_table_is_the_usual_layout():
    """The major-axis table of the usual cube map (sc, tc per face): +X (-z, -y), -X (z, -y), +Y (x, z),
    -Y (x, -z), +Z (x, -y), -Z (-x, -y) gives back (u, v): no face is mirrored."""
    back = [lambda x, y, z: (-z, -y), lambda x, y, z: (z, -y), lambda x, y, z: (x, z), lambda x, y, z: (x, -z),
            lambda x, y, z: (x, -y), lambda x, y, z: (-x, -y)]
    for face in range(6):
        for u, v in ((0.25, -0.5), (-1.0, 0.75), (1.0, 1.0)):
            assert back[face](*local(face, u, v)) == (u, v), face


def test_cube_faces_have_distinct_dominant_axes(crt):
    l = lens(crt, "cube", forward=(0.0, 0.0, 1.0))  # right = -x, up = y, forward = z
    R, U, F = (np.array(list(v)) for v in (l.right, l.up, l.forward))
    cam = camera(crt, "cornell", 8, 48, 1)
    rays, _ = lm.lens_rays(crt, cam, l, jitter=False)
    d = rays[:, 3:].reshape(6, 64, 3)
    d = d / np.sqrt((d ** 2).sum(-1, keepdims=True))
    seen = set()
    for face, (axis, sign) in enumerate(AXES):
        want = sign * (R, U, F)[axis]
        k = int(np.argmax(np.abs(want)))
        assert (np.argmax(np.abs(d[face]), -1) == k).all(), face
        assert (np.sign(d[face][:, k]) == np.sign(want[k])).all(), face
        seen.add((k, float(np.sign(want[k]))))
    assert len(seen) == 6


def test_cube_rows_map_to_faces():
    l = type("L", (), {"kind": lm.CUBE})
    assert [lm.face_rows(l, 3, 18, r) for r in (0, 2, 3, 17)] == [(3, 0, 0), (3, 0, 2), (3, 1, 0), (3, 5, 2)]
    l.kind = lm.FISHEYE
    assert lm.face_rows(l, 3, 18, 17) == (18, 0, 17)


# ---- orthographic -----------------------------------------------------------------------------------
def test_orthographic_origins_span_the_extents(crt):
    l = lens(crt, "orthographic", origin=(0.0, 0.0, 5.0), extent_x=3.0, extent_y=1.5)
    F = list(l.forward)
    for w, h in ((6, 4), (7, 5)):
        assert lm.pixel_ab(w, h, 0, 0, -0.5, -0.5) == (-1.0, 1.0)          # the frame's top-left corner
        assert lm.pixel_ab(w, h, w - 1, h - 1, 0.5, 0.5) == (1.0, -1.0)    # and its bottom-right one
    corners = {(a, b): lm.direction(l, a, b) for a in (-1.0, 1.0) for b in (-1.0, 1.0)}
    for (a, b), (o, d) in corners.items():
        assert o == [a * 3.0, b * 1.5, 5.0] and d == F
    cam = camera(crt, "cornell", 6, 4, 4)
    rays, _ = lm.lens_rays(crt, cam, l)
    assert (np.abs(rays[:, 0]) < 3.0).all() and (np.abs(rays[:, 1]) < 1.5).all() and (rays[:, 2] == 5.0).all()
    assert (rays[:, 3:] == F).all()
    centres, _ = lm.lens_rays(crt, cam, l, jitter=False)
    assert centres[0, 0] == -centres[-1, 0] and centres[0, 1] == -centres[-1, 1]
    assert rays[:, 0].min() < -2.0 and rays[:, 0].max() > 2.0  # the pixels spread over the whole width


def test_states_advance_by_two_draws(crt):
    cam = camera(crt, "cornell", 3, 2, 2)
    _, states = lm.lens_rays(crt, cam, lens(crt, "fisheye"))
    s = crt.sample_seed(cam.base_seed, 1 * 3 + 2, 1)
    s, _ = crt.rand_double(s, -0.5, 0.5)
    s, _ = crt.rand_double(s, -0.5, 0.5)
    assert states[(1 * 3 + 2) * 2 + 1] == s
