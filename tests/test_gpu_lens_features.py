"""crt_lens_centre_rays_async and crt_lens_features_async on the GPU: the centre rays against
tests/lens_pass_model.py (bit for bit, except the directions of EQUIRECT and FISHEYE: 64 eps, by
tests/test_gpu_lens.py's argument), the features against the records built from GpuScene.trace of the
device's own centre rays and the material table, and PINHOLE against crt_render_features_async byte for
byte. Output buffers are pre-filled with 0xFF bytes and followed by a sentinel tail."""
import numpy as np
import pytest

import denoise_model as dm
import lens_pass_model as lpm
from test_gpu_lens import BG, EPS, INSIDE_CORNELL, KINDS, camera, lens_for, same
from test_gpu_radiance import guard_stays_zero, resident  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
TAIL = 64


def centre_rays(s, cam, lens):
    import torch
    rays = s.lens_centre_rays(cam, lens)
    torch.cuda.synchronize()
    assert tuple(rays.shape) == (cam.image_h * cam.image_w, 6) and rays.dtype == torch.float64
    return rays


def features(s, cam, lens):
    import torch
    from cpp_raytracer_amd import FEATURE_DTYPE
    n = cam.image_h * cam.image_w * 88
    buf = torch.full((n + TAIL,), 0xFF, dtype=torch.uint8, device="cuda")
    s.lens_features(0, cam, lens, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[n:] == 0xFF).all(), "the call wrote past its h x w records"
    return host[:n].copy().view(FEATURE_DTYPE)


@pytest.mark.parametrize("name", ["rtow_final", "cornell"])
@pytest.mark.parametrize("kind", KINDS)
def test_centre_rays_equal_the_model(crt, kind, name):
    d, s = resident(crt, name)
    w, h = (3, 18) if kind == "cube" else (7, 5)
    cam = camera(crt, d, w, h, 1)
    lens = lens_for(crt, d, kind)
    got = centre_rays(s, cam, lens).cpu().numpy()
    want = lpm.centre_rays(cam, lens)
    assert same(got[:, :3], want[:, :3]), kind
    if kind in ("equirect", "fisheye"):
        err = float(np.abs(got[:, 3:] - want[:, 3:]).max()) / EPS
        print(f"{name} {kind}: largest direction error = {err:.3g} eps")
        assert err <= 64, (kind, err)
    else:
        assert same(got[:, 3:], want[:, 3:]), kind


@pytest.mark.parametrize("name,kind,inside", [("rtow_final", "equirect", False), ("rtow_final", "fisheye", False),
                                              ("rtow_final", "pinhole", False), ("cornell", "cube", True),
                                              ("cornell", "orthographic", False), ("cornell", "equirect", False)])
def test_features_are_the_trace_of_the_centre_rays(crt, name, kind, inside):
    """rtow_final: diffuse, metal and glass spheres under the sky; cornell from inside: the six faces
    see the walls, the light and the open front, from outside a panorama sees mostly background."""
    from cpp_raytracer_amd import HIT_DTYPE
    d, s = resident(crt, name)
    w, h = (8, 48) if kind == "cube" else (40, 24)
    cam = camera(crt, d, w, h, 1)
    lens = lens_for(crt, d, kind, origin=INSIDE_CORNELL if inside else None)
    rays = centre_rays(s, cam, lens)
    hits = s.trace(rays, t_min=cam.t_min).cpu().numpy().view(HIT_DTYPE).reshape(-1)
    want = dm.features_from_hits(hits, d.materials, list(cam.background), crt.FEATURE_DTYPE)
    got = features(s, cam, lens)
    assert got.tobytes() == want.tobytes(), (name, kind)
    hit = want["prim"] >= 0
    kinds = set(d.materials["kind"][want["material"][hit]].tolist())
    print(f"{name} {kind}: {int(hit.sum())} hits, {int((~hit).sum())} misses, material kinds {sorted(kinds)}")
    assert (got["albedo"][~hit] == np.array(BG)).all() and (got["t"][~hit] == 0).all()
    if (name, kind) in (("rtow_final", "equirect"), ("cornell", "cube")):
        assert hit.any() and (~hit).any()
    if (name, kind) == ("rtow_final", "equirect"):
        assert crt.CRT_DIELECTRIC in kinds
        glass = hit & (d.materials["kind"][want["material"]] == crt.CRT_DIELECTRIC)
        assert (got["albedo"][glass] == 1.0).all()
    if (name, kind) == ("cornell", "cube"):
        assert crt.CRT_DIFFUSE_LIGHT in kinds


@pytest.mark.parametrize("name", ["rtow_final", "cornell"])
def test_pinhole_is_render_features(crt, name):
    import torch
    d, s = resident(crt, name)
    w, h = 40, 24
    cam = camera(crt, d, w, h, 1)
    ref = torch.full((w * h, 88), 0xFF, dtype=torch.uint8, device="cuda")
    s.render_features(0, cam, ref.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = features(s, cam, crt.make_lens("pinhole"))
    assert got.tobytes() == ref.cpu().numpy().tobytes()
    assert (got["prim"] >= 0).any() and (got["prim"] < 0).any()


def test_refused_calls_leave_the_output_untouched(crt):
    import torch
    from cpp_raytracer_amd import CrtError
    d, s = resident(crt, "cornell")
    cam = camera(crt, d, 4, 4, 1)
    out = torch.full((4 * 4 * 88,), 0xFF, dtype=torch.uint8, device="cuda")
    with pytest.raises(CrtError, match=r"\(-1\).*CUBE needs image_h == 6 \* image_w"):
        s.lens_features(0, cam, crt.make_lens("cube"), out.data_ptr())
    with pytest.raises(CrtError, match=r"\(-1\).*d_feat is null"):
        s.lens_features(0, cam, crt.make_lens("equirect"), 0)
    with pytest.raises(CrtError, match=r"\(-1\).*ORTHOGRAPHIC extents must be > 0"):
        s.lens_centre_rays(cam, crt.make_lens("orthographic"))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xFF).all()
