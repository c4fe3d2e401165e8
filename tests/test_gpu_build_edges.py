"""The GPU scene set-up at its task and tile edges: every case of tests/build_cases.py
(tests/test_build_cases.py shows from the host tree where each one sits) is built with build_device=0
and must equal the host build (which tests/test_host_abi.py pins to the reference's BVH goldens):
the exported tree byte for byte, info()'s counts, depth and largest leaf, and the device image byte
for byte, on both routes: device_create_scene (crt_stage_gpu.hip: flatten, build, node order and
slots on the device) and, under CRT_HOST_STAGE=1, device_build_bvh (the GPU tree from host-flattened
boxes, staged on the host). The build's own CRT_DEBUG_BUILD lines show that the route really ran and
that each level had the big and small tasks the host tree implies, so a silent fall-back to the host
path or a task classed on the wrong side of kBigTask fails here even where the tree comes out equal.

One case per family also answers closest-hit queries and renders a small frame from the
device-staged copy, bit-identical to the host-staged one. Left off those: the leaves of 4097 to 5870
primitives (bigleaf family, but for its one-axis line) and the chains of depth 327 and 477, which
are beyond the leaf sizes and depths any render test here has run."""
import re

import numpy as np
import pytest

import build_cases as bc
from test_gpu_bvh_build import same_tree
from test_gpu_stage import same_image

pytestmark = pytest.mark.gpu

BIG_LINE = re.compile(r"^bvh level (\d+): (\d+) big \+ (\d+) small tasks ", re.M)
BATCH_LINE = re.compile(r"^bvh level (\d+): (\d+) small tasks \(batched\)$", re.M)
STAGE_LINE = re.compile(r"^device scene (\w+)", re.M)


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_device_route_equals_host(crt, monkeypatch, case):
    monkeypatch.delenv("CRT_HOST_STAGE", raising=False)
    d = bc.host_tree(crt, case)[0]
    same_tree(crt, d, **case.kw)
    same_image(crt, d, **case.kw)


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_host_staged_route_equals_host(crt, monkeypatch, case):
    monkeypatch.setenv("CRT_HOST_STAGE", "1")  # read at every crt_scene_create
    d = bc.host_tree(crt, case)[0]
    same_tree(crt, d, **case.kw)
    same_image(crt, d, **case.kw)


def build_lines(crt, capfd, d, kw):
    before = capfd.readouterr()
    crt.GpuScene(d, build_device=0, **kw).close()
    err = capfd.readouterr().err
    print(before.out, end="")  # what the test printed so far stays in its report
    big = [tuple(map(int, m)) for m in BIG_LINE.findall(err)]
    batched = [tuple(map(int, m)) for m in BATCH_LINE.findall(err)]
    return big, batched, STAGE_LINE.findall(err), err


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_levels_ran_the_tasks_of_the_host_tree(crt, monkeypatch, capfd, case):
    """Per level, the big and small task counts the build prints equal what tree_tasks derives from
    the host tree; the batched levels come eight at a time and are empty after the tree ends. The
    `device scene` lines show device_create_scene at work; under CRT_HOST_STAGE=1 they are absent
    and the `bvh level` lines are the same."""
    d, f, _, _ = bc.host_tree(crt, case)
    want_big, want_batched = f["lines"]
    first = f["last_big"] + 1
    want_batched = [(first + j, c) for j, c in enumerate(want_batched)]
    monkeypatch.setenv("CRT_DEBUG_BUILD", "1")
    for host_stage in (False, True):
        if host_stage:
            monkeypatch.setenv("CRT_HOST_STAGE", "1")
        else:
            monkeypatch.delenv("CRT_HOST_STAGE", raising=False)
        big, batched, stage, err = build_lines(crt, capfd, d, case.kw)
        print(f"{case.id} host_stage={int(host_stage)}: big {big} batched {[c for _, c in batched]}")
        assert big == want_big, err
        assert batched == want_batched, err
        if host_stage:
            assert stage == [], err
        else:
            assert {"upload", "validate", "primitives", "build", "image"} <= set(stage), err


# ---- (d) queries and a frame from the device-staged copy -------------------------------------------------
HIT_CASES = [c for c in bc.CASES if c.hits]
assert [c.family for c in HIT_CASES] == ["cloud", "clusters", "bigleaf", "buckets", "chain", "nodes", "scan", "scan", "ties"]


def aimed_rays(nodes, seed, n=1024):
    """Seeded rays from around the scene: half aimed at the middle of a random leaf's box, half anywhere."""
    rng = np.random.default_rng(seed)
    b = nodes["bounds"][0]
    mid, half = (b[0::2] + b[1::2]) / 2, (b[1::2] - b[0::2]) / 2 + 1.0
    o = mid + rng.uniform(-1.5, 1.5, (n, 3)) * half
    leaves = np.flatnonzero(nodes["count"] > 0)
    lb = nodes["bounds"][rng.choice(leaves, n)]
    dirs = (lb[:, 0::2] + lb[:, 1::2]) / 2 - o
    dirs[n // 2:] = rng.normal(size=(n - n // 2, 3)) * half
    return np.concatenate([o, dirs], axis=1)


BACKGROUND = (0.55, 0.7, 0.95)


def close_camera(crt, d, nodes):
    """24 x 16 x 2 spp on the first node of at most 16 primitives down the left spine, from three
    of its half extents away: some of the scene's (mostly sparse) primitives fill pixels."""
    from cpp_raytracer_amd._capi import D3
    t = bc.tree_tasks(nodes)
    i = 0
    while t["hi"][i] - t["lo"][i] > 16:
        i += 1
    b = nodes["bounds"][i]
    mid, half = (b[0::2] + b[1::2]) / 2, (b[1::2] - b[0::2]) / 2
    eye = mid + np.array([0.3, 0.2, 1.0]) * 3 * half.max()
    return crt.camera_with(d.camera, image_w=24, image_h=16, samples_per_pixel=2, max_depth=8, center=D3(*eye),
                           lookat=D3(*mid), has_lookat=1, up=D3(0.0, 1.0, 0.0), fov=float(np.deg2rad(40.0)),
                           fov_is_vertical=1, defocus_angle=0.0, focus_dist=1.0, has_focus_dist=1,
                           background=D3(*BACKGROUND))


@pytest.mark.parametrize("case", HIT_CASES, ids=lambda c: c.id)
def test_queries_and_a_frame_from_the_device_staged_scene(crt, monkeypatch, case):
    monkeypatch.delenv("CRT_HOST_STAGE", raising=False)
    d, _, nodes, _ = bc.host_tree(crt, case)
    host = crt.GpuScene(d, **case.kw)
    dev = crt.GpuScene(d, build_device=0, **case.kw)
    rays = aimed_rays(nodes, 31)
    want, got = host.closest_hits(rays), dev.closest_hits(rays)
    assert (want["prim"] >= 0).sum() >= 256
    assert got.tobytes() == want.tobytes()
    cam = crt.resolve_camera(close_camera(crt, d, nodes), 7)
    a, b = host.render(cam)[0], dev.render(cam)[0]
    assert np.isfinite(a).all() and (np.abs(a - BACKGROUND).max(-1) > 0).sum() >= 4  # not the background alone
    assert a.tobytes() == b.tobytes()
    assert host.guard(0) == 0 and dev.guard(0) == 0
    host.close()
    dev.close()
