"""Both sides of every capacity edge of the launch plans (tests/plan_worlds.py, tests/test_launch_plan.py)
on the GPU: for each row (edge, kernel, family) the scenes of n - 1 and n objects between which the plan
changes. Each case first asserts that the plan is on the side the row says, so it cannot drift into the
middle of a class, then runs that kernel at the project's usual bars:

  render    24 x 16, 4 spp, depth 8 against the oracle's render at 1e-12 * max(1, |want|), all finite,
            Schlick guard 0; bit-identical under CRT_NO_LDS_SCENE, and for HBM-scene plans under
            CRT_FORCE_GSTACK, CRT_NO_LDS_TOP and CRT_NO_PAIR_WALK; one masked pass with half the blocks
            active equals the unmasked pass in them (the MASK instance)
  trace     under CRT_TRACE_FAST: closest hits and any-hits of the centre rays and their shadow rays
            (ray_sets.set_a, set_c) equal the oracle's records (test_gpu_trace.same)
  radiance  the device's own camera rays through both routes against the oracle's ray_color
            (test_gpu_radiance_probes.held)

The treelet rows (E5) have three sides. Below the edge the treelet is the whole array, of an odd node
count (the sentinel's sibling slot lies past it); at the edge the cut leaves the last nodes of the
breadth-first array in HBM, which at a cut of one pair is the sentinel alone, so no ray can end there;
PAST objects further on the centre rays' hits lie in leaves on both sides of the cut (checked on the CPU
from export_bvh and the oracle's hits). The depth rows (E6) reach the HBM stack without
CRT_FORCE_GSTACK."""
import math

import numpy as np
import pytest

import plan_worlds as pw
import ray_sets as rs
import test_gpu_radiance as tgr
import test_gpu_trace as tgt
from oracle import crt_oracle_py as orc
from test_gpu_radiance_probes import held

pytestmark = pytest.mark.gpu
TOL = 1e-12  # relative to max(1, |want|): tests/test_gpu_fuzz_scenes.py
ROWS = pw.rows()
PAST = 100  # objects past an E5 edge at which leaves the centre rays hit lie outside the treelet
CASES = [(e, k, f, side) for e, k, f in ROWS for side in (("below", "above", "past") if e == "E5" else ("below", "above"))]
_WORLDS = {}


class World:
    """One (family, n): the scene data, the oracle's results (computed once, on demand) and the GPU
    scene of the default switches."""

    def __init__(self, crt, family, n):
        self.crt, self.family, self.n = crt, family, n
        self.d, self.kw = pw.world(crt, family, n)
        self.bvh = dict(num_buckets=self.kw.get("num_buckets", 32), max_prims=self.kw.get("max_prims_in_node", 12))
        self.cam = crt.resolve_camera(self.d.camera, pw.BASE_SEED)
        self.scene = crt.GpuScene(self.d, **self.kw)
        self.scene.upload(0)
        self._want = {}

    def fresh(self):
        """The same scene built and uploaded under the switches set now."""
        s = self.crt.GpuScene(self.d, **self.kw)
        s.upload(0)
        return s

    def want(self, what):
        if what not in self._want:
            if what == "render":
                v = orc.render(self.d, pw.BASE_SEED, threads=16)
            elif what == "sets":
                a = rs.set_a(self.crt, self.d)
                ha = orc.hits(self.d, a.rays, a.t_min, a.t_max, **self.bvh)
                c = rs.set_c(ha)
                hc = np.zeros(len(c.rays), ha.dtype)
                for t in np.unique(c.tmax):
                    sel = c.tmax == t
                    hc[sel] = orc.hits(self.d, c.rays[sel], c.t_min, float(t), **self.bvh)
                v = ((a, ha), (c, hc))
            self._want[what] = v
        return self._want[what]


def world(crt, family, n):
    if (family, n) not in _WORLDS:
        _WORLDS[family, n] = World(crt, family, n)
    return _WORLDS[family, n]


def side_of(crt, edge, kernel, family, side):
    """(World, its default plan) of the row's lower or upper side, the plan asserted to be there."""
    lo, hi = pw.edge(crt, family, kernel, edge)
    assert hi == lo + 1
    w = world(crt, family, {"below": lo, "above": hi, "past": hi + PAST}[side])
    with pw.route("default"):
        p = pw.plan_dict(w.scene.launch_plan(kernel))
    read, below, above = pw.EDGES[edge]
    assert read(p) == (below if side == "below" else above), (edge, kernel, family, side, w.n, p)
    return w, p


def render(scene, cam):
    out, _ = scene.render(cam, 1)
    return out


def device_leaf_offsets(scene):
    """primitive -> byte offset of its leaf in the device's f32 node array: crt_host.cpp stage()'s order
    (the root, a pad, then sibling pairs breadth-first for the first 1024 nodes and pair-wise depth-first
    below) restated over export_bvh's preorder nodes."""
    nodes, order = scene.export_bvh()
    nn = len(nodes)

    def interior(i):
        return nodes[i]["count"] == 0 and not (nodes[i]["flags"] & 1) and i + 1 < nn

    bfs, q = [0], 0
    while q < len(bfs) and len(bfs) < 1024:
        i = bfs[q]
        if interior(i):
            bfs += [i + 1, int(nodes[i]["index"])]
        q += 1
    todo = list(reversed(bfs[q:]))
    while todo:
        i = todo.pop()
        if interior(i):
            left, right = i + 1, int(nodes[i]["index"])
            bfs += [left, right]
            todo += [right, left]
    assert sorted(bfs) == list(range(nn))
    off = np.zeros(len(order), np.int64)
    for k, i in enumerate(bfs):
        if nodes[i]["count"] > 0:
            first = int(nodes[i]["index"])
            off[order[first:first + int(nodes[i]["count"])]] = (0 if k == 0 else k + 1) * 32
    return off


def check_treelet_row(w, p, side):
    """E5: the centre rays end in leaves inside the treelet and, past the cut, outside it too."""
    (a, ha), _ = w.want("sets")
    hit = ha["prim"][ha["prim"] >= 0]
    assert len(hit) > 100
    off = device_leaf_offsets(w.scene)[hit]
    inside, outside = int((off < p["ntop"]).sum()), int((off >= p["ntop"]).sum())
    print(f"{w.family} n={w.n} {side}: ntop {p['ntop']} of {p['all_nodes']}, hit leaves inside {inside}, outside {outside}")
    if side == "below":  # the whole array, an odd number of nodes: the sentinel's sibling is past the nodes
        assert p["ntop"] == p["all_nodes"] and p["all_nodes"] % 64 == 32 and outside == 0 and inside > 0
    elif side == "above":
        assert p["ntop"] % 64 == 0 and p["ntop"] < p["all_nodes"] and inside > 0
    else:
        assert p["ntop"] % 64 == 0 and inside > 0 and outside > 0


def check_render(crt, monkeypatch, w, p):
    want = w.want("render")
    got = render(w.scene, w.cam)
    assert w.scene.guard(0) == 0
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{w.family} n={w.n}: class {p['klass']}, max rel err {err.max():.3g}, max |want| {np.abs(want).max():.3g}")
    assert np.isfinite(got).all() and err.max() <= TOL, (w.family, w.n, float(err.max()))
    assert np.abs(want).max() > 0
    routes = [("CRT_NO_LDS_SCENE",)]
    if p["klass"] != pw.LDS_SCENE:  # route independence of an HBM scene
        routes += [("CRT_FORCE_GSTACK",), ("CRT_NO_LDS_TOP",), ("CRT_NO_PAIR_WALK",)]
    for env in routes:
        with monkeypatch.context() as m:
            for k in env:
                m.setenv(k, "1")
            s = w.fresh()
            other = render(s, w.cam)
            s.close()
        assert np.array_equal(tgr.bits(got), tgr.bits(other)), (w.family, w.n, env)
    check_masked(crt, w, got)


def check_masked(crt, w, frame):
    """One masked pass over the whole job with every other 16 x 4 block active: sums, noise state and
    preview equal the unmasked pass's in the active blocks, whose preview is the one-shot frame."""
    import torch
    h, wd = pw.H, pw.W
    nbx, nby = (wd + 15) // 16, (h + 3) // 4
    assert crt.block_count(wd, h) == nbx * nby and crt.sample_chunk_len(pw.SPP) == pw.SPP
    on = (np.add.outer(np.arange(nby), np.arange(nbx)) % 2 == 0)
    inside = torch.from_numpy(np.repeat(np.repeat(on, 4, axis=0), 16, axis=1)[:h, :wd].copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    plain = [torch.full((h, wd, k), math.nan, dtype=torch.float64, device="cuda") for k in (3, 2, 3)]
    w.scene.render_pass(0, w.cam, 0, pw.SPP, plain[0].data_ptr(), plain[1].data_ptr(), plain[2].data_ptr(), st)
    masked = [torch.full((h, wd, k), math.nan, dtype=torch.float64, device="cuda") for k in (3, 2, 3)]
    words = torch.from_numpy(np.where(on.reshape(-1), 0, 0x80000000).astype(np.uint32).view(np.int32).copy()).cuda()
    w.scene.render_pass_masked(0, w.cam, 0, pw.SPP, masked[0].data_ptr(), masked[1].data_ptr(), masked[2].data_ptr(),
                               words.data_ptr(), 0, st)
    torch.cuda.synchronize()
    assert torch.equal(plain[2], torch.from_numpy(frame).cuda()), "the unmasked pass's frame is not the one-shot frame"
    for got, want in zip(masked, plain):
        assert torch.equal(got[inside], want[inside])
        assert (got[~inside] == 0).all()
    assert (words.cpu().numpy().view(np.uint32).reshape(nby, nbx)[on] == pw.SPP).all()


def check_trace(monkeypatch, w):
    monkeypatch.setenv("CRT_TRACE_FAST", "1")
    for name, (call, want) in zip("AC", w.want("sets")):
        assert min((want["prim"] >= 0).sum(), (want["prim"] < 0).sum()) >= 20 or name == "C", (w.family, w.n, name)
        tgt.same(tgt.run(w.scene, call), want, f"{w.family} n={w.n} {name}")
        assert np.array_equal(tgt.run(w.scene, call, tgt.ANY), want["prim"] >= 0), f"{w.family} n={w.n} {name} any"


def check_radiance(w):
    rays, states = tgr.device_rays(w.scene, w.cam)
    bg = tuple(w.cam.background)
    want = orc.radiance(w.d, rays, states, pw.DEPTH, bg, w.cam.t_min, threads=16, **w.bvh)
    assert np.abs(want).max() > 0
    held(w.scene, f"{w.family} n={w.n}", rays, states, pw.DEPTH, bg, w.cam.t_min, want)
    assert w.scene.guard(0) == 0


@pytest.mark.parametrize("edge,kernel,family,side", CASES, ids=["-".join(c) for c in CASES])
def test_both_sides_of_an_edge(crt, monkeypatch, edge, kernel, family, side):
    w, p = side_of(crt, edge, kernel, family, side)
    if edge == "E5":
        check_treelet_row(w, p, side)
    if edge == "E6" and side == "above":
        assert p["klass"] == pw.HBM_STACK and p["hbm_stack_levels"] == p["depth"] + 4
    if kernel == "render":
        check_render(crt, monkeypatch, w, p)
    elif kernel == "trace":
        check_trace(monkeypatch, w)
    else:
        check_radiance(w)


def test_worlds_are_released():
    """Last in the module: the scenes kept for the rows above leave the device."""
    for w in _WORLDS.values():
        w.scene.close()
    _WORLDS.clear()
