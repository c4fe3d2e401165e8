"""The lights instances of the radiance kernels on the worlds of tests/light_truth.py, bit for bit: every
edge world, every closed-form world, stacked, bulb and the all-sphere variants, each under
plan_worlds.route("default") and route("gstack"), the plan read through launch_plan("radiance") and
asserted first: the worlds with a parallelogram reach the PM 1 instances, the all-sphere ones (solid,
hollow and half_sunk on a ground sphere) the sphere-only instances; default gives an LDS scene, gstack the
HBM stack.

A call is 2304 paths of the world's one ray at depths 2 and 8: probe_sets.states(2048, 77), then the
crafted start states the world has (light_truth.crafted_states: xi1, xi2 or xi3 above 1 on the first
bounce, so the clamp in light_pick and points outside a parallelogram go through the kernel), then ordinary
states that pad the call to nine blocks of 256. The fast route's bytes are the plain route's and both are
tests/light_nee_model.py's. tests/test_light_truth.py has shown, without a GPU, that the model's trace of
these very calls holds each event (missed, below, far_side, hidden_light, hidden_other, after_specular,
unweighable, the clamp): here the assertion is ==.

Outputs are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact afterwards
(test_gpu_light_nee.run); a scene is built and uploaded under its route's switches, its parity guard count
is 0 afterwards and it is closed in the test."""
import numpy as np
import pytest

import light_nee_model as lm
import light_truth as lt
import plan_worlds as pw
import probe_sets as ps
import test_gpu_light_nee as tgl
from oracle import crt_oracle_py as orc
from test_gpu_env_instances import differing
from test_gpu_radiance import guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
PLAIN = tgl.PLAIN
WORLDS = lt.EDGE + lt.CLOSED + lt.OPEN + lt.SPHERES_ONLY
DEPTHS = (2, 8)
KLASS = {"default": pw.LDS_SCENE, "gstack": pw.HBM_STACK}
N_CALL = 2304

_WANT = {}


def call_states(crt, w):
    cs = lt.crafted_states(crt, w)
    crafted = np.array(list(cs.values()), np.uint32)
    pad = ps.states(N_CALL - 2048 - len(crafted), 78)
    return np.concatenate([ps.states(2048, 77), crafted, pad]), len(crafted)


def modelled(crt, w, states, depth):
    k = (w.name, depth)
    if k not in _WANT:
        want, _, tr = lm.ray_color(orc, w.d, w.rays(len(states)), states, depth, lt.BG, lt.T_MIN, lm.tables(w.d), crt=crt)
        want.setflags(write=False)
        _WANT[k] = (want, tr)
    return _WANT[k]


@pytest.mark.parametrize("route", ["default", "gstack"])
@pytest.mark.parametrize("name", WORLDS)
def test_edge_and_truth_worlds_are_the_model_bit_for_bit(crt, name, route):
    w = lt.world(crt, name)
    states, n_crafted = call_states(crt, w)
    assert len(states) == N_CALL and N_CALL % 256 == 0
    assert n_crafted == (3 if name in ("in_plane", "clamp_tail", "clamp_head", "skew", "skew_back", "stacked") else 1)
    rays = w.rays(N_CALL)
    with pw.route(route):
        s = crt.GpuScene(w.d)
        try:
            p = pw.plan_dict(s.launch_plan("radiance"))
            print(f"{name} under {route}: klass {p['klass']}, entry_bytes {p['entry_bytes']}, prim_mode {p['prim_mode']}")
            assert (p["klass"], p["prim_mode"]) == (KLASS[route], 0 if w.spheres_only else 1), (name, route, p)
            s.upload(0)
            smp = s.light_sampler(0)
            for depth in DEPTHS:
                want, tr = modelled(crt, w, states, depth)
                if name == "clamp_tail":  # the clamped pick of the crafted path is in this very call
                    assert (2048, 1, lt.RND01_OF_MAX) in tr.picks and 2048 in tr.unweighable
                fast = tgl.run(s, rays, states, depth, smp, bg=lt.BG, t_min=lt.T_MIN)
                plain = tgl.run(s, rays, states, depth, smp, bg=lt.BG, t_min=lt.T_MIN, flags=PLAIN)
                bad = differing(fast, plain)
                assert len(bad) == 0, (name, route, depth, "fast != plain", len(bad), bad[:5], fast[bad[:3]], plain[bad[:3]])
                bad = differing(fast, want)
                assert len(bad) == 0, (name, route, depth, "fast != model", len(bad), bad[:5], states[bad[:3]], fast[bad[:3]], want[bad[:3]])
            del smp
            assert s.guard(0) == 0, (name, route)
        finally:
            s.close()
