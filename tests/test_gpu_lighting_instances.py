"""Every reachable lit instance of the radiance kernels on the GPU, `radiance_kernel<SE, GSTACK, LSCENE,
PM, true, NEE, true>` for NEE true (a sampled map with the lights) and false (a plain map with the
lights), held to tests/lighting_model.py bit for bit on env_cases.ROWS unchanged, at plan_worlds.DEPTH
(tests/test_lighting_model.py checks without a GPU that every row's rays bounce with both shadow rays).

  1. instances  every row, both combinations: the fast route's bytes are the plain route's and both are
                the model's; both members are seen
  2. refill     the two PM 1 rows on grids of 1 and 3 blocks: a lane runs two shadow segments and its
                saved continuation while the lanes beside it are refilled

Every call has 384 paths at depth 8; the largest world has 2950 objects. Outputs are pre-filled with 0xFF
bytes and followed by a sentinel tail that must be intact afterwards (test_gpu_lighting.run); a row's
scene is built and uploaded under its route's switches, its plan is asserted before it runs, its parity
guard count is 0 afterwards and it is closed in the row."""
import contextlib

import numpy as np
import pytest

import env_cases as ec
import lighting_cases as cs
import lighting_model as lg
import plan_worlds as pw
import test_gpu_env_nee as tgn
import test_gpu_lighting as tgl
from oracle import crt_oracle_py as orc
from test_gpu_radiance import bits, guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
DEPTH = pw.DEPTH
N = 384
LABELS = [r.label for r in ec.ROWS]
TWO_ROWS = ["lds-u16-pm1", "gstack-u16-pm1"]  # the LDS-scene PM 1 row and the u16 HBM-stack PM 1 row
same, differing = tgl.same, tgl.differing


@contextlib.contextmanager
def opened(crt, row):
    """(the row's scene on device 0, its SceneData, rays, states): the plan asserted first, the scene built
    and uploaded under the row's route, which stays set for the calls; guard 0, closed."""
    d, kw = pw.world(crt, row.family, row.n)
    rays, states = ec.ray_set(crt, row.family, row.n)
    with pw.route(row.route):
        s = crt.GpuScene(d, **kw)
        try:
            plan = ec.plan_of(s, row)
            print(f"{row.label}: {row.family} {row.n} under {row.route}, (klass, entry_bytes, prim_mode) = {plan}")
            s.upload(0)
            yield s, d, rays[:N], states[:N]
            assert s.guard(0) == 0, row.label
        finally:
            s.close()


def lightings(crt, s, d):
    """[(sampled, the model's Lighting, the package's)] of a row's scene, a sampled map and a plain one, each with the scene's lights."""
    lights = s.light_sampler(0)
    out = []
    for sampled in (True, False):
        mlit = cs.row_lighting(d, sampled)
        out.append((sampled, mlit, crt.Lighting(env=tgn.device_env(crt, mlit.env, {}, importance=sampled), lights=lights)))
    return out


@pytest.mark.parametrize("label", LABELS)
def test_every_lit_instance_is_the_model_bit_for_bit(crt, label):
    row = ec.BY_LABEL[label]
    with opened(crt, row) as (s, d, rays, states):
        for sampled, mlit, lit in lightings(crt, s, d):
            want, _, tr = lg.ray_color(orc, d, rays, states, DEPTH, ec.BG, ec.T_MIN, mlit, crt=crt, bvh=ec.bvh_of(row.family))
            assert len(tr.light_only) and len(tr.none) and (not sampled or (len(tr.both) and len(tr.map_only))), lg.counts(tr)
            fast = tgl.run(crt, s, rays, states, DEPTH, lit, bg=ec.BG, t_min=ec.T_MIN)
            plain = tgl.run(crt, s, rays, states, DEPTH, lit, bg=ec.BG, t_min=ec.T_MIN, flags=tgl.PLAIN)
            bad = differing(fast, plain)
            assert len(bad) == 0, (label, sampled, "fast != plain", len(bad), bad[:5], fast[bad[:3]], plain[bad[:3]])
            bad = differing(fast, want)
            assert len(bad) == 0, (label, sampled, "fast != model", len(bad), bad[:5], rays[bad[:3]], fast[bad[:3]], want[bad[:3]])
            for one in (crt.Lighting(env=lit.env), crt.Lighting(lights=lit.lights)):  # both members are seen
                assert not same(fast, tgl.run(crt, s, rays, states, DEPTH, one, bg=ec.BG, t_min=ec.T_MIN))


@pytest.mark.parametrize("label", TWO_ROWS)
def test_small_grids_under_a_lighting(crt, monkeypatch, label):
    row = ec.BY_LABEL[label]
    with opened(crt, row) as (s, d, rays, states):
        for sampled, mlit, lit in lightings(crt, s, d):
            want = lg.ray_color(orc, d, rays, states, DEPTH, ec.BG, ec.T_MIN, mlit, crt=crt, bvh=ec.bvh_of(row.family))[0]
            whole = tgl.run(crt, s, rays, states, DEPTH, lit, bg=ec.BG, t_min=ec.T_MIN)
            for blocks in ("1", "3"):
                with monkeypatch.context() as m:
                    m.setenv("CRT_GRID_BLOCKS", blocks)
                    got = tgl.run(crt, s, rays, states, DEPTH, lit, bg=ec.BG, t_min=ec.T_MIN)
                assert same(got, whole), (label, sampled, blocks, "the default grid's bytes")
                bad = differing(got, want)
                assert len(bad) == 0, (label, sampled, blocks, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
