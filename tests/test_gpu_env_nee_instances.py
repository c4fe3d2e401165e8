"""Every reachable NEE instance of the radiance kernels on the GPU, held to tests/env_nee_model.py bit
for bit at the smallest worlds that reach it: tests/env_cases.py's rows, unchanged, each row's plan
asserted before anything runs (the sampler adds no LDS, so GpuScene.launch_plan("radiance") is the
sampled call's plan too).

  1. instances  every row, a random map behind a rotated basis: the fast route's bytes are the plain
                route's and both are the model's at depth 8 on the row's 1536 seeded rays; the model takes
                at least one unoccluded NEE, one occluded NEE and one weighted escape in every world
  2. refill     the LDS-scene PM 1 row and the u16 HBM-stack PM 1 row on grids of 1 and 3 blocks: a lane
                runs its shadow segment and its saved continuation while the lanes beside it refill

Outputs are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact afterwards
(test_gpu_env_nee.run); a row's scene is built and uploaded under its route's switches, its parity guard
count is 0 afterwards and it is closed in the row (test_gpu_env_instances.opened)."""
import numpy as np
import pytest

import env_cases as ec
import env_model as em
import env_nee_model as nm
import plan_worlds as pw
import test_gpu_env_nee as tgn
from oracle import crt_oracle_py as orc
from test_env_model import ROTATED
from test_gpu_env_instances import TWO_ROWS, differing, opened
from test_gpu_radiance import guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
BG, PLAIN, DEPTH = ec.BG, tgn.PLAIN, pw.DEPTH
LABELS = [r.label for r in ec.ROWS]
same = tgn.same

_WANT = {}


def modelled(crt, row, p, filt):
    """(the map, the model's output for the row's world and ray set under it), once per world and filter."""
    k = (row.family, row.n, filt)
    if k not in _WANT:
        menv = em.make(tgn.random_map(5, 400 + row.n), filter=filt, **ROTATED)
        want, _, tr = nm.ray_color(orc, p.d, p.rays, p.states, DEPTH, BG, ec.T_MIN, menv, nm.tables(menv), crt=crt, bvh=p.bvh)
        print(f"{row.family} {row.n}: {len(tr.nee_free)} unoccluded and {len(tr.nee_occluded)} occluded NEE samples, "
              f"{len(tr.escapes_weighted)} weighted escapes, {len(tr.escapes_plain)} unweighted ones")
        assert tr.nee_free and tr.nee_occluded and tr.escapes_weighted
        want.setflags(write=False)
        _WANT[k] = (menv, want)
    return _WANT[k]


def held(s, p, env, want, what):
    fast = tgn.run(s, p.rays, p.states, DEPTH, env, bg=BG, t_min=ec.T_MIN)
    plain = tgn.run(s, p.rays, p.states, DEPTH, env, bg=BG, t_min=ec.T_MIN, flags=PLAIN)
    bad = differing(fast, plain)
    assert len(bad) == 0, (what, "fast != plain", len(bad), bad[:5], fast[bad[:3]], plain[bad[:3]])
    bad = differing(fast, want)
    assert len(bad) == 0, (what, "fast != model", len(bad), bad[:5], p.rays[bad[:3]], fast[bad[:3]], want[bad[:3]])
    return fast


@pytest.mark.parametrize("label", LABELS)
def test_every_nee_instance_is_the_model_bit_for_bit(crt, label):
    row = ec.BY_LABEL[label]
    with opened(crt, row) as (s, p):
        filt = em.BILINEAR if LABELS.index(label) % 2 else em.NEAREST
        menv, want = modelled(crt, row, p, filt)
        assert not same(want, ec.lit_by(menv, p))  # not the unsampled estimator's bytes
        held(s, p, tgn.device_env(crt, menv, ROTATED), want, (label, filt))


@pytest.mark.parametrize("label", TWO_ROWS)
def test_small_grids_under_a_sampler(crt, monkeypatch, label):
    row = ec.BY_LABEL[label]
    with opened(crt, row) as (s, p):
        for filt in tgn.FILTERS:
            menv, want = modelled(crt, row, p, filt)
            env = tgn.device_env(crt, menv, ROTATED)
            for blocks in ("1", "3"):
                with monkeypatch.context() as m:
                    m.setenv("CRT_GRID_BLOCKS", blocks)
                    got = tgn.run(s, p.rays, p.states, DEPTH, env, bg=BG, t_min=ec.T_MIN)
                bad = differing(got, want)
                assert len(bad) == 0, (label, filt, blocks, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
