"""Every reachable lights instance of the radiance kernels on the GPU, held to tests/light_nee_model.py
bit for bit at the smallest worlds that reach it: tests/env_cases.py's rows, unchanged, each row's plan
asserted before anything runs (the sampler adds no LDS, so GpuScene.launch_plan("radiance") is the
sampled call's plan too). Every fifth object of these worlds is a light: spheres, hollow ones among them,
parallelograms and Boxes.

  1. instances  every row: the fast route's bytes are the plain route's and both are the model's at depth 8
                on the row's 1536 seeded rays; the model keeps at least one sample and loses at least one to
                an occluder in every world, and weights a light hit in all but chain's nested shells
  2. refill     the two PM 1 rows on grids of 1 and 3 blocks: a lane runs its shadow segment and its saved
                continuation while the lanes beside it refill

Outputs are pre-filled with 0xFF bytes and followed by a sentinel tail that must be intact afterwards
(test_gpu_light_nee.run); a row's scene is built and uploaded under its route's switches, its parity guard
count is 0 afterwards and it is closed in the row (test_gpu_env_instances.opened)."""
import pytest

import env_cases as ec
import light_cases as lc
import light_nee_model as lm
import plan_worlds as pw
import test_gpu_light_nee as tgl
from oracle import crt_oracle_py as orc
from test_gpu_env_instances import TWO_ROWS, differing, opened
from test_gpu_radiance import guard_stays_zero  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
BG, PLAIN, DEPTH = ec.BG, tgl.PLAIN, pw.DEPTH
LABELS = [r.label for r in ec.ROWS]
same = tgl.same

_WANT = {}


def modelled(crt, row, p):
    """The model's output for the row's world and ray set, once per world."""
    k = (row.family, row.n)
    if k not in _WANT:
        want, _, tr = lm.ray_color(orc, p.d, p.rays, p.states, DEPTH, BG, ec.T_MIN, lm.tables(p.d), crt=crt, bvh=p.bvh)
        print(f"{row.family} {row.n}: {lc.counts(tr)}, {len(tr.hits_plain)} unweighted light hits")
        # chain's nested shells leave no Lambertian bounce a free way to a light: samples are kept there, but
        # no bounce ray of its 1536 reaches a light with pb set
        assert tr.kept and (tr.hidden_other or tr.hidden_light) and (tr.hits_weighted or row.family == "chain")
        want.setflags(write=False)
        _WANT[k] = want
    return _WANT[k]


@pytest.mark.parametrize("label", LABELS)
def test_every_lights_instance_is_the_model_bit_for_bit(crt, label):
    row = ec.BY_LABEL[label]
    with opened(crt, row) as (s, p):
        want = modelled(crt, row, p)
        assert not same(want, p.flat)  # not the unsampled estimator's bytes
        smp = s.light_sampler(0)
        fast = tgl.run(s, p.rays, p.states, DEPTH, smp, bg=BG, t_min=ec.T_MIN)
        plain = tgl.run(s, p.rays, p.states, DEPTH, smp, bg=BG, t_min=ec.T_MIN, flags=PLAIN)
        bad = differing(fast, plain)
        assert len(bad) == 0, (label, "fast != plain", len(bad), bad[:5], fast[bad[:3]], plain[bad[:3]])
        bad = differing(fast, want)
        assert len(bad) == 0, (label, "fast != model", len(bad), bad[:5], p.rays[bad[:3]], fast[bad[:3]], want[bad[:3]])
        del smp


@pytest.mark.parametrize("label", TWO_ROWS)
def test_small_grids_under_a_sampler(crt, monkeypatch, label):
    row = ec.BY_LABEL[label]
    with opened(crt, row) as (s, p):
        want = modelled(crt, row, p)
        smp = s.light_sampler(0)
        for blocks in ("1", "3"):
            with monkeypatch.context() as m:
                m.setenv("CRT_GRID_BLOCKS", blocks)
                got = tgl.run(s, p.rays, p.states, DEPTH, smp, bg=BG, t_min=ec.T_MIN)
            bad = differing(got, want)
            assert len(bad) == 0, (label, blocks, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
        del smp
