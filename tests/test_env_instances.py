"""CPU-side checks of tests/env_cases.py, the table tests/test_gpu_env_instances.py runs on the GPU. No
kernel runs here.

  - every row's radiance plan is the instance the row names, and the rows cover every reachable
    (class, entry width, primitive mode);
  - every row's ray set is worth running: a fifth or more of its paths escape after a bounce, some end
    on a light, some escape after two or more bounces;
  - the path model with a constant background is the oracle's ray_color on those rays through the
    world's own tree, within the project's bar for a forward-throughput integrator (1e-12, DESIGN
    section 6e);
  - exact face ties of the lookup survive a bounce off an axis-aligned mirror.
"""
import numpy as np
import pytest

import env_cases as ec
import env_model as em
import plan_worlds as pw
import probe_sets as ps
from oracle import crt_oracle_py as orc
from test_env_model import probe_directions

WORLDS = sorted({(r.family, r.n) for r in ec.ROWS})


def test_every_row_plans_its_instance_and_the_rows_cover_the_reachable_ones(crt):
    seen = set()
    for row in ec.ROWS:
        with pw.route(row.route):
            _, s = pw.gpu_scene(crt, row.family, row.n)
            plan = ec.plan_of(s, row)
            s.close()
        print(f"{row.label:22} {row.family:8} {row.n:5} {row.route:8} (klass, entry_bytes, prim_mode) = {plan}")
        seen.add(plan)
    assert seen == ec.REACHABLE and len(ec.REACHABLE) == 10
    assert any(r.route == "notop" and r.family == "mixed" for r in ec.ROWS)
    assert len(ec.BY_LABEL) == len(ec.ROWS)


@pytest.mark.parametrize("family,n", WORLDS, ids=[f"{f}-{n}" for f, n in WORLDS])
def test_ray_sets_bounce_before_they_leave(crt, family, n):
    p = ec.paths(crt, family, n, orc)
    assert len(p.rays) == ec.N_RAYS == 1536 and p.states.dtype == np.uint32
    o = np.array(list(p.d.camera.center))
    assert (p.rays[:, :3] == o).all()
    share, lights, after_two = ec.shares(p)
    print(f"{family} {n}: {share:.3f} of the paths escape after a bounce, {after_two} of them after two or more; "
          f"ends {np.bincount(p.ended, minlength=4).tolist()} (miss, light, absorbed, depth)")
    assert share >= ec.MIN_ESCAPE_SHARE == 0.20
    assert lights >= 1
    assert after_two >= 1
    # an escape after a bounce leaves along a direction the caller never supplied
    after = (p.ended == em.MISS) & ~p.first_miss
    assert (p.last[after] != p.rays[after, 3:]).any(1).all()


@pytest.mark.parametrize("family,n", WORLDS, ids=[f"{f}-{n}" for f, n in WORLDS])
def test_path_model_is_the_oracles_ray_color_through_the_worlds_tree(crt, family, n):
    p = ec.paths(crt, family, n, orc)
    want = orc.radiance(p.d, p.rays, p.states, pw.DEPTH, ec.BG, ec.T_MIN, threads=16, **p.bvh)
    err = np.abs(p.flat - want) / np.maximum(1.0, np.abs(want))
    print(f"{family} {n}: max |model - oracle| / max(1, |oracle|) = {err.max():.3g}, max |oracle| = {np.abs(want).max():.3g}")
    assert err.max() <= 1e-12
    assert np.abs(want).max() > 0


@pytest.mark.parametrize("axis", [1, 0], ids=["normal-y", "normal-x"])
def test_face_ties_survive_a_mirror_bounce(crt, axis):
    """Reflection about an exact axis normal flips one sign and the normalisation scales the three
    components alike, so |x| = |y| and |y| = |z| are still exact in the direction the path leaves on."""
    d = ec.mirror_world(crt, axis)
    rays = ec.mirror_rays(probe_directions(), axis)
    states = ps.states(len(rays), 5)
    _, ended, last, T = em.ray_color(orc, d, rays, states, pw.DEPTH, ec.BG, ec.T_MIN, crt=crt)
    bounced = (ended == em.MISS) & (np.array(last) != rays[:, 3:]).any(1)
    tied = bounced & ec.ties(last)
    print(f"mirror with normal {'xyz'[axis]}: {len(rays)} rays, {int(bounced.sum())} bounce and escape, "
          f"{int(tied.sum())} of them on an exact tie")
    assert len(rays) == 870
    assert tied.sum() >= 10
    assert (last[bounced][:, axis] > 0).all()  # they leave on the mirror's near side
    assert (T[bounced] == np.array([0.5, 0.75, 0.25])).all()
