"""CPU-side checks of tests/lighting_model.py, the restatement the GPU tests of the lit estimator
(tests/test_gpu_lighting*.py) hold the kernels to, and of the ray sets those tests send. No kernel runs here.

  - with one member of the lighting set the model gives the bits of the model of that member alone:
    env_nee_model.ray_color (a sampler), light_nee_model.ray_color (lights), env_model.ray_color (a plain
    map, and nothing);
  - at max_depth == 1, and on every path without a Lambertian bounce, a map with lights gives the plain
    map's bits;
  - the draws of a bounce are the map's four, then the light's: a lighting with both gives neither single
    model's bits on paths that bounce, and its map samples are the sampler-only model's while no light
    sample has been drawn before them (the first bounce of every path);
  - the ray sets of tests/lighting_cases.py show every event the estimator has at least once under every
    lighting, a bounce with both shadow rays and one with each single ray among them, so the GPU tests
    cannot pass on sets that never take a branch; what a scene cannot show is listed in
    lighting_cases.MISSING and asserted absent;
  - the instance rows' ray sets (env_cases.ROWS) show bounces with both rays under a sampled map.
"""
import numpy as np
import pytest

import env_cases as ec
import env_model as em
import env_nee_model as enm
import light_nee_model as lm
import lighting_cases as cs
import lighting_model as lg
import plan_worlds as pw
import probe_sets as ps
from oracle import crt_oracle_py as orc

N = 384  # of each set, for the reductions


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def small(crt, name):
    rays, states = cs.lc.query(crt, name, N, N)
    return ps.scene_data(crt, name), rays, states


@pytest.mark.parametrize("depth", [2, 50])
@pytest.mark.parametrize("name", cs.SCENES)
def test_one_member_gives_that_members_model(crt, name, depth):
    d, rays, states = small(crt, name)
    for label in cs.FIRST + ["sampled-sun-nearest"]:
        lit = cs.lighting(d, label)
        run = lambda L: lg.ray_color(orc, d, rays, states, depth, cs.BG, cs.T_MIN, L, crt=crt)  # noqa: E731
        if lit.etb is not None:
            got, ended, tr = run(lg.Lighting(lit.env, lit.etb, None))
            want, wended, wtr = enm.ray_color(orc, d, rays, states, depth, cs.BG, cs.T_MIN, lit.env, lit.etb, crt=crt)
            assert same(got, want) and np.array_equal(ended, wended), (name, label, "sampler alone")
            assert len(tr.map_kept) == len(wtr.nee_free) and len(tr.map_occluded) == len(wtr.nee_occluded)
            assert sorted(tr.map_skipped) == sorted(wtr.nee_skipped) and not tr.light_kept and not tr.both
        got, ended, _, _ = em.ray_color(orc, d, rays, states, depth, cs.BG, cs.T_MIN, env=lit.env, crt=crt)
        assert same(run(lg.Lighting(lit.env, None, None))[0], got), (name, label, "a plain map alone")
    lit = cs.lighting(d, cs.FIRST[0])
    got, ended, tr = lg.ray_color(orc, d, rays, states, depth, cs.BG, cs.T_MIN, lg.Lighting(None, None, lit.ltb), crt=crt)
    want, wended, wtr = lm.ray_color(orc, d, rays, states, depth, cs.BG, cs.T_MIN, lit.ltb, crt=crt)
    assert same(got, want) and np.array_equal(ended, wended), (name, "lights alone")
    assert len(tr.light_kept) == len(wtr.kept) and sorted(tr.light_far_side) == sorted(wtr.far_side)
    assert sorted(tr.light_hidden_other) == sorted(wtr.hidden_other) and not tr.map_kept and not tr.both
    got = lg.ray_color(orc, d, rays, states, depth, cs.BG, cs.T_MIN, lg.Lighting(), crt=crt)[0]
    assert same(got, em.ray_color(orc, d, rays, states, depth, cs.BG, cs.T_MIN, crt=crt)[0]), (name, "nothing")


@pytest.mark.parametrize("name", cs.SCENES)
def test_depth_one_and_paths_without_a_lambertian_bounce_are_the_plain_maps(crt, name):
    d, rays, states = small(crt, name)
    for label in cs.FIRST:
        lit = cs.lighting(d, label)
        flat1 = em.ray_color(orc, d, rays, states, 1, cs.BG, cs.T_MIN, env=lit.env, crt=crt)[0]
        got1, _, tr1 = lg.ray_color(orc, d, rays, states, 1, cs.BG, cs.T_MIN, lit, crt=crt)
        assert same(got1, flat1) and not tr1.both and not tr1.none, (name, label)
        flat = em.ray_color(orc, d, rays, states, 50, cs.BG, cs.T_MIN, env=lit.env, crt=crt)[0]
        got, _, tr = lg.ray_color(orc, d, rays, states, 50, cs.BG, cs.T_MIN, lit, crt=crt)
        plain = np.ones(len(rays), bool)
        plain[list(tr.lambertian)] = False
        assert plain.sum() >= 50 and (~plain).sum() >= 50
        assert same(got[plain], flat[plain]) and not same(got[~plain], flat[~plain]), (name, label)


def test_both_members_draw_the_maps_numbers_first(crt):
    """Under a sampler with lights the first bounce of a path draws the map's four numbers where the
    sampler-only model draws them, so the first map sample of a path is that model's; the light's
    numbers follow, so from the second bounce on the two part."""
    name = "cornell"
    d, rays, states = small(crt, name)
    lit = cs.lighting(d, "sampled-random-bilinear")
    both, _, tr = lg.ray_color(orc, d, rays, states, 2, cs.BG, cs.T_MIN, lit, crt=crt)
    only, _, otr = lg.ray_color(orc, d, rays, states, 2, cs.BG, cs.T_MIN, lg.Lighting(lit.env, lit.etb, None), crt=crt)
    # depth 2 has one bounce a path: the map terms are equal, term for term
    assert len(tr.map_kept) >= 20 and tr.map_kept == otr.map_kept and tr.map_occluded == otr.map_occluded
    assert tr.map_skipped == otr.map_skipped and len(tr.light_kept) >= 20
    deep, _, _ = lg.ray_color(orc, d, rays, states, 50, cs.BG, cs.T_MIN, lit, crt=crt)
    for single in (lg.Lighting(lit.env, lit.etb, None), lg.Lighting(None, None, lit.ltb)):
        assert not same(deep, lg.ray_color(orc, d, rays, states, 50, cs.BG, cs.T_MIN, single, crt=crt)[0])


@pytest.mark.parametrize("label", list(cs.LIGHTINGS))
@pytest.mark.parametrize("name", cs.SCENES)
def test_the_gpu_tests_ray_sets_show_every_event(crt, name, label):
    _, ended, tr = cs.model(crt, orc, name, label, 50)
    seen = lg.counts(tr)
    print(name, label, len(ended), seen)
    assert cs.missing_events(name, label, tr) == [], (name, label, seen)
    for e in cs.MISSING[name]:
        assert seen[e] == 0, (name, label, e, "listed as impossible, yet seen")
    if not cs.LIGHTINGS[label][0]:  # a plain map is never sampled
        assert all(seen[e] == 0 for e in cs.MAP_EVENTS)
    # the sub-events partition their parents
    assert len(tr.map_below) + len(tr.map_zero_pdf) == len(tr.map_skipped)
    assert len(tr.light_below) + len(tr.light_far_side) == len(tr.light_no_ray)
    if name == "rtow_final_lights":
        assert cs.events(name, True) == list(lg.EVENTS)  # one scene shows them all
    # the events are consistent with the patterns: a map ray was kept or occluded, a light ray kept, hidden or dropped
    assert len(tr.both) + len(tr.map_only) == len(tr.map_kept) + len(tr.map_occluded)
    assert len(tr.both) + len(tr.light_only) == (len(tr.light_kept) + len(tr.light_hidden_other) + len(tr.light_hidden_light) +
                                                 len(tr.light_dropped))


def test_the_capacity_set_has_4097_paths_and_more(crt):
    rays, states = cs.big_query(crt, "rtow_final_lights")
    assert len(rays) >= 4097 and len(states) == len(rays)


@pytest.mark.parametrize("label", [r.label for r in ec.ROWS])
def test_the_instance_rows_bounce_with_both_rays(crt, label):
    row = ec.BY_LABEL[label]
    d, _ = pw.world(crt, row.family, row.n)
    assert lm.usable(lm.tables(d)), label
    rays, states = ec.ray_set(crt, row.family, row.n)
    rays, states = rays[:384], states[:384]
    for sampled in (True, False):
        _, _, tr = lg.ray_color(orc, d, rays, states, pw.DEPTH, ec.BG, ec.T_MIN, cs.row_lighting(d, sampled), crt=crt,
                                bvh=ec.bvh_of(row.family))
        seen = lg.counts(tr)
        print(label, sampled, seen)
        if sampled:
            assert seen["both"] >= 5 and seen["map_only"] >= 5 and seen["map_kept"] >= 5, (label, seen)
        assert seen["light_only"] >= 5 and seen["none"] >= 1, (label, seen)
        assert seen["light_kept"] + seen["light_hidden_other"] + seen["light_hidden_light"] >= 5, (label, seen)
