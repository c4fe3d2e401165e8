"""tests/env_nee_model.py, the restatement the GPU tests hold the sampled-environment kernels to, held in turn
to truth that is not a restatement (tests/env_truth.py): the closed-form irradiance of a cube map's texels,
and the estimator's edge events on worlds built to produce them. No kernel runs here.

  1. closed forms  the factors of all 6 n^2 texels sum to 1 and their solid angles to 4 pi (1e-12; measured 0
                   to 1.1e-16 and 0 to 3.6e-15) for n in {1, 2, 5, 8} and three normals. texel_factor against quadrature_texel on
                   the n = 5 map under ROTATED and tilted's normal, whole texels and horizon-cut ones apart: a
                   whole texel's error is relative to its factor, a cut one's to solid angle / pi, the factor it
                   would have face on (a sliver's own factor can be as small as the rule's error). Measured at
                   512 x 512 cells a texel: whole 3.2e-7, cut 5.5e-8 (solid angles 1.4e-7); at 256 x 256: whole
                   1.3e-6, cut 2.2e-7. The bars are ten times the 512 figures: WHOLE_BAR = 3.3e-6, CUT_BAR =
                   5.5e-7. The rule is of second order on whole texels (256 / 512 between 3.9 and 4.1, asserted
                   texel by texel). quadrature_lookup gives the closed-form sum of a NEAREST map to 1e-5
                   (measured 1e-6 to 2.3e-6 at 480 x 480 cells a face), so it may stand in under BILINEAR. Under
                   ROTATED, tilted's horizon cuts texels of four faces (34 texels at n = 8); +Y lies whole above
                   it and -Y whole below.
  2. model         nm.ray_color at depth 2 on every CLOSED, BILINEAR and all-sphere world, 2^14 paths of one
                   ray, states sample_seed(SEED, i, 0): per channel |mean - rho sum L F| <= 5 standard errors,
                   the standard error from the same values. random, tilted and under also through the
                   unsampled env_model.ray_color. The per-path sd / mean is held to env_truth.RATIO, from which
                   the GPU test takes its N; glass's pair ratio (depths 2 and 8, 2^12 paths) to RATIO2.
  3. events        from the Trace of the world built for each: below the horizon (every world; sun_horizon
                   half of all samples), zero_pdf only through a clamp (half_black: xi1 above 1 clamps onto
                   row 6n - 1, an empty row), xi3 above 1 at column n - 1 (sun: d_s projects onto the next
                   face, where the density is a dim texel's), occluded by roof and by ball, escapes_plain
                   after glass at depth 8.
  4. crafted       start states that make xi1 .. xi4 rnd_01(0xFFFFFFFF) > 1 on the floor bounce. rnd_01 = 0
                   cannot follow a Lambertian scatter: the triples one to four draws before the state 0 lie
                   outside the unit ball (asserted), so xi = 0 is asked of the host-compiled env_sample: the
                   direction lies on the texel's first edge, on a face edge where the column is 0, and
                   env_pdf there is the density of the face the tie rule picks.

Seeds: SEED = 6200 (2), SEED2 = 6300 (glass), each the first and only one tried. Measured z (three channels):
random 0.8, 0.9, 0.0 (unsampled -0.3, 1.6, 0.7); tilted 1.3, -1.3, -0.4 (0.5, -1.4, -0.1); sun 0.4; sun_horizon
0.4; half_black 1.1, 1.7, 2.1; under -1.4, -0.2, 0.5 (0.3, 0.5, 1.5); roof 0.6, -0.3, -0.5; ball -2.3, -0.2, 0.1
(on the GPU at 2^17 paths of another seed 0.9, -0.6, -0.3: chance); random_bilinear 0.5, -0.1, 0.2;
sun_bilinear -1.4; glass, sampled against unsampled: -0.4 to -0.1 at depth 2, -0.5 to -0.3 at depth 8.
"""
import math

import numpy as np
import pytest

import env_model as em
import env_nee_model as nm
import env_truth as et
import probe_sets as ps
from oracle import crt_oracle_py as orc
from test_env_model import ROTATED
from test_env_nee_model import host  # noqa: F401 (a fixture: crt_env_sampler.h compiled for the host)

SEED, SEED2, N, N2 = 6200, 6300, 1 << 14, 1 << 12
NORMALS = [(dict(), (0.0, 1.0, 0.0)), (ROTATED, et.TILTED_N), (dict(), et.HALF_BLACK_N)]
WHOLE_BAR, CUT_BAR = 3.3e-6, 5.5e-7
STATISTICAL = et.CLOSED + et.BILINEAR + et.SPHERES_ONLY
_RUN = {}


def modelled(crt, name, depth, states, key):
    """nm.ray_color of a world's ray under `states`, once per (name, depth, key)."""
    k = (name, depth, key)
    if k not in _RUN:
        w = et.world(crt, name)
        rgb, ended, tr = nm.ray_color(orc, w.d, w.rays(len(states)), states, depth, et.BG, et.T_MIN, w.env, nm.tables(w.env), crt=crt)
        rgb.setflags(write=False)
        _RUN[k] = (w, rgb, ended, tr)
    return _RUN[k]


def seeded(crt, name):
    return modelled(crt, name, 2, ps.default_states(SEED, N), "seeded")


def events(tr):
    return {k: len(v) for k, v in vars(tr).items() if k != "picks" and len(v)}


def paths_of(entries):
    return [e if isinstance(e, int) else e[0] for e in entries]


# ---- 1. the closed forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_factors_sum_to_one_and_solid_angles_to_four_pi(n):
    omega = et.solid_angles(n)
    assert abs(omega.sum() - 4 * math.pi) <= 1e-12 and (omega > 0).all()
    for basis, nrm in NORMALS:
        env = em.make(np.ones((6 * n, n, 3)), **basis)
        F = et.factors(env, nrm)
        print(f"n = {n}, normal {nrm}: sum F - 1 = {F.sum() - 1:.3g} (fsum {math.fsum(F.reshape(-1)) - 1:.3g}), sum omega - 4 pi = {omega.sum() - 4 * math.pi:.3g}")
        assert abs(F.sum() - 1) <= 1e-12 and (F >= 0).all()
        assert (F <= omega / math.pi * (1 + 1e-12)).all()  # cos <= 1
        if n > 1:
            assert (F == 0).any() and (F > 0).sum() >= 3 * n * n  # texels below the horizon see nothing


def test_whole_texels_are_polygon_factors_and_cut_ones_are_clipped():
    env = em.make(np.ones((48, 8, 3)), **ROTATED)
    whole = cut = 0
    for r in range(48):
        for c in range(8):
            q = et.texel_corners(env, r // 8, r % 8, c)
            # the corners are a face's own: one local coordinate is +-1, the others the texel's bounds
            local = q @ np.array([env.right, env.up, env.forward]).T
            assert np.isclose(np.abs(local).max(1), 1.0).all()
            h = q @ np.array(et.TILTED_N)
            if (h > 0).all():
                whole += 1
                assert et.texel_factor(env, r // 8, r % 8, c, et.TILTED_N) == et.polygon_factor(q, (0, 0, 0), et.TILTED_N)
                assert abs(et.edge_sum_factor(q, et.TILTED_N) - et.polygon_factor(q, (0, 0, 0), et.TILTED_N)) <= 1e-15
            elif et.is_cut(env, r // 8, r % 8, c, et.TILTED_N):
                cut += 1
                p = et.clip_to_horizon(q, et.TILTED_N)
                assert 3 <= len(p) <= 5 and (p @ np.array(et.TILTED_N) >= -1e-15).all()
    faces_cut = {r // 8 for r in range(48) for c in range(8) if et.is_cut(env, r // 8, r % 8, c, et.TILTED_N)}
    print(f"tilted, n = 8: {whole} whole texels, {cut} cut ones on faces {sorted(faces_cut)}")
    assert whole >= 150 and cut >= 30 and faces_cut == {0, 1, 4, 5}  # +Y whole above, -Y whole below


def test_closed_forms_are_the_quadratures_limit():
    env = em.make(np.ones((30, 5, 3)), **ROTATED)
    nrm = et.TILTED_N
    worst = {256: [0.0, 0.0, 0.0], 512: [0.0, 0.0, 0.0]}
    for r in range(30):
        for c in range(5):
            F = et.texel_factor(env, r // 5, r % 5, c, nrm)
            om = et.texel_solid_angle(5, r % 5, c)
            if F == 0:
                continue
            cut = et.is_cut(env, r // 5, r % 5, c, nrm)
            err = {}
            for g in (256, 512):
                q, qo, _, _ = et.quadrature_texel(env, r // 5, r % 5, c, nrm, g)
                err[g] = (q - F) / (om / math.pi if cut else F)
                worst[g][1 if cut else 0] = max(worst[g][1 if cut else 0], abs(err[g]))
                worst[g][2] = max(worst[g][2], abs(qo - om) / om)
            if not cut:
                assert 3.9 < err[256] / err[512] < 4.1, (r, c, err)
    print(f"quadrature error, whole / cut / solid angle: 512: {worst[512]}, 256: {worst[256]}")
    assert worst[512][0] <= WHOLE_BAR and worst[512][1] <= CUT_BAR and worst[512][2] <= WHOLE_BAR


def test_quadrature_lookup_is_the_closed_form_sum_under_nearest(crt):
    for name in ("random", "tilted", "half_black"):
        w = et.world(crt, name)
        q, s = et.quadrature_lookup(w.env, w.n), w.irradiance()
        print(f"{name}: quadrature of the lookup {q.tolist()}, sum L F {s.tolist()}, relative {(q / s - 1).tolist()}")
        assert (np.abs(q / s - 1) <= 1e-5).all()


def test_every_face_carries_a_share_of_some_world(crt):
    shares = np.array([et.world(crt, name).face_shares() for name in et.CLOSED])
    print(np.round(shares, 3).tolist())
    assert (shares.max(0) >= 0.05).all()
    w = et.world(crt, "ball")
    assert et.ball_margin(w) >= 0.4  # the ball's cone lies well inside its block of equal texels
    rows, cols = et.BALL_BLOCK
    assert all((w.env.texels[16 + r, c] == et.BALL_L).all() for r in rows for c in cols)
    w = et.world(crt, "roof")  # the roof's outline from o is its block of +Y texels, corner for corner
    rows, cols = et.ROOF_BLOCK
    q = np.array([et.texel_corners(w.env, 2, rows[0], cols[0])[0], et.texel_corners(w.env, 2, rows[0], cols[-1])[1],
                  et.texel_corners(w.env, 2, rows[-1], cols[-1])[2], et.texel_corners(w.env, 2, rows[-1], cols[0])[3]]) * 2.0
    v = w.d.objects["v"][1][:9]
    roof = {tuple(p) for p in (v[:3], v[:3] + v[3:6], v[:3] + v[6:9], v[:3] + v[3:6] + v[6:9])}
    assert {tuple(p) for p in q.tolist()} == {tuple(float(x) for x in p) for p in roof}


# ---- 2. the model against the closed forms --------------------------------------------------------------
@pytest.mark.parametrize("name", STATISTICAL)
def test_the_models_mean_is_the_closed_form(crt, name):
    w, rgb, ended, tr = seeded(crt, name)
    want = w.expected()
    mean, sd = rgb.mean(0), rgb.std(0, ddof=1)
    se = sd / math.sqrt(N)
    ratio = float(np.abs(sd / mean).max())
    print(f"{name}: rho sum L F = {want.tolist()}, mean {mean.tolist()}, se {se.tolist()}, z {((mean - want) / se).tolist()}, "
          f"sd / mean {(sd / mean).tolist()}, events {events(tr)}")
    assert (np.abs(mean - want) <= 5 * se).all()
    assert abs(ratio - et.RATIO[name][0]) <= 0.005, (ratio, et.RATIO[name])
    # the estimator is at work: samples arrive, escapes are weighted, and no density is 0 where a sample lands
    assert len(tr.nee_free) >= N // 4 and len(tr.escapes_weighted) >= N // 2 and not tr.escapes_plain and not tr.zero_pdf
    assert sorted(tr.below + paths_of(tr.nee_free) + paths_of(tr.nee_occluded)) == list(range(N))


@pytest.mark.parametrize("name", et.UNSAMPLED_TOO)
def test_the_unsampled_models_mean_is_the_closed_form(crt, name):
    w = et.world(crt, name)
    rgb = em.ray_color(orc, w.d, w.rays(N), ps.default_states(SEED, N), 2, et.BG, et.T_MIN, env=w.env, crt=crt)[0]
    want = w.expected()
    mean, se = rgb.mean(0), rgb.std(0, ddof=1) / math.sqrt(N)
    print(f"{name} unsampled: mean {mean.tolist()}, z {((mean - want) / se).tolist()}, sd / mean {(se * math.sqrt(N) / mean).tolist()}")
    assert (np.abs(mean - want) <= 5 * se).all()


@pytest.mark.parametrize("depth", [2, 8])
def test_glass_pair_ratio(crt, depth):
    w = et.world(crt, "glass")
    st = ps.default_states(SEED2, N2)
    flat = em.ray_color(orc, w.d, w.rays(N2), st, depth, et.BG, et.T_MIN, env=w.env, crt=crt)[0]
    _, nee, _, tr = modelled(crt, "glass", depth, st, "pair")
    m0, m1 = flat.mean(0), nee.mean(0)
    v0, v1 = flat.var(0, ddof=1), nee.var(0, ddof=1)
    ratio = float((np.sqrt(v0 + v1) / m0).max())
    se = np.sqrt((v0 + v1) / N2)
    print(f"glass at depth {depth}: unsampled {m0.tolist()}, sampled {m1.tolist()}, z {((m1 - m0) / se).tolist()}, pair ratio {ratio:.4f}, "
          f"events {events(tr)}")
    assert (np.abs(m0 - m1) <= 5 * se).all()
    assert abs(ratio - et.RATIO2[depth][0]) <= 0.005, (ratio, et.RATIO2[depth])
    assert {k for _, k in tr.nee_occluded} == {em.DIELECTRIC} and len(tr.nee_occluded) >= 200  # glass stops shadow rays
    if depth == 2:
        assert not tr.escapes_plain  # the sphere ends every path that meets it
    else:  # paths cross the glass and leave with pb none: f = 1, as many as a quarter of all
        assert len(tr.escapes_plain) >= N2 // 8 and len(tr.escapes_weighted) >= N2 // 2


def test_every_recorded_n_meets_its_condition():
    assert set(et.RATIO) == set(STATISTICAL) and set(et.RATIO2) == {2, 8}
    for table, share in ((et.RATIO, 0.01), (et.RATIO2, 0.02)):
        for name, (ratio, log2n) in table.items():
            assert et.n_for(ratio, share) == (log2n, True) and log2n <= 20, (name, ratio, log2n)


# ---- 3. the events --------------------------------------------------------------------------------------
def test_samples_below_the_horizon_get_no_ray(crt):
    for name in et.CLOSED:
        w, rgb, _, tr = seeded(crt, name)
        assert len(tr.below) >= (N // 64 if name == "sun" else N // 3), (name, len(tr.below))
        assert tr.nee_skipped == tr.below  # nothing but the horizon skips a sample on these maps
        nrm = np.array(w.n)
        d = {i: np.array(ds) for i, _, _, _, ds in tr.picks}
        assert all(d[i] @ nrm <= 0 for i in tr.below[:500]) and all(d[i] @ nrm > 0 for i in paths_of(tr.nee_free)[:500])
    _, _, _, tr = seeded(crt, "sun_horizon")  # the horizon halves the bright texel: its samples split evenly
    sun_row = et.SUN_HORIZON_AT[0]
    sun = [i for i, r, k, _, _ in tr.picks if (r, k) == et.SUN_HORIZON_AT]
    under = len(set(sun) & set(tr.below))
    assert len(sun) >= 0.95 * N and abs(under - len(sun) / 2) <= 5 * math.sqrt(len(sun)) / 2, (len(sun), under, sun_row)


def test_occluded_by_the_roof_and_by_the_ball(crt):
    for name, least in (("roof", N // 20), ("ball", N // 100), ("ball_spheres", N // 100)):
        w, _, ended, tr = seeded(crt, name)
        assert len(tr.nee_occluded) >= least and {k for _, k in tr.nee_occluded} == {em.LAMBERTIAN}, (name, events(tr))
        assert (ended == em.DEPTH).sum() >= least  # bounces that end on the occluder gather nothing
        picks = {i: (r, k) for i, r, k, _, _ in tr.picks}
        n = w.env.n
        rows, cols = et.ROOF_BLOCK if name == "roof" else et.BALL_BLOCK
        block = {(2 * n + r, c) for r in rows for c in cols}
        assert {picks[i] for i, _ in tr.nee_occluded} <= block  # only samples of the block behind it are stopped
        if name == "roof":  # and every sample of that block is
            assert not {picks[i] for i in paths_of(tr.nee_free)} & block
    assert not seeded(crt, "random")[3].nee_occluded


# ---- 4. crafted states ----------------------------------------------------------------------------------
CRAFTED = {("xi1", "max"): 0x7E33F89B, ("xi2", "max"): 0x72E9A72C, ("xi3", "max"): 0xD39AD4C1, ("xi4", "max"): 0xDBFE206A}


def crafted(crt, name):
    w = et.world(crt, name)
    cs = et.crafted_states(crt, w)
    assert cs == CRAFTED
    keys = list(cs)
    _, rgb, ended, tr = modelled(crt, name, 2, np.array([cs[k] for k in keys], np.uint32), "crafted")
    picks = {keys[i][0]: (i, r, k, xi, np.array(ds)) for i, r, k, xi, ds in tr.picks}
    for j, which in enumerate(("xi1", "xi2", "xi3", "xi4")):
        assert picks[which][3][j] == et.RND01_OF_MAX > 1
    return w, tr, picks


def test_zero_never_follows_a_lambertian_scatter(crt):
    """xi1 .. xi4 follow the scatter's accepted triple by 1 .. 4 draws. The triples that end 1 .. 4 draws
    before the state 0 all lie outside the unit ball, so the rejection loop never ends there."""
    for j in range(4):
        s = et.states_reaching(0, 3 + j + 1)
        v = []
        for _ in range(3):
            s, x = crt.rand_double(s, -1.0, 1.0)
            v.append(x)
        assert sum(x * x for x in v) >= 1, (j, v)
    assert crt.rand_double(et.lcg_prev(0), 0.0, 1.0) == (0, 0.0)


def test_a_draw_above_one_clamps_onto_the_last_row(crt):
    w, tr, picks = crafted(crt, "half_black")
    n = w.env.n
    i, r, k, xi, ds = picks["xi1"]
    tb = nm.tables(w.env)
    assert (r, k) == (6 * n - 1, n - 1) and tb.w[r, k] == 0 and tb.c[r, n - 1] == 0  # an empty row: the count is n, clamped
    assert ds @ np.array(w.n) > 0 and tr.zero_pdf == [i] and i not in tr.below  # above the horizon, and no ray
    assert tb.m[0] == 0 and nm.pick(w.env, tb, [0.0], [0.0])[0][0] == 1  # xi1 = 0 skips the empty first row
    _, _, _, seeded_tr = seeded(crt, "half_black")
    assert not seeded_tr.zero_pdf and not {r for _, r, _, _, _ in seeded_tr.picks} & set(et.HALF_BLACK_ROWS)


def test_a_draw_above_one_at_the_last_column_lands_on_the_next_face(crt):
    for name in ("sun", "sun_horizon", "random", "tilted", "under", "roof", "ball", "glass"):
        w, tr, picks = crafted(crt, name)
        n = w.env.n
        for which, axis in (("xi3", 0), ("xi4", 1)):
            i, r, k, xi, ds = picks[which]
            ok, face, u, v, h, fx, fy = nm.project(w.env, [ds])
            print(f"{name} {which} = max: picked row {r} column {k}, d_s projects to face {int(face[0])} fx {float(fx[0])!r} fy {float(fy[0])!r}")
            at = (k if axis == 0 else r % n) + 1
            if at < n:  # one texel on: 2.3e-10 of a texel past the edge
                assert int(face[0]) == r // n and math.floor(float((fx, fy)[axis][0])) == at
            else:
                assert int(face[0]) != r // n
    w, tr, picks = crafted(crt, "sun")
    i, r, k, xi, ds = picks["xi3"]
    n = w.env.n
    tb = nm.tables(w.env)
    assert (r, k) == et.SUN_AT and k == n - 1 and nm.project(w.env, [ds])[1][0] == 5  # +X's last column: past it lies -Z
    # the sample sees a dim texel and is weighted with that texel's density, not the sun's
    assert i in paths_of(tr.nee_free) and float(nm.pdf(w.env, tb, [ds])[0]) < 1e-3 * float(nm.pdf(w.env, tb, [et.direction(w.env, 0, 0.9, -0.6)])[0])
    assert (em.lookup(w.env, [ds])[0] == 0.5).all()


def test_samples_are_the_forward_maps_directions_on_every_face(crt, host):  # noqa: F811
    """env_sample's direction, the model's and the host-compiled header's, is the CUBE table's direction of the
    (face, u, v) it picked, times the basis: a face of its table that differs from include/crt_render.h's shows
    here, whatever env_project does."""
    for name in ("random", "tilted", "half_black"):
        w = et.world(crt, name)
        n = w.env.n
        tb = nm.tables(w.env)
        xi = np.random.default_rng(9).random((1200, 4))
        r, k = nm.pick(w.env, tb, xi[:, 0], xi[:, 1])
        assert set((r // n).tolist()) == set(range(6))
        g = 2.0 / n
        want = np.array([et.direction(w.env, int(r[j] // n), np.array((k[j] + xi[j, 2]) * g - 1.0), np.array((r[j] % n + xi[j, 3]) * g - 1.0))
                         for j in range(len(xi))])
        for got in (nm.sample(w.env, tb, xi[:, 0], xi[:, 1], xi[:, 2], xi[:, 3]), host.sample(w.env, tb, xi)):
            assert np.abs(got - want).max() <= 1e-15, name
        # and the density asked of that direction is the picked texel's own: project inverts the table
        ok, face, u, v, h, fx, fy = nm.project(w.env, want)
        assert ok.all() and np.array_equal(face, r // n) and np.array_equal(np.floor(fx).astype(int), k)
        assert np.array_equal(np.floor(fy).astype(int), r % n)


def test_zero_draws_lie_on_the_texels_first_edge_and_ties_take_the_rules_face(crt, host):  # noqa: F811
    for name in ("random", "tilted"):
        w = et.world(crt, name)
        n = w.env.n
        tb = nm.tables(w.env)
        rng = np.random.default_rng(7)
        xi = rng.random((600, 4))
        xi[:200, 2] = 0.0
        xi[200:400, 3] = 0.0
        xi[400:, 2:] = 0.0
        got = host.sample(w.env, tb, xi)
        r, k = nm.pick(w.env, tb, xi[:, 0], xi[:, 1])
        g = 2.0 / n
        edges = ties = 0
        for j in range(len(xi)):
            u, v = (k[j] + xi[j, 2]) * g - 1.0, (r[j] % n + xi[j, 3]) * g - 1.0
            want = et.direction(w.env, int(r[j] // n), np.array(u), np.array(v))  # the forward map, nothing inverted
            assert np.abs(got[j] - want).max() <= 1e-15, (name, j)
            on_edge = (xi[j, 2] == 0 and k[j] == 0) or (xi[j, 3] == 0 and r[j] % n == 0)
            if on_edge:
                edges += 1
                ok, face, pu, pv, h, fx, fy = nm.project(w.env, [got[j]])
                p = host.pdf(w.env, tb, [got[j]])[0]
                assert ok[0] and p > 0 and math.isfinite(p)
                ties += int(face[0]) != r[j] // n
                if int(face[0]) != r[j] // n:  # the tie went to the neighbour: its density, an edge texel's of that face
                    col = min(max(math.floor(float(fx[0])), 0), n - 1)
                    row = min(max(math.floor(float(fy[0])), 0), n - 1)
                    assert col in (0, n - 1) or row in (0, n - 1)
        print(f"{name}: {edges} zero draws on a face edge, {ties} of them projected onto the neighbouring face")
        assert edges >= 20 and (ties >= 1 or name == "tilted")


# ---- 5. the probes' own estimators ----------------------------------------------------------------------
def test_probe_estimators_have_the_closed_forms_moments(crt):
    rng = np.random.default_rng(8)
    count = 1 << 16
    u = rng.normal(size=(count, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    for name in ("random", "tilted"):
        w = et.world(crt, name)
        L = em.lookup(w.env, np.array(w.n) + u, et.BG)  # cosine about n
        mean, sd = L.mean(0), L.std(0, ddof=1)
        want = w.irradiance()
        print(f"{name}: cosine estimator mean {mean.tolist()} against sum L F {want.tolist()}, sd / mean {(sd / mean).max():.4f} against {et.cosine_ratio(w):.4f}")
        assert (np.abs(mean - want) <= 5 * sd / math.sqrt(count)).all()
        assert abs((sd / mean).max() - et.cosine_ratio(w)) <= 0.01
        assert et.n_for(et.cosine_ratio(w), 0.01) == (et.PROBE_LOG2_S[name], True)
    w = et.world(crt, "random")
    m, sd = et.sphere_moments(w.env)
    terms = 4 * math.pi * et.sh_basis(u)[:, :, None] * em.lookup(w.env, u, et.BG)[:, None, :]
    z = (terms.mean(0) - m) / (terms.std(0, ddof=1) / math.sqrt(count))
    print(f"sphere estimator: z {np.round(z, 2).tolist()}, sd ratio {np.round(terms.std(0, ddof=1) / sd, 3).tolist()}")
    assert (np.abs(z) <= 5).all() and (np.abs(terms.std(0, ddof=1) / sd - 1) <= 0.03).all()
    assert et.n_for(float((sd[0] / m[0]).max()), 0.01) == (et.PROBE_LOG2_S["sphere"], True)
