"""CPU-side checks of tests/env_nee_model.py, the restatement the GPU tests of luminance-sampled
environments (tests/test_gpu_env_nee.py) hold the kernels to. No kernel runs here.

  - csrc/crt_env_sampler.h compiled for the host gives the model's bits for the tables, env_pdf and
    env_sample, the `<=` rule at exact table entries and the numbers 0 and the largest rnd_01 included;
  - env_pdf is the density env_sample draws with: the mean of 1 / env_pdf over its draws is 4 pi;
  - a Lambertian plane under a map of equal texels: NEE and the escape integrate to albedo * L;
  - the two identities with the unsampled estimator (no Lambertian bounce; max_depth == 1), bit for bit;
  - the sampled and the unsampled estimator agree in the mean, and under a map with one bright texel
    the sampled one has the lower per-path variance.

Bounds: a mean of N independent values is held to 5 standard errors of that mean, the standard error
estimated from the same N values (a normal tail of 6e-7 a comparison); for two estimators the two
standard errors are combined in quadrature.
"""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import env_model as em
import env_nee_model as nm
import probe_sets as ps
from conftest import ROOT
from oracle import crt_oracle_py as orc
from test_env_model import ROTATED, integer_map, probe_directions

RND01_MAX = float(0xFFFFFFFF) * (1 / float(4294967295 - 1))  # rnd_01 of the state 0xFFFFFFFF: above 1
SIZES = (1, 2, 5, 8)
BASES = [dict(), ROTATED]


def special_maps(n, seed):
    """name -> texels: a random positive map, whole zero rows (the first and the last among them), zero
    leading and trailing columns, one non-zero texel, and odd values (-0.0, negatives, NaN)."""
    rng = np.random.default_rng(seed)
    base = rng.random((6 * n, n, 3)) * 4.0 + 0.01
    out = {"random": base}
    rows = base.copy()
    rows[[0, 6 * n - 1]] = 0.0
    rows[rng.permutation(6 * n)[:2 * n]] = 0.0
    out["zero_rows"] = rows
    cols = base.copy()
    cols[:, 0] = 0.0
    cols[:, n - 1] = 0.0
    out["zero_edge_columns"] = cols
    one = np.zeros_like(base)
    one[(7 * n) // 2 % (6 * n), n // 2] = (0.5, 2.0, 1.0)
    out["one_texel"] = one
    odd = base.copy()
    flat = odd.reshape(-1)
    where = rng.permutation(flat.size)[:flat.size // 3]
    flat[where] = np.array([-0.0, -1.5, np.nan, 0.0, -1e-3])[np.arange(len(where)) % 5]
    out["odd_values"] = odd
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = tmp_path_factory.mktemp("env_sampler") / "env_sampler_check.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                        f"-I{ROOT / 'cpp_raytracer_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "env_sampler_check.cpp"),
                        "-o", str(so)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(so))
    vp = C.c_void_p
    lib.env_tables_host.argtypes = [vp, vp, vp, vp]
    lib.env_pdf_many.argtypes = [vp, vp, vp, vp, C.c_double, vp, C.c_size_t, vp]
    lib.env_sample_many.argtypes = [vp, vp, vp, vp, C.c_double, vp, C.c_size_t, vp]
    for f in (lib.env_tables_host, lib.env_pdf_many, lib.env_sample_many):
        f.restype = None

    class Host:
        @staticmethod
        def view(env):
            from cpp_raytracer_amd import _capi
            D3 = _capi.D3
            t = np.ascontiguousarray(env.texels, np.float64)
            return t, _capi.EnvView(t.ctypes.data, env.n, env.filter, D3(*env.right), D3(*env.up), D3(*env.forward))

        @staticmethod
        def tables(env):
            t, v = Host.view(env)
            n = env.n
            w, c, m = np.full((6 * n, n), np.nan), np.full((6 * n, n), np.nan), np.full(6 * n, np.nan)
            lib.env_tables_host(C.addressof(v), w.ctypes.data, c.ctypes.data, m.ctypes.data)
            return nm.Tables(w, c, m, float(m[-1]))

        @staticmethod
        def pdf(env, tb, dirs):
            t, v = Host.view(env)
            d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
            out = np.full(len(d), np.nan)
            lib.env_pdf_many(C.addressof(v), tb.w.ctypes.data, tb.c.ctypes.data, tb.m.ctypes.data, tb.W, d.ctypes.data,
                             len(d), out.ctypes.data)
            return out

        @staticmethod
        def sample(env, tb, xi):
            t, v = Host.view(env)
            x = np.ascontiguousarray(xi, np.float64).reshape(-1, 4)
            out = np.full((len(x), 3), np.nan)
            lib.env_sample_many(C.addressof(v), tb.w.ctypes.data, tb.c.ctypes.data, tb.m.ctypes.data, tb.W,
                                x.ctypes.data, len(x), out.ctypes.data)
            return out
    return Host


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def exact_numbers(env, tb, rng, count):
    """(xi (count, 4), how many xi1 * W equal an m entry exactly, how many xi2 * rowsum equal a c entry):
    numbers aimed at table entries, kept where the product lands on the entry exactly."""
    n = env.n
    xi = rng.random((count, 4))
    rows = rng.integers(0, 6 * n, count)
    x1 = tb.m[rows] / tb.W
    hit1 = x1 * tb.W == tb.m[rows]
    xi[hit1, 0] = x1[hit1]
    r, _ = nm.pick(env, tb, xi[:, 0], np.zeros(count))
    cols = rng.integers(0, n, count)
    total = tb.c[r, n - 1]
    with np.errstate(all="ignore"):
        x2 = tb.c[r, cols] / total
        hit2 = (total > 0) & (x2 * total == tb.c[r, cols])
    xi[hit2, 1] = x2[hit2]
    # the rule itself: an entry equal to the product is counted, so the pick lies beyond it (or is clamped)
    r2, k2 = nm.pick(env, tb, xi[:, 0], xi[:, 1])
    assert (r2[hit1] >= np.minimum(rows[hit1] + 1, 6 * n - 1)).all()
    assert (k2[hit2] >= np.minimum(cols[hit2] + 1, n - 1)).all()
    return xi, int(hit1.sum()), int(hit2.sum())


# ---- the host header --------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", BASES, ids=["default", "rotated"])
@pytest.mark.parametrize("n", SIZES)
def test_the_kernels_sampler_is_the_models_on_the_host(host, n, basis):
    rng = np.random.default_rng(100 + n)
    dirs = np.concatenate([probe_directions(), np.array([(0.0, 0.0, 0.0), (math.nan, 1.0, 0.0), (0.0, math.inf, 0.0),
                                                         (1.7e308, 1.7e308, -1.7e308)])])
    usable, exact1, exact2 = 0, 0, 0
    for name, texels in special_maps(n, 200 + n).items():
        env = em.make(texels, filter=em.BILINEAR if n % 2 else em.NEAREST, **basis)
        tb = nm.tables(env)
        got = host.tables(env)
        assert same(got.w, tb.w) and same(got.c, tb.c) and same(got.m, tb.m), (n, name)
        assert (tb.w >= 0).all() and not np.signbit(tb.w).any()  # NaN, negatives and -0.0 weigh +0
        if not nm.usable(tb):
            continue
        usable += 1
        assert same(host.pdf(env, tb, dirs), nm.pdf(env, tb, dirs)), (n, name)
        xi, h1, h2 = exact_numbers(env, tb, rng, 512)
        exact1, exact2 = exact1 + h1, exact2 + h2
        ends = np.array([(a, b, c, d) for a in (0.0, RND01_MAX) for b in (0.0, RND01_MAX) for c in (0.0, RND01_MAX)
                         for d in (0.0, RND01_MAX)])
        xi = np.concatenate([xi, ends, rng.random((256, 4))])
        want = nm.sample(env, tb, xi[:, 0], xi[:, 1], xi[:, 2], xi[:, 3])
        assert same(host.sample(env, tb, xi), want), (n, name)
        # a draw lands in the texel it picked: its density is that texel's weight, positive unless
        # the pick was clamped onto an empty texel (those are skipped)
        r, k = nm.pick(env, tb, xi[:, 0], xi[:, 1])
        inside = (xi[:, 2] > 0) & (xi[:, 2] < 1) & (xi[:, 3] > 0) & (xi[:, 3] < 1) & (tb.w[r, k] > 0)
        assert (nm.pdf(env, tb, want[inside]) > 0).all(), (n, name)
    assert usable >= 2 and exact1 > 0
    assert exact2 > 0 or n == 1


def test_rnd01_max_is_the_packages(crt):
    assert crt.rand_double(_state_before(0xFFFFFFFF), 0.0, 1.0) == (0xFFFFFFFF, RND01_MAX)
    assert RND01_MAX > 1.0


def _state_before(s):
    """The LCG state whose successor is s: s = 1664525 * p + 1013904223 mod 2^32."""
    inv = pow(1664525, -1, 1 << 32)
    return ((s - 1013904223) * inv) % (1 << 32)


@pytest.mark.parametrize("n", SIZES)
def test_projection_is_env_models(n):
    """project's face, row and column are the ones env_model.lookup reads under NEAREST."""
    t = np.zeros((6 * n, n, 3))
    t[:, :, 0] = np.arange(6 * n)[:, None]
    t[:, :, 1] = np.arange(n)[None, :]
    for basis in BASES:
        env = em.make(t, filter=em.NEAREST, **basis)
        dirs = probe_directions()
        ok, face, u, v, h, fx, fy = nm.project(env, dirs)
        seen = em.lookup(env, dirs, (-1.0, -1.0, -1.0))
        assert np.array_equal(ok, seen[:, 0] >= 0)
        row = np.clip(np.floor(fy[ok]).astype(np.int64), 0, n - 1)
        col = np.clip(np.floor(fx[ok]).astype(np.int64), 0, n - 1)
        assert np.array_equal(face[ok] * n + row, seen[ok, 0].astype(np.int64))
        assert np.array_equal(col, seen[ok, 1].astype(np.int64))


# ---- the density ------------------------------------------------------------------------------------------
def test_pdf_is_the_density_of_the_draws():
    rng = np.random.default_rng(5)
    env = em.make(rng.random((24, 4, 3)) * 4.0 + 0.05, **ROTATED)
    tb = nm.tables(env)
    xi = rng.random((200_000, 4))
    d = nm.sample(env, tb, xi[:, 0], xi[:, 1], xi[:, 2], xi[:, 3])
    p = nm.pdf(env, tb, d)
    assert (p > 0).all()
    inv = 1.0 / p
    mean, se = float(inv.mean()), float(inv.std(ddof=1) / math.sqrt(len(inv)))
    print(f"mean 1 / env_pdf = {mean:.6f} (4 pi = {4 * math.pi:.6f}), standard error {se:.3g}")
    assert abs(mean - 4 * math.pi) <= 5 * se


# ---- a plane under a uniform sky ---------------------------------------------------------------------------
def plane_world(crt, albedo):
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE
    mats = np.zeros(1, MATERIAL_DTYPE)
    mats["kind"], mats["color"], mats["param"] = em.LAMBERTIAN, [albedo], 0.0
    objs = np.zeros(1, OBJECT_DTYPE)
    objs["kind"] = 2
    objs["v"][0] = [-1000.0, 0.0, -1000.0, 2000.0, 0.0, 0.0, 0.0, 0.0, 2000.0]
    d = crt.SceneData.named("config1")
    d.materials, d.objects = mats, objs
    return d


def test_plane_under_equal_texels_gathers_albedo_times_L(crt):
    albedo, L = (0.5, 0.75, 0.25), (1.0, 2.0, 3.0)
    d = plane_world(crt, albedo)
    env = em.make(np.broadcast_to(np.array(L), (24, 4, 3)).copy(), **ROTATED)
    tb = nm.tables(env)
    rng = np.random.default_rng(11)
    count = 4096
    o = np.stack([rng.uniform(-5, 5, count), np.full(count, 3.0), rng.uniform(-5, 5, count)], 1)
    dirs = np.stack([rng.normal(0, 0.5, count), np.full(count, -1.0), rng.normal(0, 0.5, count)], 1)
    rgb, ended, tr = nm.ray_color(orc, d, np.concatenate([o, dirs], 1), ps.states(count, 12), 2, (9.0, 9.0, 9.0), 1e-5,
                                  env, tb, crt=crt)
    assert (ended == em.MISS).all()  # hit the plane, bounced, left
    assert not tr.nee_occluded and len(tr.escapes_weighted) == count and not tr.escapes_plain
    assert len(tr.nee_free) + len(tr.nee_skipped) == count and len(tr.nee_free) > count // 4
    want = np.array(albedo) * np.array(L)
    mean, se = rgb.mean(0), rgb.std(0, ddof=1) / math.sqrt(count)
    print(f"plane: mean / (albedo L) = {(mean / want).tolist()}, standard errors {(se / want).tolist()}")
    assert (np.abs(mean - want) <= 5 * se).all()
    # the unsampled estimator gathers albedo * L on every path (every escape sees L): the same mean
    flat = em.ray_color(orc, d, np.concatenate([o, dirs], 1), ps.states(count, 12), 2, (9.0, 9.0, 9.0), 1e-5, env=env, crt=crt)[0]
    assert np.allclose(flat, want, rtol=1e-15)


# ---- the identities ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtow_final", "mixed", "rtow_final_lights"])
def test_identities_with_the_unsampled_estimator(crt, name):
    d, _ = ps.world(crt, name)
    p = ps.probe(crt, name, "S")
    rays, states = p.rays[:1024], p.states[:1024]
    env = em.make(np.random.default_rng(3).random((30, 5, 3)) * 4.0, **ROTATED)
    tb = nm.tables(env)
    # max_depth == 1: every path
    want = em.ray_color(orc, d, rays, states, 1, ps.BG, p.t_min, env=env, crt=crt)[0]
    got, _, tr = nm.ray_color(orc, d, rays, states, 1, ps.BG, p.t_min, env, tb, crt=crt)
    assert same(got, want)
    assert not tr.nee_free and not tr.nee_occluded and not tr.escapes_weighted
    # any depth: the paths that never scatter off a Lambertian
    # (the four numbers of a Lambertian bounce move the state, so the other paths differ from there on)
    want = em.ray_color(orc, d, rays, states, 50, ps.BG, p.t_min, env=env, crt=crt)[0]
    got, _, tr = nm.ray_color(orc, d, rays, states, 50, ps.BG, p.t_min, env, tb, crt=crt)
    plain = np.ones(len(rays), bool)
    plain[list(tr.lambertian)] = False
    assert plain.sum() >= 50 and (~plain).sum() >= 50, plain.sum()
    assert same(got[plain], want[plain])
    assert (want[plain] != 0).any() and not same(got[~plain], want[~plain])


# ---- against the unsampled estimator ----------------------------------------------------------------------
def brightest_escape_texel(env, last):
    """(row, col, how many of the directions land there) of the texel most of them land in."""
    ok, face, u, v, h, fx, fy = nm.project(env, last)
    n = env.n
    row = face[ok] * n + np.clip(np.floor(fy[ok]).astype(np.int64), 0, n - 1)
    col = np.clip(np.floor(fx[ok]).astype(np.int64), 0, n - 1)
    flat = np.bincount(row * n + col, minlength=6 * n * n)
    best = int(flat.argmax())
    return best // n, best % n, int(flat[best])


@pytest.mark.parametrize("name,filt", [("cornell", em.NEAREST), ("rtow_final", em.BILINEAR)])
def test_sampled_and_unsampled_estimators_agree_and_the_sampled_one_is_quieter(crt, name, filt):
    d, _ = ps.world(crt, name)
    s, v = ps.probe(crt, name, "S"), ps.probe(crt, name, "V")
    rays = np.concatenate([s.rays[:2048], v.rays[:1024]])
    states = np.concatenate([s.states[:2048], v.states[:1024]])
    n, depth = 8, 50
    dull = em.make(np.full((6 * n, n, 3), 0.5), filter=filt, **ROTATED)
    _, ended, last, _ = em.ray_color(orc, d, rays, states, depth, ps.BG, 1e-5, env=dull, crt=crt)
    after = (ended == em.MISS) & (np.array(last) != rays[:, 3:]).any(1)
    row, col, count = brightest_escape_texel(dull, last[after])
    assert count >= 1  # the unsampled estimator alone finds the bright texel at these seeds and counts
    t = np.full((6 * n, n, 3), 0.5)
    t[row, col] = 1e4
    env = em.make(t, filter=filt, **ROTATED)
    tb = nm.tables(env)
    flat = em.ray_color(orc, d, rays, states, depth, ps.BG, 1e-5, env=env, crt=crt)[0]
    nee, _, tr = nm.ray_color(orc, d, rays, states, depth, ps.BG, 1e-5, env, tb, crt=crt)
    assert tr.nee_free and tr.nee_occluded and tr.escapes_weighted
    N = len(rays)
    m0, m1 = flat.mean(0), nee.mean(0)
    v0, v1 = flat.var(0, ddof=1), nee.var(0, ddof=1)
    se = np.sqrt(v0 / N + v1 / N)
    print(f"{name}: {count} of {int(after.sum())} bounced escapes land in the bright texel ({row}, {col}); means unsampled "
          f"{m0.tolist()} sampled {m1.tolist()}, combined standard errors {se.tolist()}; per-path variance "
          f"unsampled / sampled = {(v0 / v1).tolist()}")
    assert (np.abs(m0 - m1) <= 5 * se).all()
    assert (v1 < v0).all()
    # a first segment that leaves the scene sees the texel directly, with f = 1 in both estimators: the
    # variance those paths carry is common to both. Over the paths that start with a hit:
    hit = orc.hits(d, rays, 1e-5)["prim"] >= 0
    assert same(flat[~hit], nee[~hit])
    r = flat[hit].var(0, ddof=1) / nee[hit].var(0, ddof=1)
    print(f"{name}: over the {int(hit.sum())} paths whose first segment hits, per-path variance unsampled / sampled = {r.tolist()}")
    assert (r > 1).all()
