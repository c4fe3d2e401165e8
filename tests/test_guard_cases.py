"""The range-guard cases (tests/guard_cases.py) hold what they claim, shown without a GPU: for every
case the centre rays' a = dot(d, d), min / max |d_k| and |o_k|, the scene's largest record and bound,
|sn|_1 of its parallelograms and (Ladder A) the discriminants of the oracle's first hits fall on the
claimed side of the named guard; every guard has a case strictly inside and one strictly outside,
within a factor 8 of the bound; and no case is vacuous: the oracle's frame is finite and differs from
the background in at least a quarter of its pixels.

Two facts about the reference that the table has to live with, both established here:
- Parallelogram::hit_by misses when |dot(unit normal, d)| < 1e-9, an absolute cutoff. On Ladder A
  from F = 2^-31 down (|d| <= 1.1 F < 1e-9) no primary ray hits a parallelogram: the frames of the
  two parallelogram-only families are the background exactly (asserted, instead of the quarter), the
  mixed family keeps its spheres (and the quarter), and only the sphere family's Ladder A frames are
  bit-identical to its base frame; the other families' are bit-identical to one another from
  F = 2^-31 down.
- |sn|_1 >= 2^-64 (quad_record) cannot fail alone: sides within 2^30 give |s1 x s2| <= 3 * 2^60, so
  |sn|_1 >= 1 / |n| >= 2^-61.6. Its outside cases (s = 36) are outside the 2^30 record bound too."""
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import crt_oracle_py as orc  # noqa: E402
import denoise_model as dm  # noqa: E402
import guard_cases as gc  # noqa: E402

BG = np.array(gc.BACKGROUND)
_cache = {}


def facts(crt, case, fam):
    """(the oracle's frame, the measured quantities) of a case and family, computed once."""
    key = (case.id, fam)
    if key not in _cache:
        d = gc.scene(crt, fam, case.s, case.e, case.cam)
        frame = orc.render(d, gc.BASE_SEED, threads=8)
        cam = crt.resolve_camera(d.camera, 0)
        hits = orc.hits(d, dm.centre_rays(cam).reshape(-1, 6), cam.t_min)
        _cache[key] = frame, gc.measure(crt, d, hits)
    return _cache[key]


def applies(guard, fam):
    if guard == "sqrt_lo":
        return fam in ("spheres", "mixed")  # discriminants of spheres
    if guard.startswith("sn1"):
        return fam != "spheres"
    return True


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.id)
def test_case_is_on_its_side_and_not_vacuous(crt, case):
    for fam in case.families:
        frame, m = facts(crt, case, fam)
        assert np.isfinite(frame).all(), fam
        share = float((np.abs(frame - BG).max(-1) > 0).mean())
        if gc.quads_cut(case) and fam in ("flat", "rotated"):
            assert share == 0.0, (fam, share)  # the reference's 1e-9 cutoff: see the module docstring
        else:
            assert share >= 0.25, (fam, share)
        for guard, want in case.claimed(fam).items():
            if applies(guard, fam):
                got, q = gc.side(guard, m)
                print(f"{case.id} {fam} {guard}: {got}, 2^{gc.log2(q):.1f} vs 2^{gc.log2(gc.GUARDS[guard][0]):.0f}")
                assert got == want, (fam, guard, got, q)


def test_every_guard_has_a_case_on_each_side_within_a_factor_8(crt):
    for guard, (bound, _) in gc.GUARDS.items():
        for fam in gc.FAMILIES:
            if not applies(guard, fam):
                continue
            near = {}
            for case in gc.CASES:
                if fam in case.families and guard in case.claimed(fam):
                    got, q = gc.side(guard, facts(crt, case, fam)[1])
                    assert got == case.claimed(fam)[guard]
                    r = max(q / bound, bound / q)
                    near[got] = min(near.get(got, np.inf), r)
                    print(f"{guard:10s} {fam:8s} {got:3s} {case.id:22s} 2^{gc.log2(q):.1f}")
            assert set(near) == {"in", "out"}, (guard, fam, near)
            if guard != "sn1_lo":  # not reachable alone: see the module docstring
                assert near["in"] <= 8 and near["out"] <= 8, (guard, fam, near)
    # strictly: no deciding quantity sits on a bound, except d_z = -2^30 exactly (allowed: <=)
    m = facts(crt, gc.BY_ID["B-s12-e30-origin"], "spheres")[1]
    assert m["dmax_max"] == 2.0 ** 30 and m["a_min"] > 2.0 ** 60


def test_sn1_restated_from_the_constructor_matches_the_scale(crt):
    """|sn|_1 = |n|_1 / |n|^2 with n = s1 x s2 scales as S^-2 exactly (powers of two)."""
    for fam in gc.QUADS:
        m0 = gc.measure(crt, gc.scene(crt, fam, 0, 0, "offset"))
        m1 = gc.measure(crt, gc.scene(crt, fam, -21, -21, "offset"))
        assert m1["sn1_max"] == m0["sn1_max"] * 2.0 ** 42 and m1["sn1_min"] == m0["sn1_min"] * 2.0 ** 42
        assert 2.0 ** -8 < m0["sn1_min"] <= m0["sn1_max"] < 2.0 ** 2


def test_ladder_a_frames_do_not_see_the_scale(crt):
    ladder = [c for c in gc.CASES if c.ladder == "A"]
    base, cut = gc.BY_ID["A-s0-e0-origin"], gc.BY_ID["A-s0-e-31-origin"]
    for case in ladder:
        assert dm.bits(facts(crt, case, "spheres")[0]).tobytes() == dm.bits(facts(crt, base, "spheres")[0]).tobytes(), case
        for fam in gc.QUADS:
            if gc.quads_cut(case):
                assert dm.bits(facts(crt, case, fam)[0]).tobytes() == dm.bits(facts(crt, cut, fam)[0]).tobytes(), (case, fam)
    for fam in gc.QUADS:  # and the cutoff does change what the base frame shows
        assert not np.array_equal(facts(crt, cut, fam)[0], facts(crt, base, fam)[0])


def test_closest_hit_rays_scale_exactly_in_the_oracle(crt):
    """orc.hits of the closest-hit rays with directions times 2^k and t_min times 2^-k: the sphere
    family's hits are the k = 0 hits with t times 2^-k, bit for bit, for every k of the GPU test;
    the families with parallelograms for k >= 0 (below, the 1e-9 cutoff drops parallelograms)."""
    for fam in gc.FAMILIES:
        d = gc.scene(crt, fam)
        rays = gc.closest_hit_rays(fam)
        base = orc.hits(d, rays, 1e-5)
        hit = base["prim"] >= 0
        print(fam, "hit share", hit.mean())
        assert 0.15 < hit.mean() < 0.9, (fam, hit.mean())
        assert (rays[:, 3:] == 0).any(1).mean() > 0.03
        for k in gc.HIT_SCALES:
            if k < 0 and fam != "spheres":
                continue
            r = rays.copy()
            r[:, 3:] *= 2.0 ** k
            got = orc.hits(d, r, 1e-5 * 2.0 ** -k)
            assert np.array_equal(got["prim"], base["prim"]), (fam, k)
            assert np.array_equal(dm.bits(got["t"][hit] * 2.0 ** k), dm.bits(base["t"][hit])), (fam, k)
            for name in ("point", "normal"):
                assert np.array_equal(dm.bits(got[name][hit]), dm.bits(base[name][hit])), (fam, k, name)
