"""tests/lighting_truth.py checked without a GPU: the model's mean over 2^14 paths agrees with each
world's closed form within 5 standard errors, and the per-path sd / mean and the N it gives are the ones
recorded in lighting_truth.RATIO, which the GPU test (tests/test_gpu_lighting_truth.py) takes its path
counts from; the same for the lit and the unlit model on two plan worlds, where no closed form exists
(lighting_truth.RATIO2, seeds 7300 and 7301). Seed 7100, the first and only one tried."""
import math

import numpy as np
import pytest

import env_nee_model as enm
import light_nee_model as lm
import lighting_model as lg
import lighting_truth as ltr
import probe_sets as ps
from oracle import crt_oracle_py as orc

N = 1 << 14
CASES = [(w, s) for w in ltr.WORLDS for s in (True, False)]


@pytest.mark.parametrize("name,sampled", CASES)
def test_the_models_mean_is_the_closed_form_and_its_ratio_is_recorded(crt, name, sampled):
    w, want = ltr.world(crt, name)
    lit = lg.Lighting(w.env, enm.tables(w.env) if sampled else None, lm.tables(w.d))
    bvh = {}
    got, _, tr = lg.ray_color(orc, w.d, w.rays(N), ps.default_states(ltr.SEED, N), 2, ltr.et.BG, ltr.et.T_MIN, lit, crt=crt, bvh=bvh)
    mean, sd = got.mean(0), got.std(0, ddof=1)
    se = sd / math.sqrt(N)
    ratio = float((sd / mean).max())
    log2n, within = ltr.n_for(ratio, 0.01)
    print(f"{name} sampled={sampled}: want {want.tolist()}, mean {mean.tolist()}, z {((mean - want) / se).tolist()}, "
          f"sd / mean {ratio:.3f}, log2 N {log2n}, events {lg.counts(tr)}")
    assert within or (name, sampled) == ("lamp_sun", False)  # the one capped case (lighting_truth.RATIO)
    assert (np.abs(mean - want) <= 5 * se).all()
    assert len(tr.light_kept) > 0 and (not sampled or len(tr.map_kept) > 0)
    rec_ratio, rec_log2n = ltr.RATIO[name, sampled]
    assert abs(ratio - rec_ratio) <= 1e-3 * rec_ratio and log2n == rec_log2n, (ratio, log2n)


@pytest.mark.parametrize("name,sampled", [(w, s) for w in ltr.PLAN_WORLDS for s in (True, False)])
def test_lit_and_unlit_models_agree_on_plan_worlds_and_their_ratio_is_recorded(crt, name, sampled):
    d, _, bvh, rays, menv = ltr.plan_world(crt, name)
    import plan_worlds as pw
    n = ltr.N2
    rays = np.ascontiguousarray(np.resize(rays, (n, 6)))
    unlit = lg.Lighting(menv, None, None)
    lit = lg.Lighting(menv, enm.tables(menv) if sampled else None, lm.tables(d))
    a = lg.ray_color(orc, d, rays, ps.default_states(ltr.SEED0, n), pw.DEPTH, ltr.et.BG, ltr.et.T_MIN, unlit, crt=crt, bvh=bvh)[0]
    b, _, tr = lg.ray_color(orc, d, rays, ps.default_states(ltr.SEED1, n), pw.DEPTH, ltr.et.BG, ltr.et.T_MIN, lit, crt=crt, bvh=bvh)
    m0, m1 = a.mean(0), b.mean(0)
    sd0, sd1 = a.std(0, ddof=1), b.std(0, ddof=1)
    se = np.sqrt(sd0 ** 2 + sd1 ** 2) / math.sqrt(n)
    ratio = float((np.sqrt(sd0 ** 2 + sd1 ** 2) / m0).max())
    log2n, within = ltr.n_for(ratio, 0.02)
    print(f"{name} sampled={sampled}: unlit {m0.tolist()}, lit {m1.tolist()}, z {((m1 - m0) / se).tolist()}, ratio {ratio:.3f}, "
          f"log2 N {log2n}, events {lg.counts(tr)}")
    assert within and (np.abs(m0 - m1) <= 5 * se).all()
    assert len(tr.light_kept) > 0 and (not sampled or len(tr.both) > 0)
    rec_ratio, rec_log2n = ltr.RATIO2[name, sampled]
    assert abs(ratio - rec_ratio) <= 1e-3 * rec_ratio and log2n == rec_log2n, (ratio, log2n)
