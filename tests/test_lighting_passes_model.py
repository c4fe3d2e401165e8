"""The adaptive scenario that tests/test_gpu_lighting_passes.py runs under a lighting, checked without a GPU
on tests/lighting_model.py's radiance of the lens model's rays: with lighting_cases.SCEN_THRESHOLD it is a
real mix of blocks that stop at the first eligible pass, blocks that stop later at different counts and
blocks that never stop, and a stopped block holds what plain passes hold after its own count."""
import numpy as np
import pytest

import lens_model as lm
import lens_pass_model as lpm
import lighting_cases as cs
import lighting_model as lg
import pass_model as pm
import test_lens_pass_model as tl
from oracle import crt_oracle_py as orc


@pytest.mark.parametrize("kind", ["equirect", "cube"])
def test_the_lit_adaptive_scenario_is_a_mix(crt, kind):
    w, h = lpm.SCEN_FRAMES[kind]
    d, cam, lens = tl.setup(crt, "cornell", kind, w, h, lpm.SCEN_SPP, lpm.SCEN_INSIDE[kind])
    rays, states = lm.lens_rays(crt, cam, lens)
    rad, _, tr = lg.ray_color(orc, d, rays, states, 50, tl.BG, cam.t_min, cs.lighting(d, cs.SCEN_LIGHTING), crt=crt)
    assert len(tr.both) and len(tr.map_kept) and len(tr.light_kept)  # the frame's paths take both samples
    rad = rad.reshape(h, w, lpm.SCEN_SPP, 3)
    st = lpm.fresh_state(w, h)
    for first, count in lpm.pass_plan(lpm.SCEN_SPP, 4, lpm.SCEN_PASS):  # the ratios the thresholds were chosen from
        lpm.lens_pass(st, rad[:, :, first:first + count], first, 4)
        sse, sm = pm.block_sums(st["noise"], w, h, (first + count) // 4, 4)
        with np.errstate(all="ignore"):
            print(kind, first + count, np.array2string(sse / sm, precision=4, max_line_width=200))
    steps = lpm.run_adaptive(rad, lpm.SCEN_PASS, cs.SCEN_THRESHOLD[kind])
    counts, stopped = lpm.check_mix(steps)  # early, never, and two different later counts
    print(kind, "counts", counts.tolist(), "stopped", stopped.tolist())
    assert len(steps) == lpm.SCEN_SPP // lpm.SCEN_PASS  # a block is active to the end
    late = counts[stopped & (counts > lpm.SCEN_PASS)]
    assert len(late) >= 2 and (~stopped).sum() >= 2, (counts, stopped)
    final = steps[-1][2]
    for b, (ys, xs) in enumerate(pm.block_slices(w, h)):
        n = int(counts[b])
        assert tl.same(final["rgb"][ys, xs], lm.frame(rad[:, :, :n], 4)[ys, xs]), b
