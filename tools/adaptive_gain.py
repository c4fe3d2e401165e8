#!/usr/bin/env python3
"""What adaptive sampling saves: BASELINE config 2 (rtow_final 1200 x 800, 500 spp) on one GPU in
10 passes, plain (crt_render_pass_async) and adaptive (one crt_render_pass_masked_async and one
crt_adaptive_update per pass) for a few thresholds, each timed with device events on one stream,
the median of --reps runs after a warm-up. Per threshold: frame ms, samples rendered, mean spp and
ms per rendered Gsample beside the plain render's. Also the mask's overhead (a never-stopping
adaptive render against the plain one), the time of a masked pass with no active block and of one
update, each timed on its own; what is left of the overhead after those two is inferred by
subtraction, not measured.
  python tools/adaptive_gain.py [--reps 3] [--spp 500] [--passes 10] [--thresholds 0.02 0.05 0.1]
Prints one JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.02, 0.05, 0.1])
    a = ap.parse_args()
    import numpy as np
    import torch
    import cpp_raytracer_amd as crt
    from cpp_raytracer_amd import camera_with

    d = crt.SceneData.named("rtow_final", 42)
    d.camera = camera_with(d.camera, image_w=a.width, image_h=a.height, samples_per_pixel=a.spp, max_depth=50)
    s = crt.GpuScene(d)
    s.upload(0)
    cam = crt.resolve_camera(d.camera, 2024)
    L = crt.sample_chunk_len(a.spp)
    chunks = (a.spp + L - 1) // L
    shape = (a.height, a.width)
    ref = torch.empty(shape + (3,), dtype=torch.float64, device="cuda")
    out = torch.empty_like(ref)
    total = torch.empty_like(ref)
    noise = torch.empty(shape + (2,), dtype=torch.float64, device="cuda")
    n_blocks = crt.block_count(a.width, a.height)
    blocks = torch.zeros(n_blocks, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    edges = [min(a.spp, (chunks * i // a.passes) * L) for i in range(a.passes)] + [a.spp]
    bounds = list(zip(edges, edges[1:]))
    min_samples = bounds[1][1] if len(bounds) > 1 else a.spp  # two passes' worth
    bw = np.minimum(16, a.width - 16 * np.arange((a.width + 15) // 16))
    bh = np.minimum(4, a.height - 4 * np.arange((a.height + 3) // 4))
    block_px = np.outer(bh, bw).reshape(-1).astype(np.uint64)
    info = {}

    def plain():
        for lo, hi in bounds:
            s.render_pass(0, cam, lo, hi - lo, total.data_ptr(), noise.data_ptr(), ref.data_ptr() if hi == a.spp else 0, st)

    def adaptive(threshold, floor):
        blocks.zero_()
        active, passes, upd = n_blocks, 0, 0.0
        for lo, hi in bounds:
            s.render_pass_masked(0, cam, lo, hi - lo, total.data_ptr(), noise.data_ptr(), out.data_ptr(),
                                 blocks.data_ptr(), active, st)
            t0 = time.perf_counter()
            active = crt.adaptive_update(0, cam, noise.data_ptr(), blocks.data_ptr(), hi, threshold, floor, st)
            upd += time.perf_counter() - t0  # includes waiting for the pass: host view only
            passes += 1
            if active == 0:
                break
        info["passes"], info["host_ms_in_update_calls"] = passes, upd * 1e3

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    pixels = a.width * a.height
    res = {"width": a.width, "height": a.height, "spp": a.spp, "chunk_len": L, "reps": a.reps, "passes": a.passes,
           "blocks": n_blocks, "min_samples": min_samples}
    base = timed(plain)
    b = statistics.median(base)
    res["plain_ms"] = [round(x, 3) for x in base]
    res["plain_median_ms"] = round(b, 3)
    res["plain_ms_per_gsample"] = round(b / (pixels * a.spp / 1e9), 3)
    # the mask's overhead: no block ever stops (min_samples = spp); the same frame bits
    ms = timed(lambda: adaptive(1e9, a.spp))
    m = statistics.median(ms)
    res["never_stopping"] = {"ms": [round(x, 3) for x in ms], "median_ms": round(m, 3), "over_plain": round(m / b, 4),
                             "bit_identical": bool(torch.equal(out, ref)),
                             # host wall time inside the update calls of the last run: they wait for the
                             # pass before them, so this is an upper bound on the updates, not their cost
                             "host_ms_in_update_calls": round(info["host_ms_in_update_calls"], 3)}
    # where it goes: the list build + masked accumulate against the plain accumulate (one pass's
    # kernels without the draw: a pass with no active block), and the update
    words = blocks.clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    zero = []
    for hint in (0, 1):
        for _ in range(a.reps + 1):
            e0.record()
            s.render_pass_masked(0, cam, L, L, total.data_ptr(), noise.data_ptr(), out.data_ptr(), blocks.data_ptr(), hint, st)
            e1.record()
            e1.synchronize()
            zero.append(e0.elapsed_time(e1))
        res[f"zero_active_pass_ms_hint_{hint}"] = round(statistics.median(zero[-a.reps:]), 4)
    assert torch.equal(blocks, words)  # every word is spp: no block matched first_sample = L
    upd = []
    for _ in range(a.reps + 1):
        e0.record()
        crt.adaptive_update(0, cam, noise.data_ptr(), blocks.data_ptr(), a.spp, 1e9, a.spp, st)
        e1.record()
        e1.synchronize()
        upd.append(e0.elapsed_time(e1))
    res["update_ms"] = round(statistics.median(upd[-a.reps:]), 4)
    rows = []
    for thr in a.thresholds:
        ms = timed(lambda: adaptive(thr, min_samples))
        m = statistics.median(ms)
        counts = (blocks.cpu().numpy().view(np.uint32) & np.uint32(0x7fffffff)).astype(np.uint64)
        rendered = int((counts * block_px).sum())
        rows.append({"threshold": thr, "ms": [round(x, 3) for x in ms], "median_ms": round(m, 3),
                     "speedup_over_plain": round(b / m, 3), "samples_rendered": rendered,
                     "mean_spp": round(rendered / pixels, 2), "ms_per_gsample": round(m / (rendered / 1e9), 3),
                     "passes": info["passes"], "blocks_at_full_spp": int((counts == a.spp).sum()),
                     "finite": bool(torch.isfinite(out).all())})
    res["adaptive"] = rows
    print(json.dumps(res))
    return 0 if res["never_stopping"]["bit_identical"] and all(r["finite"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
