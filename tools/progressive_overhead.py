#!/usr/bin/env python3
"""Per-pass overhead of progressive rendering: BASELINE config 2 (rtow_final 1200 x 800, 500 spp)
rendered one-shot (crt_render_async) and through crt_render_pass_async in 1, 5, 10 and 25 equal
passes, each timed with device events on one stream after a warm-up render, with the final frame
compared with the one-shot frame. Every pass drains the persistent grid; the table shows what
that costs ("Progressive rendering").
  python tools/progressive_overhead.py [--reps 3] [--spp 500] [--passes 1 5 10 25]
Prints one JSON line."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--passes", type=int, nargs="+", default=[1, 5, 10, 25])
    a = ap.parse_args()
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
    st = torch.cuda.current_stream().cuda_stream

    def one_shot():
        s.render_async(0, cam, ref.data_ptr(), st)

    def in_passes(n):
        # n passes of whole chunks, as equal as the chunk count allows; the frame only at the end
        edges = [min(a.spp, (chunks * i // n) * L) for i in range(n)] + [a.spp]
        for lo, hi in zip(edges, edges[1:]):
            s.render_pass(0, cam, lo, hi - lo, total.data_ptr(), noise.data_ptr(),
                          out.data_ptr() if hi == a.spp else 0, st)

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

    res = {"width": a.width, "height": a.height, "spp": a.spp, "chunk_len": L, "reps": a.reps}
    base = timed(one_shot)
    res["one_shot_ms"] = [round(x, 3) for x in base]
    b = statistics.median(base)
    rows = []
    for n in a.passes:
        ms = timed(lambda: in_passes(n))
        m = statistics.median(ms)
        rows.append({"passes": n, "ms": [round(x, 3) for x in ms], "median_ms": round(m, 3),
                     "over_one_shot": round(m / b, 4), "ms_per_pass_over": round((m - b) / n, 3),
                     "bit_identical": bool(torch.equal(out, ref))})
    res["one_shot_median_ms"] = round(b, 3)
    res["progressive"] = rows
    print(json.dumps(res))
    return 0 if all(r["bit_identical"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
