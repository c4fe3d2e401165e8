#!/usr/bin/env python3
"""What lens renders in passes cost and save: a 2048 x 1024 EQUIRECT panorama and 640 x 360 PINHOLE and
FISHEYE frames at 64 spp on rtow_final and cornell (the lens at the scene camera's position; inside the
box for cornell's panorama and fisheye), on one GPU. Per job, each timed with device events on one stream,
the median of --reps runs after a warm-up:
  - crt_render_lens_async one-shot, and the job through crt_render_lens_pass_async in 1, 4 and 16 equal
    passes (the frame written by the last pass only), the final frame compared with the one-shot frame;
  - the job in 8 plain passes against an adaptive run of 8 masked passes with crt_adaptive_update at
    --threshold (a floor of two passes), with the mean samples per pixel it rendered; a never-stopping
    adaptive run is compared with the one-shot frame first; a masked pass with no active block and one
    update are timed on their own;
  - crt_lens_features_async once, and one preview's crt_pixel_variance_async + crt_denoise_async (a
    cube map would take six filter calls; none is measured here).
--one-shot-only times the one-shot renders alone (CRT_LIB=<another build> gives that build's figures, for
the ratio against a parent commit's library).
  python tools/lens_pass_overhead.py [--reps 5] [--spp 64] [--threshold 0.05] [--one-shot-only]
Prints one JSON line; exits non-zero if a frame differs from the one-shot frame."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

JOBS = [("equirect", 2048, 1024), ("pinhole", 640, 360), ("fisheye", 640, 360)]
INSIDE_CORNELL = (278.0, 400.0, 120.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--scenes", nargs="+", default=["rtow_final", "cornell"])
    ap.add_argument("--one-shot-only", action="store_true")
    a = ap.parse_args()
    import torch  # before the library: the process runs on torch's runtime
    import numpy as np
    import cpp_raytracer_amd as crt
    from cpp_raytracer_amd import camera_with

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
        return round(statistics.median(ms), 3), [round(x, 3) for x in ms]

    st = torch.cuda.current_stream().cuda_stream
    L = crt.sample_chunk_len(a.spp)
    chunks = (a.spp + L - 1) // L
    rows, ok = [], True
    for name in a.scenes:
        d = crt.SceneData.named(name, 42) if name == "rtow_final" else crt.SceneData.named(name)
        s = crt.GpuScene(d)
        s.upload(0)
        c = d.camera
        o = np.array(list(c.center))
        f = np.array(list(c.lookat)) - o if c.has_lookat else np.array(list(c.direction))
        for kind, w, h in JOBS:
            cam = crt.resolve_camera(camera_with(c, image_w=w, image_h=h, samples_per_pixel=a.spp, max_depth=50), 2024)
            origin = INSIDE_CORNELL if name == "cornell" and kind != "pinhole" else tuple(o)
            lens = crt.make_lens(kind, origin=origin, forward=tuple(f), up=tuple(c.up))
            ref, out, total = [torch.empty((h, w, 3), dtype=torch.float64, device="cuda") for _ in range(3)]
            row = {"scene": name, "kind": kind, "width": w, "height": h, "spp": a.spp, "chunk_len": L}
            row["one_shot_ms"], row["one_shot_all_ms"] = timed(lambda: s.render_lens_async(0, cam, lens, ref.data_ptr(), st))
            rows.append(row)
            if a.one_shot_only:
                continue
            noise = torch.empty((h, w, 2), dtype=torch.float64, device="cuda")
            nb = crt.block_count(w, h)
            blocks = torch.zeros(nb, dtype=torch.int32, device="cuda")

            def bounds(n):
                edges = [min(a.spp, (chunks * i // n) * L) for i in range(n)] + [a.spp]
                return [(lo, hi) for lo, hi in zip(edges, edges[1:]) if hi > lo]

            def plain(n):
                for lo, hi in bounds(n):
                    s.render_lens_pass(0, cam, lens, lo, hi - lo, total.data_ptr(), noise.data_ptr(),
                                       out.data_ptr() if hi == a.spp else 0, 0, 0, st)

            info = {}

            def adaptive(threshold, min_samples):
                blocks.zero_()
                active = nb
                for lo, hi in bounds(8):
                    if not active:
                        break
                    s.render_lens_pass(0, cam, lens, lo, hi - lo, total.data_ptr(), noise.data_ptr(), out.data_ptr(),
                                       blocks.data_ptr(), active, st)
                    active = crt.adaptive_update(0, cam, noise.data_ptr(), blocks.data_ptr(), hi, threshold, min_samples, st)
                info["words"] = blocks.cpu().numpy().view(np.uint32)

            row["passes"] = []
            for n in (1, 4, 16):
                m, ms = timed(lambda: plain(n))
                same = bool(torch.equal(out, ref))
                ok = ok and same
                row["passes"].append({"passes": len(bounds(n)), "ms": m, "all_ms": ms, "over_one_shot": round(m / row["one_shot_ms"], 4),
                                      "bit_identical": same})
            plain8, _ = timed(lambda: plain(8))
            never, _ = timed(lambda: adaptive(0.0, a.spp))  # min_samples >= spp: no block ever stops
            same = bool(torch.equal(out, ref))
            ok = ok and same
            ad, ad_all = timed(lambda: adaptive(a.threshold, bounds(8)[1][1]))
            bw = np.minimum(16, w - 16 * np.arange((w + 15) // 16))
            bh = np.minimum(4, h - 4 * np.arange((h + 3) // 4))
            counts = (info["words"] & np.uint32(0x7FFFFFFF)).astype(np.uint64)
            rendered = int((counts * np.outer(bh, bw).reshape(-1).astype(np.uint64)).sum())
            # the mask's fixed costs, each on its own: a masked pass that finds every block stopped (the
            # list, the skip kernel and the wait for the 4-byte count) and one update
            def empty_pass():
                s.render_lens_pass(0, cam, lens, 8, 8, total.data_ptr(), noise.data_ptr(), out.data_ptr(), blocks.data_ptr(), 0, st)

            blocks.fill_(-(1 << 31) + 16)  # every block stopped at 16 samples: none is at 8
            empty_ms, _ = timed(empty_pass)
            plain(1)  # a full noise state for the update to read
            blocks.fill_(a.spp)
            update_ms, _ = timed(lambda: crt.adaptive_update(0, cam, noise.data_ptr(), blocks.data_ptr(), a.spp, 0.0, a.spp, st))
            row["adaptive"] = {"empty_masked_pass_ms": empty_ms, "update_ms": update_ms, "threshold": a.threshold, "plain_8_passes_ms": plain8, "never_stopping_ms": never,
                               "never_stopping_bit_identical": same, "ms": ad, "all_ms": ad_all,
                               "over_plain_8_passes": round(ad / plain8, 4), "mean_spp": round(rendered / (w * h), 3)}
            feat = torch.empty((w * h, 88), dtype=torch.uint8, device="cuda")
            var = torch.empty((h, w), dtype=torch.float64, device="cuda")
            den = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
            prm = crt.denoise_params()
            row["features_ms"], _ = timed(lambda: s.lens_features(0, cam, lens, feat.data_ptr(), st))

            def preview():
                crt.pixel_variance(0, cam, noise.data_ptr(), var.data_ptr(), a.spp, blocks.data_ptr(), st)
                crt.denoise(0, w, h, out.data_ptr(), var.data_ptr(), feat.data_ptr(), prm, den.data_ptr(), 0, st)

            row["denoise_per_preview_ms"], _ = timed(preview)
        s.close()
    print(json.dumps({"reps": a.reps, "build": crt.lib().crt_build_info().decode(), "jobs": rows}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
