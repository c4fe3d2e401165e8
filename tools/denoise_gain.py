#!/usr/bin/env python3
"""What the denoiser costs and what it buys: BASELINE config 2 (rtow_final 1200 x 800) on one GPU.
Three steps, each a child process under its own time limit (a step that fails or runs out of time
ends the tool; nothing is started on the GPU after it):
  reference  the 500-spp frame (base seed 2024), kept for the quality step
  timing     a 50-spp job: ms of one 50-sample pass (the yardstick: a preview should cost less than
             the pass it follows), of the feature pass, the variance map and the filter, each timed
             with device events on one stream, the median of --reps runs after a warm-up; the filter
             also per iteration count and with every step forced to the gather route
  quality_plain, quality_adaptive
             RMSE against the 500-spp frame, raw and denoised, of a plain 50-spp render and of an
             adaptive render at threshold 0.05 (500-spp job, 10 passes), base seed 2025; one
             process and one scene each
  python tools/denoise_gain.py [--reps 5] [--out profiles/denoise/denoise_gain.json]
Writes the JSON file and prints it as one line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
LIMITS = {"reference": 240, "timing": 300, "quality_plain": 240, "quality_adaptive": 240}  # seconds per step


def setup(a, spp, seed):
    # torch first, as in the other tools and the test suite: the library then runs on the HIP
    # runtime PyTorch brings along. On the system's ROCm 7.0 runtime alone, renders in passes at
    # this frame size lost passes ("Pass scratch", and 6c)
    import torch  # noqa: F401
    import cpp_raytracer_amd as crt
    from cpp_raytracer_amd import camera_with
    d = crt.SceneData.named("rtow_final", 42)
    d.camera = camera_with(d.camera, image_w=a.width, image_h=a.height, samples_per_pixel=spp, max_depth=50)
    s = crt.GpuScene(d)
    s.upload(0)
    return crt, s, crt.resolve_camera(d.camera, seed)


def params(crt, a, iterations=None):
    return crt.denoise_params(iterations or a.iterations, a.squarings, a.sigma_l, a.sigma_p)


def step_reference(a, work):
    import numpy as np
    crt, s, cam = setup(a, a.ref_spp, 2024)
    frame, _ = s.render(cam, 1)
    np.save(work / "reference.npy", frame)
    return {"ref_spp": a.ref_spp}


def step_timing(a, work):
    import torch
    crt, s, cam = setup(a, a.spp, 2025)
    shape = (a.height, a.width)
    dev = "cuda"
    total, out, den = (torch.empty(shape + (3,), dtype=torch.float64, device=dev) for _ in range(3))
    noise = torch.empty(shape + (2,), dtype=torch.float64, device=dev)
    var = torch.empty(shape, dtype=torch.float64, device=dev)
    feat = torch.empty(a.height * a.width, 88, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

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
        return {"ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4)}

    def filt(iterations=None):
        crt.denoise(0, a.width, a.height, out.data_ptr(), var.data_ptr(), feat.data_ptr(), params(crt, a, iterations),
                    den.data_ptr(), 0, st)

    res = {"spp": a.spp, "reps": a.reps}
    res["pass"] = timed(lambda: s.render_pass(0, cam, 0, a.spp, total.data_ptr(), noise.data_ptr(), out.data_ptr(), st))
    res["features"] = timed(lambda: s.render_features(0, cam, feat.data_ptr(), st))
    res["variance"] = timed(lambda: crt.pixel_variance(0, cam, noise.data_ptr(), var.data_ptr(), a.spp, 0, st))
    res["filter"] = timed(filt)
    auto = den.clone()
    res["filter_by_iterations"] = {str(i): timed(lambda: filt(i))["median_ms"] for i in range(1, a.iterations + 1)}
    os.environ["CRT_DENOISE_ROUTE"] = "gather"
    res["filter_all_gather"] = timed(filt)
    res["filter_all_gather_bit_identical"] = bool(torch.equal(den, auto))
    res["filter_all_gather_by_iterations"] = {str(i): timed(lambda: filt(i))["median_ms"]
                                              for i in range(1, a.iterations + 1)}
    del os.environ["CRT_DENOISE_ROUTE"]
    preview = res["variance"]["median_ms"] + res["filter"]["median_ms"]
    res["preview_ms"] = round(preview, 4)  # features are computed once per render, not per preview
    res["preview_over_pass"] = round(preview / res["pass"]["median_ms"], 4)
    return res


def quality(a, work, raw, den):
    import numpy as np
    ref = np.load(work / "reference.npy")

    def rmse(x):
        return float(np.sqrt(np.mean((x - ref) ** 2)))

    return {"rmse_raw": round(rmse(raw), 6), "rmse_denoised": round(rmse(den), 6),
            "denoised_over_raw": round(rmse(den) / rmse(raw), 4), "finite": bool(np.isfinite(den).all())}


def step_quality_plain(a, work):
    crt, s, cam = setup(a, a.spp, 2025)
    den, raw, _ = s.render_denoised(cam, params(crt, a), noisy=True)
    return {"spp": a.spp, **quality(a, work, raw, den)}


def step_quality_adaptive(a, work):
    import numpy as np
    crt, s, cam = setup(a, a.ref_spp, 2025)
    per_pass = a.ref_spp // 10
    # the job's one-shot frame: a block that ran to the end must hold exactly its pixels (the
    # validity check of the adaptive frames below; see DESIGN 6c, "a pass-render fault met here")
    full, _ = s.render(cam, 1)
    den, raw, rendered = s.render_denoised(cam, params(crt, a), threshold=a.threshold, min_samples=2 * per_pass,
                                           samples_per_pass=per_pass, noisy=True)
    frame, counts, total = s.render_adaptive(cam, a.threshold, 2 * per_pass, per_pass)
    at_end = np.repeat(np.repeat(counts, 4, axis=0), 16, axis=1)[:a.height, :a.width] == a.ref_spp
    return {"threshold": a.threshold, "job_spp": a.ref_spp, "mean_spp": round(rendered / (a.width * a.height), 2),
            "noisy_is_render_adaptives_frame": bool(np.array_equal(raw, frame) and rendered == total),
            "pixels_at_full_count": int(at_end.sum()),
            "full_count_pixels_equal_one_shot": bool(np.array_equal(raw[at_end], full[at_end])),
            **quality(a, work, raw, den)}


STEPS = {"reference": step_reference, "timing": step_timing, "quality_plain": step_quality_plain,
         "quality_adaptive": step_quality_adaptive}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--spp", type=int, default=50)
    ap.add_argument("--ref-spp", type=int, default=500)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--squarings", type=int, default=7)
    ap.add_argument("--sigma-l", type=float, default=1.0)
    ap.add_argument("--sigma-p", type=float, default=0.05)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise" / "denoise_gain.json"))
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--work")
    a = ap.parse_args()
    if a.step:  # a child: one step, its result as JSON in the work folder
        work = Path(a.work)
        (work / f"{a.step}.json").write_text(json.dumps(STEPS[a.step](a, work)))
        return 0
    res = {"width": a.width, "height": a.height,
           "params": {"iterations": a.iterations, "normal_squarings": a.squarings, "sigma_l": a.sigma_l, "sigma_p": a.sigma_p}}
    with tempfile.TemporaryDirectory() as work:
        for name in ("reference", "timing", "quality_plain", "quality_adaptive"):
            cmd = [sys.executable, __file__, "--step", name, "--work", work] + [x for x in sys.argv[1:]]
            try:
                r = subprocess.run(cmd, timeout=LIMITS[name])
            except subprocess.TimeoutExpired:
                print(f"denoise_gain: step {name} ran past its {LIMITS[name]} s limit; stopping", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"denoise_gain: step {name} failed ({r.returncode}); stopping", file=sys.stderr)
                return 1
            res[name] = json.loads((Path(work) / f"{name}.json").read_text())
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    ok = (res["quality_plain"]["finite"] and res["quality_adaptive"]["finite"] and
          res["quality_adaptive"]["noisy_is_render_adaptives_frame"] and
          res["quality_adaptive"]["full_count_pixels_equal_one_shot"] and res["timing"]["filter_all_gather_bit_identical"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
