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
Writes the JSON file and prints it as one line.
  python tools/denoise_gain.py --devices 2 4 8 [--out profiles/denoise/denoise_devices.json]
runs one other step instead: the cost of a denoised preview and of a whole denoised render over N
devices (crt_render_denoised_devices) against one device (step_devices)."""
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
DEFAULT_OUT = str(ROOT / "profiles" / "denoise" / "denoise_gain.json")
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


class Stderr:
    """File descriptor 2 into a temporary file for the block: the library's CRT_DENOISE_TIMING lines."""

    def __enter__(self):
        sys.stderr.flush()
        self.saved, self.tmp = os.dup(2), tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def step_devices(a, work):
    """--devices N...: what a denoised preview and a whole denoised render cost over N devices
    (crt_render_denoised_devices) against one device, all in this one process. Medians of --reps
    after a warm-up; host clock around calls that end in a synchronise, and the library's own split
    of a preview (CRT_DENOISE_TIMING: events on device 0's stream). With fewer than N devices
    visible the N are emulated on device 0 (CRT_EMULATE_DEVICES) and labelled so: such figures say
    what the extra copies and launches cost, not what several GPUs gain."""
    import time
    import torch
    crt, s, cam = setup(a, a.spp, 2025)
    prm = params(crt, a)
    visible = crt.device_count()
    chunk = crt.sample_chunk_len(a.spp)
    per_pass = (max(1, a.spp // 10) + chunk - 1) // chunk * chunk
    job = dict(threshold=a.threshold, min_samples=2 * per_pass, samples_per_pass=per_pass)

    def med(xs):
        return round(statistics.median(xs), 4)

    def host_ms(fn):
        fn()  # warm-up
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return med(ms)

    # one device, low-level calls on one stream: a preview is variance + filter (+ the frame's way home)
    shape = (a.height, a.width)
    total, out, den = (torch.empty(shape + (3,), dtype=torch.float64, device="cuda") for _ in range(3))
    noise = torch.empty(shape + (2,), dtype=torch.float64, device="cuda")
    var = torch.empty(shape, dtype=torch.float64, device="cuda")
    feat = torch.empty(a.height * a.width, 88, dtype=torch.uint8, device="cuda")
    host_den, host_raw = (torch.empty(shape + (3,), dtype=torch.float64) for _ in range(2))
    st = torch.cuda.current_stream().cuda_stream
    s.render_pass(0, cam, 0, a.spp, total.data_ptr(), noise.data_ptr(), out.data_ptr(), st)
    s.render_features(0, cam, feat.data_ptr(), st)
    torch.cuda.synchronize()

    def preview_on_device():
        crt.pixel_variance(0, cam, noise.data_ptr(), var.data_ptr(), a.spp, 0, st)
        crt.denoise(0, a.width, a.height, out.data_ptr(), var.data_ptr(), feat.data_ptr(), prm, den.data_ptr(), 0, st)
        torch.cuda.synchronize()

    def preview_to_host():
        crt.pixel_variance(0, cam, noise.data_ptr(), var.data_ptr(), a.spp, 0, st)
        crt.denoise(0, a.width, a.height, out.data_ptr(), var.data_ptr(), feat.data_ptr(), prm, den.data_ptr(), 0, st)
        host_den.copy_(den)
        host_raw.copy_(out)
        torch.cuda.synchronize()

    res = {"spp": a.spp, "reps": a.reps, "visible_devices": visible, "job": job,
           "one_device": {"preview_ms": host_ms(preview_on_device), "preview_to_host_ms": host_ms(preview_to_host),
                          "render_denoised_ms": host_ms(lambda: s.render_denoised(cam, prm, noisy=True, **job)),
                          "render_adaptive_ms": host_ms(lambda: s.render_adaptive(cam, job["threshold"], job["min_samples"],
                                                                                  job["samples_per_pass"]))},
           "devices": {}}
    one_den, one_raw, one_n = s.render_denoised(cam, prm, noisy=True, **job)
    fields = ("host_ms", "lanes_ms", "gather_ms", "filter_ms", "d2h_ms")
    for n in a.devices:
        emulated = n > visible
        if emulated:
            os.environ["CRT_EMULATE_DEVICES"] = str(n)
        r = {"emulated": emulated}
        r["render_denoised_ms"] = host_ms(lambda: s.render_denoised(cam, prm, noisy=True, num_devices=n, **job))
        r["render_adaptive_ms"] = host_ms(lambda: s.render_adaptive(cam, job["threshold"], job["min_samples"],
                                                                    job["samples_per_pass"], num_devices=n))
        den_n, raw_n, n_n = s.render_denoised(cam, prm, noisy=True, num_devices=n, **job)
        r["bit_identical_to_one_device"] = bool((den_n.view("u8") == one_den.view("u8")).all() and
                                                (raw_n.view("u8") == one_raw.view("u8")).all() and n_n == one_n)
        # previews after every pass of a job that never stops a block: the library reports each one
        never = dict(threshold=a.threshold, min_samples=a.spp, samples_per_pass=per_pass)
        os.environ["CRT_DENOISE_TIMING"] = "1"
        lines = []
        for rep in range(a.reps + 1):
            with Stderr() as err:
                s.render_denoised(cam, prm, noisy=True, num_devices=n, preview=True, callback=lambda *x: 0, **never)
            if rep:  # the first call is the warm-up
                lines += [ln for ln in err.text.splitlines() if ln.startswith("crt_denoise_timing")]
        del os.environ["CRT_DENOISE_TIMING"]
        rows = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in lines]
        r["previews_timed"] = len(rows)
        r["preview"] = {f: med([float(x[f]) for x in rows]) for f in fields}
        if emulated:
            del os.environ["CRT_EMULATE_DEVICES"]
        res["devices"][str(n)] = r
    return res


STEPS = {"reference": step_reference, "timing": step_timing, "quality_plain": step_quality_plain,
         "quality_adaptive": step_quality_adaptive, "devices": step_devices}
LIMITS["devices"] = 420


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
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--devices", type=int, nargs="+", metavar="N",
                    help="only the several-devices step, for each N (emulated where fewer are visible)")
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--work")
    a = ap.parse_args()
    if a.step:  # a child: one step, its result as JSON in the work folder
        work = Path(a.work)
        (work / f"{a.step}.json").write_text(json.dumps(STEPS[a.step](a, work)))
        return 0
    res = {"width": a.width, "height": a.height,
           "params": {"iterations": a.iterations, "normal_squarings": a.squarings, "sigma_l": a.sigma_l, "sigma_p": a.sigma_p}}
    names = ("devices",) if a.devices else ("reference", "timing", "quality_plain", "quality_adaptive")
    if a.devices and a.out == DEFAULT_OUT:
        a.out = str(ROOT / "profiles" / "denoise" / "denoise_devices.json")
    with tempfile.TemporaryDirectory() as work:
        for name in names:
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
    if a.devices:
        return 0 if all(r["bit_identical_to_one_device"] for r in res["devices"]["devices"].values()) else 1
    ok = (res["quality_plain"]["finite"] and res["quality_adaptive"]["finite"] and
          res["quality_adaptive"]["noisy_is_render_adaptives_frame"] and
          res["quality_adaptive"]["full_count_pixels_equal_one_shot"] and res["timing"]["filter_all_gather_bit_identical"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
