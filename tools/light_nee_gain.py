"""What sampling the scene's own lights buys and costs: crt_radiance_lights_async against
crt_radiance_async on the same camera rays and states. DESIGN section 6m.

  python tools/light_nee_gain.py [--reps 5] [--spp 16] [--width 640] [--scenes cornell,rtow_final_lights,christmas_tree]

cornell (BASELINE config 3: one parallelogram light), rtow_final_lights and christmas_tree (emissive
spheres) with their own cameras at --width pixels across. For each scene:
  - milliseconds a call of both entries on the camera's --spp samples a pixel, alternating within one
    run, timed with device events after a warm-up: medians of --reps with min-max, and the ratio;
  - per-pixel RMSE of the frame (the mean over a pixel's samples) against a reference: a sampled run 16
    times as long with other seeds; for the unsampled entry at --spp samples (equal sample count) and at
    the number of samples it traces in the sampled call's time (equal time), for the sampled entry at
    --spp.
Nothing here is a pass/fail bar."""
import argparse
import json
import sys
from pathlib import Path

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import cpp_raytracer_amd as crt  # noqa: E402
from radiance_rate import timed  # noqa: E402

SCENES = {"cornell": ("cornell", None), "rtow_final_lights": ("rtow_final_lights", 42),
          "christmas_tree": ("christmas_tree", None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--scenes", default="cornell,rtow_final_lights,christmas_tree")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    for key in a.scenes.split(","):
        name, seed = SCENES[key]
        d = crt.SceneData.named(name, seed)
        w = a.width
        h = max(1, round(w * d.camera.image_h / d.camera.image_w))
        scene = crt.GpuScene(d)
        scene.upload(0)
        lights = scene.light_sampler(0)
        L = len(lights.tables.prim)

        def job(spp, cam_seed):
            cam = crt.resolve_camera(crt.camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp), cam_seed)
            rays, states = scene.camera_rays(cam)
            return cam, rays, states

        def frame(cam, rays, states, sampled, out=None):
            n = len(rays)
            out = torch.empty((n, 3), dtype=torch.float64, device="cuda") if out is None else out
            scene.radiance_async(0, rays.data_ptr(), n, out.data_ptr(), states.data_ptr(), max_depth=cam.max_depth,
                                 background=tuple(cam.background), t_min=cam.t_min, stream=stream,
                                 lights=lights.handle if sampled else 0)
            return out

        def image(out, spp):
            return out.view(h * w, spp, 3).mean(1)

        cam, rays, states = job(a.spp, 1)
        out = frame(cam, rays, states, False)
        frame(cam, rays, states, True, out)  # warm-up of both
        torch.cuda.synchronize()
        ms = {"unsampled": [], "sampled": []}
        for _ in range(a.reps):  # alternating: one of each per round
            ms["unsampled"].append(timed(lambda: frame(cam, rays, states, False, out)))
            ms["sampled"].append(timed(lambda: frame(cam, rays, states, True, out)))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        ratio = med["sampled"] / med["unsampled"]
        # the reference: 16 sampled jobs of --spp with other seeds
        ref = torch.zeros((h * w, 3), dtype=torch.float64, device="cuda")
        for k in range(16):
            c2, r2, s2 = job(a.spp, 1000 + k)
            ref += image(frame(c2, r2, s2, True), a.spp)
        ref /= 16

        def rmse(img):
            return float(torch.sqrt(((img - ref) ** 2).mean()))

        equal_spp = max(1, round(a.spp * ratio))
        c3, r3, s3 = job(equal_spp, 1)
        err = {"unsampled": rmse(image(frame(cam, rays, states, False), a.spp)),
               "sampled": rmse(image(frame(cam, rays, states, True), a.spp)),
               "unsampled_equal_time": rmse(image(frame(c3, r3, s3, False), equal_spp))}
        torch.cuda.synchronize()
        rows.append({"scene": key, "lights": L, "w": w, "h": h, "spp": a.spp, "ms": med,
                     "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
                     "ratio": ratio, "equal_time_spp": equal_spp, "rmse": err, "ref_mean": float(ref.mean())})
        for k in ("unsampled", "sampled"):
            print(f"{key:17s} {L:5d} lights {w}x{h}x{a.spp:<3d} {k:9s} {med[k]:9.2f} ms ({min(ms[k]):.2f}-{max(ms[k]):.2f})", flush=True)
        print(f"{key:17s} sampled / unsampled time = {ratio:.3f}; RMSE against the reference (mean {rows[-1]['ref_mean']:.4g}): "
              f"unsampled {err['unsampled']:.4g}, sampled {err['sampled']:.4g} ({err['unsampled'] / err['sampled']:.2f} x lower) "
              f"at {a.spp} spp; unsampled at {equal_spp} spp (equal time) {err['unsampled_equal_time']:.4g} "
              f"({err['unsampled_equal_time'] / err['sampled']:.2f} x)", flush=True)
        del lights
        scene.close()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
