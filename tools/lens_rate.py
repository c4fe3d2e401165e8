"""Lens-render throughput: crt_render_lens_async against the render it equals and against its own
middle stage, alternating within one run. DESIGN section 6g.

  python tools/lens_rate.py [--reps 7] [--width 640] [--height 360] [--spp 64]
                            [--scenes rtow_final,cornell] [--pano 2048x1024] [--out FILE]

Per scene, with the scene's own camera at --width x --height and --spp samples and kind PINHOLE:
  (a) lens      GpuScene.render_lens_async: generate, trace and reduce on the device, in the batches
                the library picks (256 MiB of scratch); `lens_1` is the same call with batch_pixels =
                width * height, one batch;
  (b) render    crt_render_async on the same camera: the same frame, bit for bit;
  (c) radiance  crt_radiance_async alone, on the very rays and states (a) generates
                (crt_lens_rays_async, called once outside the timing).
(a)/(c) is what generating and reducing cost; (a)/(b) what the general route costs over the render
kernel. Then an equirectangular --pano frame at --spp samples from the camera's position, default
batches, on its own. The calls are timed with device events after a warm-up, medians of --reps with
min-max. Before any rate is printed (a)'s frames are compared, byte for byte, with (b)'s."""
import argparse
import json
import sys
from pathlib import Path

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import cpp_raytracer_amd as crt  # noqa: E402

SCENES = {"rtow_final": ("rtow_final", 42), "cornell": ("cornell", None), "christmas_tree": ("christmas_tree", None)}


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--scenes", default="rtow_final,cornell")
    ap.add_argument("--pano", default="2048x1024")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    w, h, spp = a.width, a.height, a.spp
    pw, ph = (int(v) for v in a.pano.split("x"))
    for key in a.scenes.split(","):
        name, seed = SCENES[key]
        d = crt.SceneData.named(name, seed)
        scene = crt.GpuScene(d)
        scene.upload(0)
        cam = crt.resolve_camera(crt.camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp), 1)
        bg = tuple(cam.background)
        lens, lens_1 = crt.make_lens("pinhole"), crt.make_lens("pinhole", batch_pixels=w * h)
        rays, states = scene.lens_rays(cam, lens)
        n = w * h * spp
        frames = {k: torch.empty((h, w, 3), dtype=torch.float64, device="cuda") for k in ("lens", "lens_1", "render")}
        L = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        calls = {
            "lens": lambda: scene.render_lens_async(0, cam, lens, frames["lens"].data_ptr(), stream),
            "lens_1": lambda: scene.render_lens_async(0, cam, lens_1, frames["lens_1"].data_ptr(), stream),
            "render": lambda: scene.render_async(0, cam, frames["render"].data_ptr(), stream),
            "radiance": lambda: scene.radiance_async(0, rays.data_ptr(), n, L.data_ptr(), states.data_ptr(),
                                                     max_depth=cam.max_depth, background=bg, t_min=cam.t_min, stream=stream),
        }
        for c in calls.values():  # warm-up, then the checks
            c()
        torch.cuda.synchronize()
        for k in ("lens", "lens_1"):
            assert torch.equal(frames[k].view(torch.int64), frames["render"].view(torch.int64)), (key, k, "!= the render")
        ms = {k: [] for k in calls}
        for _ in range(a.reps):  # alternating: one of each per round
            for k, c in calls.items():
                ms[k].append(timed(c))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, v in ms.items():
            rate = [n / (x * 1e3) for x in v]
            rows.append({"scene": key, "kind": "pinhole", "w": w, "h": h, "spp": spp, "call": k, "ms": med[k], "ms_min": min(v),
                         "ms_max": max(v), "mpaths_s": float(np.median(rate))})
            print(f"{key:14s} pinhole {w} x {h} x {spp}  {k:8s} {med[k]:9.2f} ms ({min(v):.2f}-{max(v):.2f})  "
                  f"{np.median(rate):8.1f} M paths/s", flush=True)
        for k in ("lens", "lens_1"):
            r_b = [x / y for x, y in zip(ms[k], ms["render"])]
            r_c = [x / y for x, y in zip(ms[k], ms["radiance"])]
            rows.append({"scene": key, "call": "ratios", "of": k, "over_render": med[k] / med["render"],
                         "over_render_min": min(r_b), "over_render_max": max(r_b), "over_radiance": med[k] / med["radiance"],
                         "over_radiance_min": min(r_c), "over_radiance_max": max(r_c)})
            print(f"{key:14s} {k:8s} / render = {med[k] / med['render']:.3f} ({min(r_b):.3f}-{max(r_b):.3f} per round)   "
                  f"/ radiance = {med[k] / med['radiance']:.3f} ({min(r_c):.3f}-{max(r_c):.3f})", flush=True)
        del rays, states, L, frames
        torch.cuda.empty_cache()
        # the panorama: from the camera's position, looking where it looks
        c = d.camera
        o = np.array(list(c.center))
        f = np.array(list(c.lookat)) - o if c.has_lookat else np.array(list(c.direction))
        pano = crt.make_lens("equirect", origin=tuple(o), forward=tuple(f), up=tuple(c.up))
        pcam = crt.resolve_camera(crt.camera_with(d.camera, image_w=pw, image_h=ph, samples_per_pixel=spp), 1)
        out = torch.empty((ph, pw, 3), dtype=torch.float64, device="cuda")

        def panorama():
            scene.render_lens_async(0, pcam, pano, out.data_ptr(), stream)

        panorama()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0, (key, "the panorama is empty")
        v = [timed(panorama) for _ in range(a.reps)]
        rate = [pw * ph * spp / (x * 1e3) for x in v]
        rows.append({"scene": key, "kind": "equirect", "w": pw, "h": ph, "spp": spp, "call": "lens", "ms": float(np.median(v)),
                     "ms_min": min(v), "ms_max": max(v), "mpaths_s": float(np.median(rate))})
        print(f"{key:14s} equirect {pw} x {ph} x {spp}  lens     {np.median(v):9.2f} ms ({min(v):.2f}-{max(v):.2f})  "
              f"{np.median(rate):8.1f} M paths/s", flush=True)
        del out
        scene.close()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
