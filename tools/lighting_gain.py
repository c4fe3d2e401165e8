"""What sampling an environment and the scene's lights together buys and costs: the four lightings of
crt_radiance_lit_async (unlit: a plain map, nothing sampled; the map's sampler only; the lights only; both) on
the same camera rays and states, and what cutting a lit panorama into passes costs. DESIGN section 6q.

  python tools/lighting_gain.py [--reps 5] [--spp 16] [--width 640] [--face 64] [--scenes cornell,rtow_final_lights]
                                [--pano 2048x1024x64] [--out FILE]

cornell (BASELINE config 3, seen from outside through its open front) and rtow_final_lights with their own
cameras at --width pixels across, under an n = --face map of 0.5 with one texel at 1e4 (env_nee_gain's
direction for cornell, the same for rtow_final_lights as for rtow_final), nearest filter. For each scene:
  - milliseconds a call of the four lightings on the camera's --spp samples a pixel, alternating within one
    run, timed with device events after a warm-up: medians of --reps with min-max, and the ratios to unlit;
  - per-pixel RMSE of the frame (the mean over a pixel's samples) against a reference: a run with both
    samplers 16 times as long with other seeds; for every lighting at --spp samples, and for unlit at the
    number of samples it traces in the time of "both" (equal time).
Then a --pano EQUIRECT frame of the first scene under both samplers: one render_lens call against
LensRender in 1, 4 and 16 passes (the same bits), milliseconds each, medians of --reps.
Nothing here is a pass/fail bar."""
import argparse
import json
import sys
from pathlib import Path

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import cpp_raytracer_amd as crt  # noqa: E402
from env_nee_gain import sun_map  # noqa: E402
from radiance_rate import timed  # noqa: E402

SCENES = {"cornell": ("cornell", None), "rtow_final_lights": ("rtow_final_lights", 42)}
SUN = {"cornell": (-0.2, 0.35, -1.0), "rtow_final_lights": (0.3, 0.8, 0.5)}
ENTRIES = ("unlit", "sampler", "lights", "both")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--face", type=int, default=64)
    ap.add_argument("--scenes", default="cornell,rtow_final_lights")
    ap.add_argument("--pano", default="2048x1024x64")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    from cpp_raytracer_amd import _lighting_on
    for key in a.scenes.split(","):
        name, seed = SCENES[key]
        d = crt.SceneData.named(name, seed)
        w = a.width
        h = max(1, round(w * d.camera.image_h / d.camera.image_w))
        texels, _, _ = sun_map(a.face, SUN[key])
        t = torch.from_numpy(texels).cuda()
        plain_env = crt.make_env(t, filter="nearest")
        nee_env = crt.make_env(t, filter="nearest", importance=True)
        scene = crt.GpuScene(d)
        scene.upload(0)
        lights = scene.light_sampler(0)
        lit = {"unlit": crt.Lighting(env=plain_env), "sampler": crt.Lighting(env=nee_env),
               "lights": crt.Lighting(env=plain_env, lights=lights), "both": crt.Lighting(env=nee_env, lights=lights)}
        view = {k: _lighting_on("lighting_gain", v, None, None, scene, 0) for k, v in lit.items()}

        def job(spp, cam_seed):
            cam = crt.resolve_camera(crt.camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp), cam_seed)
            rays, states = scene.camera_rays(cam)
            return cam, rays, states

        def frame(cam, rays, states, entry, out=None):
            n = len(rays)
            out = torch.empty((n, 3), dtype=torch.float64, device="cuda") if out is None else out
            scene.radiance_async(0, rays.data_ptr(), n, out.data_ptr(), states.data_ptr(), max_depth=cam.max_depth,
                                 background=tuple(cam.background), t_min=cam.t_min, stream=stream, lighting=view[entry])
            return out

        def image(out, spp):
            return out.view(h * w, spp, 3).mean(1)

        cam, rays, states = job(a.spp, 1)
        out = frame(cam, rays, states, "unlit")
        for e in ENTRIES[1:]:
            frame(cam, rays, states, e, out)  # warm-up of all four
        torch.cuda.synchronize()
        ms = {e: [] for e in ENTRIES}
        for _ in range(a.reps):  # alternating: one of each per round
            for e in ENTRIES:
                ms[e].append(timed(lambda: frame(cam, rays, states, e, out)))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        ref = torch.zeros((h * w, 3), dtype=torch.float64, device="cuda")
        for k in range(16):  # the reference: 16 jobs of --spp under both samplers with other seeds
            c2, r2, s2 = job(a.spp, 1000 + k)
            ref += image(frame(c2, r2, s2, "both"), a.spp)
        ref /= 16

        def rmse(img):
            return float(torch.sqrt(((img - ref) ** 2).mean()))

        err = {e: rmse(image(frame(cam, rays, states, e), a.spp)) for e in ENTRIES}
        equal_spp = max(1, round(a.spp * med["both"] / med["unlit"]))
        c3, r3, s3 = job(equal_spp, 1)
        err["unlit_equal_time"] = rmse(image(frame(c3, r3, s3, "unlit"), equal_spp))
        torch.cuda.synchronize()
        rows.append({"scene": key, "w": w, "h": h, "spp": a.spp, "face": a.face, "ms": med,
                     "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
                     "equal_time_spp": equal_spp, "rmse": err, "ref_mean": float(ref.mean())})
        for e in ENTRIES:
            print(f"{key:17s} {w}x{h}x{a.spp:<3d} {e:8s} {med[e]:9.2f} ms ({min(ms[e]):.2f}-{max(ms[e]):.2f}) "
                  f"{med[e] / med['unlit']:.2f} x unlit; RMSE {err[e]:.4g} ({err['unlit'] / err[e]:.2f} x lower than unlit)", flush=True)
        print(f"{key:17s} unlit at {equal_spp} spp (the time of both): RMSE {err['unlit_equal_time']:.4g} "
              f"({err['unlit_equal_time'] / err['both']:.2f} x that of both); reference mean {rows[-1]['ref_mean']:.4g}", flush=True)
        if a.pano and key == a.scenes.split(",")[0]:
            pw_, ph_, pspp = (int(x) for x in a.pano.split("x"))
            c = d.camera
            o = tuple(c.center)
            f = tuple(np.array(list(c.lookat)) - np.array(o)) if c.has_lookat else tuple(c.direction)
            lens = crt.make_lens("equirect", origin=o, forward=f, up=tuple(c.up))
            pcam = crt.resolve_camera(crt.camera_with(d.camera, image_w=pw_, image_h=ph_, samples_per_pixel=pspp), 1)
            L = crt.sample_chunk_len(pspp)

            def passes(k):
                r = crt.LensRender(scene, pcam, lens, lighting=lit["both"])
                per = (pspp // k + L - 1) // L * L
                while not r.finished:
                    r.step(per)
                return r

            scene.render_lens(pcam, lens, lighting=lit["both"])  # warm-up
            torch.cuda.synchronize()
            pano = {"one_shot": [timed(lambda: scene.render_lens(pcam, lens, lighting=lit["both"])) for _ in range(a.reps)]}
            for k in (1, 4, 16):
                pano[f"passes_{k}"] = [timed(lambda: passes(k)) for _ in range(a.reps)]
            pmed = {k: float(np.median(v)) for k, v in pano.items()}
            rows.append({"scene": key, "pano": a.pano, "ms": pmed, "ms_min": {k: min(v) for k, v in pano.items()},
                         "ms_max": {k: max(v) for k, v in pano.items()}})
            for k, v in pmed.items():
                print(f"{key:17s} panorama {a.pano} under both {k:10s} {v:9.2f} ms ({min(pano[k]):.2f}-{max(pano[k]):.2f}) "
                      f"{v / pmed['one_shot']:.3f} x one shot", flush=True)
        del lights, lit, view
        scene.close()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
