"""What luminance sampling of a cube-map environment buys and costs: crt_radiance_env_sampled_async
against crt_radiance_env_async on the same camera rays and states, under a map with a small sun.
DESIGN section 6l.

  python tools/env_nee_gain.py [--reps 5] [--spp 16] [--width 640] [--face 64] [--scenes rtow_final,cornell]
                               [--filters nearest,bilinear]

rtow_final and cornell with their own cameras (BASELINE configs 2 and 3; cornell's camera stands outside
the box and looks in through its open front) at --width pixels across. The map has face size --face,
every texel 0.5 but one at 1e4, in the direction SUN[scene] (for cornell: out of the open front, towards
the camera and up). env_pdf follows the texel a direction falls in whatever the filter, so under
BILINEAR the bright texel's light also arrives through the half-texel rim around it, where the sampler's
density is the neighbours': both filters are measured. For each scene and filter:
  - milliseconds a call of both entries on the camera's --spp samples a pixel, alternating within one
    run, timed with device events after a warm-up: medians of --reps with min-max, and the ratio;
  - per-pixel RMSE of the frame (the mean over a pixel's samples) against a reference: a sampled run 16
    times as long with another seed; for the unsampled entry at --spp samples (equal sample count) and
    at the number of samples it traces in the sampled call's time (equal time), for the sampled entry at
    --spp. The pixels that see the bright texel directly carry the same error in both and are left out.
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
import env_model as em  # noqa: E402
import env_nee_model as nm  # noqa: E402
from radiance_rate import SCENES, timed  # noqa: E402

SUN = {"rtow_final": (0.3, 0.8, 0.5), "cornell": (-0.2, 0.35, -1.0)}


def sun_map(n, direction):
    """The map and the (row, column) of its bright texel: the texel `direction` looks up."""
    t = np.full((6 * n, n, 3), 0.5)
    menv = em.make(t)
    ok, face, _, _, _, fx, fy = nm.project(menv, [direction])
    row = int(face[0]) * n + int(np.clip(np.floor(fy[0]), 0, n - 1))
    col = int(np.clip(np.floor(fx[0]), 0, n - 1))
    t[row, col] = 1e4
    return t, row, col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--filters", default="nearest,bilinear")
    ap.add_argument("--face", type=int, default=64)
    ap.add_argument("--scenes", default="rtow_final,cornell")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    for key, filt in ((k, f) for k in a.scenes.split(",") for f in a.filters.split(",")):
        name, seed = SCENES[key]
        d = crt.SceneData.named(name, seed)
        w = a.width
        h = max(1, round(w * d.camera.image_h / d.camera.image_w))
        texels, row, col = sun_map(a.face, SUN[key])
        t = torch.from_numpy(texels).cuda()
        plain_env = crt.make_env(t, filter=filt)
        nee_env = crt.make_env(t, filter=filt, importance=True)
        scene = crt.GpuScene(d)
        scene.upload(0)

        def job(spp, cam_seed):
            cam = crt.resolve_camera(crt.camera_with(d.camera, image_w=w, image_h=h, samples_per_pixel=spp), cam_seed)
            rays, states = scene.camera_rays(cam)
            return cam, rays, states

        def frame(cam, rays, states, env, out=None):
            n = len(rays)
            out = torch.empty((n, 3), dtype=torch.float64, device="cuda") if out is None else out
            scene.radiance_async(0, rays.data_ptr(), n, out.data_ptr(), states.data_ptr(), max_depth=cam.max_depth,
                                 background=tuple(cam.background), t_min=cam.t_min, stream=stream,
                                 env=env.view, sampler=env.sampler or 0)
            return out

        def image(out, spp):
            return out.view(h * w, spp, 3).mean(1)

        cam, rays, states = job(a.spp, 1)
        out = frame(cam, rays, states, plain_env)
        frame(cam, rays, states, nee_env, out)  # warm-up of both
        torch.cuda.synchronize()
        ms = {"unsampled": [], "sampled": []}
        for _ in range(a.reps):  # alternating: one of each per round
            ms["unsampled"].append(timed(lambda: frame(cam, rays, states, plain_env, out)))
            ms["sampled"].append(timed(lambda: frame(cam, rays, states, nee_env, out)))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        ratio = med["sampled"] / med["unsampled"]
        # the reference: 16 sampled jobs of --spp with other seeds
        ref = torch.zeros((h * w, 3), dtype=torch.float64, device="cuda")
        for k in range(16):
            c2, r2, s2 = job(a.spp, 1000 + k)
            ref += image(frame(c2, r2, s2, nee_env), a.spp)
        ref /= 16
        # the pixels whose centre ray leaves the scene straight into the bright texel
        centre = rays.view(h * w, a.spp, 6)[:, 0, 3:].cpu().numpy()
        ok, face, _, _, _, fx, fy = nm.project(em.make(texels), centre)
        n = a.face
        direct = ok & (face * n + np.clip(np.floor(fy), 0, n - 1) == row) & (np.clip(np.floor(fx), 0, n - 1) == col)
        keep = torch.from_numpy(~direct).cuda()

        def rmse(img):
            return float(torch.sqrt(((img - ref)[keep] ** 2).mean()))

        equal_spp = max(1, round(a.spp * ratio))
        c3, r3, s3 = job(equal_spp, 1)
        err = {"unsampled": rmse(image(frame(cam, rays, states, plain_env), a.spp)),
               "sampled": rmse(image(frame(cam, rays, states, nee_env), a.spp)),
               "unsampled_equal_time": rmse(image(frame(c3, r3, s3, plain_env), equal_spp))}
        torch.cuda.synchronize()
        rows.append({"scene": key, "filter": filt, "w": w, "h": h, "spp": a.spp, "face": n, "sun_texel": [row, col],
                     "direct_pixels": int(direct.sum()), "ms": med, "ms_min": {k: min(v) for k, v in ms.items()},
                     "ms_max": {k: max(v) for k, v in ms.items()}, "ratio": ratio, "equal_time_spp": equal_spp,
                     "rmse": err, "ref_mean": float(ref[keep].mean())})
        for k in ("unsampled", "sampled"):
            print(f"{key:11s} {filt:8s} {w}x{h}x{a.spp:<3d} {k:9s} {med[k]:9.2f} ms ({min(ms[k]):.2f}-{max(ms[k]):.2f})", flush=True)
        print(f"{key:11s} {filt:8s} sampled / unsampled time = {ratio:.3f}; RMSE against the reference (mean {rows[-1]['ref_mean']:.4g}, "
              f"{int(direct.sum())} direct pixels left out): unsampled {err['unsampled']:.4g}, sampled {err['sampled']:.4g} "
              f"({err['unsampled'] / err['sampled']:.2f} x lower) at {a.spp} spp; unsampled at {equal_spp} spp (equal time) "
              f"{err['unsampled_equal_time']:.4g} ({err['unsampled_equal_time'] / err['sampled']:.2f} x)", flush=True)
        scene.close()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
