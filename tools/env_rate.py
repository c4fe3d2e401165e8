"""What a cube-map environment costs a radiance query: crt_radiance_env_async (both filters) against
crt_radiance_async with the constant background on the same rays and states, alternating within one
run. Milliseconds per call and the ratio to the constant-background call; DESIGN section 6k.

  python tools/env_rate.py [--reps 7] [--spp 48] [--probes 4000000] [--face 256] [--scenes rtow_final,cornell]

rtow_final and cornell with their own cameras are BASELINE configs 2 and 3. Ray sets (radiance_rate.py's):
  camera  the camera's own rays and states from crt_camera_rays_async at min(--spp, what keeps the job
          under --max-paths) samples a pixel;
  probes  seeded rays from surface points into the normal's hemisphere, default seeding.
The environment is a seeded random map of face size --face in [0, 4) behind a rotated basis. The calls
are timed with device events after a warm-up, medians of --reps with min-max; every environment output
is compared with the plain route's bytes (CRT_RADIANCE_PLAIN) before a time is printed."""
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
from radiance_rate import SCENES, probe_rays, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spp", type=int, default=48)
    ap.add_argument("--max-paths", type=int, default=48_000_000)
    ap.add_argument("--probes", type=int, default=4_000_000)
    ap.add_argument("--face", type=int, default=256)
    ap.add_argument("--scenes", default="rtow_final,cornell")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    n = a.face
    texels = torch.from_numpy(np.random.default_rng(3).random((6 * n, n, 3)) * 4.0).cuda()
    envs = {f: crt.make_env(texels, forward=(0.3, -0.5, -0.8), up=(0.1, 1.0, 0.2), filter=f) for f in ("nearest", "bilinear")}
    for key in a.scenes.split(","):
        name, seed = SCENES[key]
        d = crt.SceneData.named(name, seed)
        pixels = d.camera.image_w * d.camera.image_h
        spp = max(4, min(a.spp, a.max_paths // pixels) // 4 * 4)  # whole sample chunks
        scene = crt.GpuScene(d)
        scene.upload(0)
        cam = crt.resolve_camera(crt.camera_with(d.camera, samples_per_pixel=spp), 1)
        bg = tuple(cam.background)
        crays, cstates = scene.camera_rays(cam)
        sets = {"camera": (crays, cstates), "probes": (torch.from_numpy(probe_rays(scene, cam, a.probes)).cuda(), None)}
        for set_name, (rays, states) in sets.items():
            paths = len(rays)
            out = torch.empty((paths, 3), dtype=torch.float64, device="cuda")
            check = torch.empty((paths, 3), dtype=torch.float64, device="cuda")

            def query(env, dst=out, flags=0):
                scene.radiance_async(0, rays.data_ptr(), paths, dst.data_ptr(), states.data_ptr() if states is not None else 0,
                                     max_depth=cam.max_depth, background=bg, t_min=cam.t_min, base_seed=7, flags=flags,
                                     stream=stream, env=envs[env].view if env else None)

            calls = {"constant": lambda: query(None), "nearest": lambda: query("nearest"), "bilinear": lambda: query("bilinear")}
            query(None, check)
            for f in envs:  # warm-up and the check: the fast route's bytes are the plain route's, and the map is seen
                query(f)
                query(f, check, crt.CRT_RADIANCE_PLAIN)
                torch.cuda.synchronize()
                assert torch.equal(out.view(torch.int64), check.view(torch.int64)), (key, set_name, f, "fast != plain")
            query(None, check)
            torch.cuda.synchronize()
            assert not torch.equal(out.view(torch.int64), check.view(torch.int64)), (key, set_name, "the map is not seen")
            ms = {k: [] for k in calls}
            for _ in range(a.reps):  # alternating: one of each per round
                for k, c in calls.items():
                    ms[k].append(timed(c))
            ref = float(np.median(ms["constant"]))
            for k, v in ms.items():
                med = float(np.median(v))
                rows.append({"scene": key, "set": set_name, "paths": paths, "spp": spp, "face": n, "call": k, "ms": med,
                             "ms_min": min(v), "ms_max": max(v), "ratio_to_constant": med / ref})
                print(f"{key:14s} {set_name:7s} {paths:9d} paths  {k:9s} {med:9.2f} ms ({min(v):.2f}-{max(v):.2f})  "
                      f"{med / ref:6.3f} x the constant background's time", flush=True)
            del out, check
        del crays, cstates, sets
        scene.close()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
