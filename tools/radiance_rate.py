"""Radiance-query throughput: crt_radiance_async's fast route (radiance_kernel) and plain route
(CRT_RADIANCE_PLAIN) against crt_render_async of the same job, alternating within one run.
M paths/s per (scene, ray set, route) and the ratio to the render; DESIGN section 6e.

  python tools/radiance_rate.py [--reps 7] [--spp 48] [--probes 4000000] [--scenes rtow_final,cornell,christmas_tree]

Scenes with their own cameras (rtow_final, cornell and millions are BASELINE configs 2, 3 and 4;
christmas_tree is a small HBM-resident scene; `--scenes millions` is optional). Ray sets:
  camera  the camera's own rays and states from crt_camera_rays_async at min(--spp, what keeps the job
          under --max-paths) samples a pixel: the job crt_render_async renders, path for path;
  probes  seeded rays from surface points (the centre rays' hit points, pushed off the surface, into the
          normal's hemisphere), default seeding: what an irradiance probe or a lightmap sends.
The calls are timed with device events after a warm-up, medians of --reps with min-max; every fast
output is compared with the plain route's bytes before a rate is printed, and the camera set's
summed radiance with the render's frame."""
import argparse
import json
import sys
from pathlib import Path

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import cpp_raytracer_amd as crt  # noqa: E402
import denoise_model as dm  # noqa: E402

SCENES = {"rtow_final": ("rtow_final", 42), "cornell": ("cornell", None), "christmas_tree": ("christmas_tree", None),
          "millions": ("millions", 42)}


def probe_rays(scene, cam, n):
    centre = dm.centre_rays(cam).reshape(-1, 6)
    h = scene.closest_hits(centre)
    h = h[h["prim"] >= 0]
    rng = np.random.default_rng(13)
    pick = rng.integers(0, len(h), n)
    p, nrm = h["point"][pick], h["normal"][pick]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = nrm + d  # cosine-weighted about the normal
    return np.concatenate([p + 1e-6 * nrm, d], 1)


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
    ap.add_argument("--spp", type=int, default=48)
    ap.add_argument("--max-paths", type=int, default=48_000_000)
    ap.add_argument("--probes", type=int, default=4_000_000)
    ap.add_argument("--scenes", default="rtow_final,cornell,christmas_tree")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    for key in a.scenes.split(","):
        name, seed = SCENES[key]
        d = crt.SceneData.named(name, seed)
        pixels = d.camera.image_w * d.camera.image_h
        spp = max(4, min(a.spp, a.max_paths // pixels) // 4 * 4)  # whole sample chunks
        scene = crt.GpuScene(d)
        scene.upload(0)
        cam = crt.resolve_camera(crt.camera_with(d.camera, samples_per_pixel=spp), 1)
        bg = tuple(cam.background)
        frame = torch.empty((cam.image_h, cam.image_w, 3), dtype=torch.float64, device="cuda")

        def render():
            scene.render_async(0, cam, frame.data_ptr(), stream)

        crays, cstates = scene.camera_rays(cam)
        sets = {"camera": (crays, cstates), "probes": (torch.from_numpy(probe_rays(scene, cam, a.probes)).cuda(), None)}
        for set_name, (rays, states) in sets.items():
            n = len(rays)
            outs = {k: torch.empty((n, 3), dtype=torch.float64, device="cuda") for k in ("fast", "plain")}

            def query(k):
                scene.radiance_async(0, rays.data_ptr(), n, outs[k].data_ptr(), states.data_ptr() if states is not None else 0,
                                     max_depth=cam.max_depth, background=bg, t_min=cam.t_min, base_seed=7,
                                     flags=crt.CRT_RADIANCE_PLAIN if k == "plain" else 0, stream=stream)

            calls = {"render": render, "fast": lambda: query("fast"), "plain": lambda: query("plain")}
            for c in calls.values():  # warm-up, then the checks
                c()
            torch.cuda.synchronize()
            assert torch.equal(outs["fast"].view(torch.int64), outs["plain"].view(torch.int64)), (key, set_name, "fast != plain")
            if set_name == "camera":
                smp = outs["fast"].view(cam.image_h, cam.image_w, spp, 3)
                total = None
                for c0 in range(0, spp, 4):  # the render's sums: per chunk of 4 samples in order, chunks in order
                    u = ((smp[:, :, c0] + smp[:, :, c0 + 1]) + smp[:, :, c0 + 2]) + smp[:, :, c0 + 3]
                    total = u if total is None else total + u
                assert crt.sample_chunk_len(spp) == 4
                assert torch.equal((total * (1 / float(spp))).view(torch.int64), frame.view(torch.int64)), (key, "render identity")
                del smp, total
            ms = {k: [] for k in calls}
            for _ in range(a.reps):  # alternating: one of each per round
                for k, c in calls.items():
                    ms[k].append(timed(c))
            ref = float(np.median(ms["render"]))
            for k, v in ms.items():
                paths = n if k != "render" else pixels * spp
                rate = [paths / (x * 1e3) for x in v]
                row = {"scene": key, "set": set_name, "paths": paths, "spp": spp, "call": k, "ms": float(np.median(v)),
                       "ms_min": min(v), "ms_max": max(v), "mpaths_s": float(np.median(rate)), "min": min(rate), "max": max(rate)}
                if set_name == "camera":
                    row["ratio_to_render"] = float(np.median(v)) / ref
                rows.append(row)
                ratio = f"  {np.median(v) / ref:5.2f} x the render's time" if set_name == "camera" and k != "render" else ""
                print(f"{key:14s} {set_name:7s} {paths:9d} paths  {k:7s} {np.median(v):9.2f} ms ({min(v):.2f}-{max(v):.2f})  "
                      f"{np.median(rate):9.1f} M paths/s ({min(rate):.1f}-{max(rate):.1f}){ratio}", flush=True)
            del outs
        del crays, cstates, sets, frame
        scene.close()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
