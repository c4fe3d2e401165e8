"""Ray-query throughput: crt_closest_hits (host arrays, blocking: the only route before
crt_trace_async) against crt_trace_async's plain route, fast route and fast any-hit on device
buffers, alternating within one run. Mrays/s per (scene, ray set, call); DESIGN section 6d.

  python tools/ray_query_rate.py [--reps 7] [--rays 4000000] [--scenes rtow_final,cornell,christmas_tree,millions]

Scenes with their own cameras (rtow_final, cornell and millions are BASELINE configs 2, 3 and 4;
christmas_tree is a small HBM-resident scene); ray sets: the camera's centre rays, their
reflected secondaries, and seeded random rays over and beyond the scene box. The device calls are
timed with events after a warm-up, medians with min-max; every timed output is compared with the
plain route's bytes before a rate is printed. As context, the render kernel's own rays / kernel_ms
from crt_render_count on the same scene."""
import argparse
import json
import sys
import time
from pathlib import Path

import os

os.environ["CRT_TRACE_FAST"] = "1"  # "fast" means the fast instances, also where they are not the default
import torch  # first: the library then shares torch's HIP runtime
import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import cpp_raytracer_amd as crt  # noqa: E402
import denoise_model as dm  # noqa: E402

SCENES = {"rtow_final": ("rtow_final", 42), "cornell": ("cornell", None), "christmas_tree": ("christmas_tree", None),
          "millions": ("millions", 42)}


def random_rays(scene, n):
    nodes, _ = scene.export_bvh()
    b = nodes[0]["bounds"]
    lo, hi = np.maximum(b[0::2], -1e3), np.minimum(b[1::2], 1e3)
    rng = np.random.default_rng(7)
    o = lo - 0.25 * (hi - lo) + rng.random((n, 3)) * 1.5 * (hi - lo)
    d = rng.normal(size=(n, 3))
    d[: n // 20, rng.integers(0, 3)] = 0.0
    return np.concatenate([o, d], 1)


def device_call(scene, rays, flags):
    n = len(rays)
    any_hit = bool(flags & crt.CRT_TRACE_ANY)
    out = torch.empty((n, 4 if any_hit else 72), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        scene.trace_async(0, rays.data_ptr(), n, 0 if any_hit else out.data_ptr(), out.data_ptr() if any_hit else 0,
                          flags=flags, stream=stream)
    return call, out


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rays", type=int, default=4_000_000)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for key in a.scenes.split(","):
        name, seed = SCENES[key]
        d = crt.SceneData.named(name, seed)
        scene = crt.GpuScene(d)
        scene.upload(0)
        cam = crt.resolve_camera(d.camera, 1)
        centre = dm.centre_rays(cam).reshape(-1, 6)
        first = scene.closest_hits(centre)
        hit = first["prim"] >= 0
        dd, nn = centre[hit, 3:], first["normal"][hit]
        dn = (dd[:, 0] * nn[:, 0] + dd[:, 1] * nn[:, 1]) + dd[:, 2] * nn[:, 2]
        sets = {"centre": centre, "reflected": np.concatenate([first["point"][hit], dd - 2 * dn[:, None] * nn], 1),
                "random": random_rays(scene, a.rays)}
        small = crt.camera_with(d.camera, samples_per_pixel=4)
        st = scene.render_count(0, crt.resolve_camera(small, 1))
        render_rate = st.rays / (st.kernel_ms * 1e3)
        for set_name, host_rays in sets.items():
            dev = torch.from_numpy(np.ascontiguousarray(host_rays)).cuda()
            calls = {"plain": device_call(scene, dev, crt.CRT_TRACE_PLAIN), "fast": device_call(scene, dev, 0),
                     "fast any": device_call(scene, dev, crt.CRT_TRACE_ANY)}
            ms = {k: [] for k in ("closest_hits (host)", *calls)}
            for k, (call, _) in calls.items():  # warm-up, then the checks against the plain route's bytes
                call()
            torch.cuda.synchronize()
            ref = calls["plain"][1].cpu().numpy()
            assert (calls["fast"][1].cpu().numpy() == ref).all(), (key, set_name, "fast != plain")
            prim = ref.view(crt.HIT_DTYPE)["prim"].reshape(-1)
            assert ((calls["fast any"][1].cpu().numpy().view(np.uint32).reshape(-1) == 1) == (prim >= 0)).all()
            for _ in range(a.reps):  # alternating: one of each per round
                t0 = time.perf_counter()
                host = scene.closest_hits(host_rays)
                ms["closest_hits (host)"].append((time.perf_counter() - t0) * 1e3)
                for k, (call, _) in calls.items():
                    ms[k] += timed(call, 1)
            assert host.tobytes() == ref.tobytes(), (key, set_name, "closest_hits != plain")
            for k, v in ms.items():
                rate = [len(host_rays) / (x * 1e3) for x in v]
                rows.append({"scene": key, "set": set_name, "rays": len(host_rays), "call": k,
                             "mrays_s": float(np.median(rate)), "min": min(rate), "max": max(rate),
                             "hit_share": float((prim >= 0).mean()), "render_kernel_mrays_s": render_rate})
                print(f"{key:11s} {set_name:9s} {len(host_rays):8d} rays  {k:20s} {np.median(rate):9.1f} Mrays/s "
                      f"({min(rate):.1f}-{max(rate):.1f})  [render kernel {render_rate:.1f}]", flush=True)
        scene.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
