"""Probe-bake throughput: crt_probes_async against its own middle stage and against the route a
caller had to take before it, alternating within one run. DESIGN section 6f.

  python tools/probe_rate.py [--reps 7] [--probes 4096] [--samples 1024] [--mode sphere]
                             [--scenes rtow_final,cornell,christmas_tree] [--out FILE]

Probe points are hit points of the scene camera's centre rays, pushed off the surface along the normal
(with --mode hemisphere the normals are the hits'). Per scene:
  (a) probes    GpuScene.probes_async: generate, trace and reduce on the device, in the batches the
                library picks (256 MiB of scratch: two batches at the default size); `probes_1` is
                the same call with batch_probes = --probes, one batch;
  (b) radiance  crt_radiance_async alone, on the very rays and states (a) generates
                (crt_probe_rays_async, called once outside the timing);
  (c) by hand   today's route: the same rays, already expanded to one a record in a tensor, then
                crt_radiance_async, then the basis and the sum over the samples in torch.
(a)/(b) is what generating and reducing cost; (a)/(c) what the bake saves. The calls are timed with
device events after a warm-up, medians of --reps with min-max. Before any rate is printed (a)'s output
is compared, byte for byte, with tests/probe_model.py's numpy reduction of (b)'s output."""
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
import probe_model as pm  # noqa: E402

SCENES = {"rtow_final": ("rtow_final", 42), "cornell": ("cornell", None), "christmas_tree": ("christmas_tree", None),
          "millions": ("millions", 42)}


def probe_points(scene, cam, n):
    h = scene.closest_hits(dm.centre_rays(cam).reshape(-1, 6))
    h = h[h["prim"] >= 0]
    pick = np.random.default_rng(13).integers(0, len(h), n)
    p, nrm = np.array(h["point"][pick], np.float64), np.array(h["normal"][pick], np.float64)
    return p + 1e-6 * nrm, nrm


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def torch_basis(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return torch.stack([torch.full_like(x, pm.C0), pm.C1 * y, pm.C1 * z, pm.C1 * x, pm.C2 * (x * y), pm.C2 * (y * z),
                        pm.C6 * ((3.0 * z) * z - 1.0), pm.C2 * (x * z), pm.C8 * (x * x - y * y)], -1)


def model_check(key, coeff, rays, L, n, S, sphere):
    """(a)'s coefficients against the model's reduction of (b)'s radiance, in slices of 256 probes."""
    dirs = rays[:, 3:].cpu().numpy()
    L = L.cpu().numpy()
    got = coeff.cpu().numpy()
    for p0 in range(0, n, 256):
        p1 = min(n, p0 + 256)
        want = pm.reduce(dirs[p0 * S:p1 * S], L[p0 * S:p1 * S], S, sphere)
        assert np.array_equal(dm.bits(got[p0:p1]), dm.bits(want)), (key, "probes != the model's reduction of radiance", p0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--mode", default="sphere", choices=["sphere", "hemisphere"])
    ap.add_argument("--scenes", default="rtow_final,cornell,christmas_tree")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    n, S, sphere = a.probes, a.samples, a.mode == "sphere"
    K, W = (9, pm.W_SPHERE) if sphere else (1, pm.W_HEMISPHERE)
    for key in a.scenes.split(","):
        name, seed = SCENES[key]
        d = crt.SceneData.named(name, seed)
        scene = crt.GpuScene(d)
        scene.upload(0)
        cam = crt.resolve_camera(d.camera, 1)
        bg = tuple(cam.background)
        p, nrm = probe_points(scene, cam, n)
        points = torch.from_numpy(p).cuda()
        normals = None if sphere else torch.from_numpy(nrm).cuda()
        rays, states = scene.probe_rays(points, normals, samples=S, mode=a.mode, base_seed=7)
        coeff = torch.empty((n, K, 3), dtype=torch.float64, device="cuda")
        coeff_1 = torch.empty_like(coeff)
        L = torch.empty((n * S, 3), dtype=torch.float64, device="cuda")
        hand = [None]

        def probes(batch=0, out=coeff):
            scene.probes_async(0, points.data_ptr(), normals.data_ptr() if normals is not None else 0, n, out.data_ptr(),
                               samples=S, mode=a.mode, max_depth=cam.max_depth, background=bg, t_min=cam.t_min, base_seed=7,
                               batch_probes=batch, stream=stream)

        def radiance():
            scene.radiance_async(0, rays.data_ptr(), n * S, L.data_ptr(), states.data_ptr(), max_depth=cam.max_depth,
                                 background=bg, t_min=cam.t_min, stream=stream)

        def by_hand():
            radiance()
            if sphere:
                t = torch_basis(rays[:, 3:])[:, :, None] * L[:, None, :]
            else:
                t = L[:, None, :]
            hand[0] = t.view(n, S, K, 3).sum(1) * (W / float(S))

        calls = {"probes": probes, "probes_1": lambda: probes(n, coeff_1), "radiance": radiance, "by_hand": by_hand}
        for c in calls.values():  # warm-up, then the checks
            c()
        torch.cuda.synchronize()
        model_check(key, coeff, rays, L, n, S, sphere)
        assert torch.equal(coeff.view(torch.int64), coeff_1.view(torch.int64)), (key, "one batch != the default batches")
        scale = float(coeff.abs().max())
        drift = float((hand[0] - coeff).abs().max())  # torch's sum has an order of its own: close, not equal
        assert drift <= 1e-9 * max(1.0, scale), (key, "the hand-made route is not the same estimate", drift)
        hand[0] = None
        ms = {k: [] for k in calls}
        for _ in range(a.reps):  # alternating: one of each per round
            for k, c in calls.items():
                ms[k].append(timed(c))
            hand[0] = None
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, v in ms.items():
            rate = [n * S / (x * 1e3) for x in v]
            rows.append({"scene": key, "mode": a.mode, "probes": n, "samples": S, "call": k, "ms": med[k], "ms_min": min(v),
                         "ms_max": max(v), "mpaths_s": float(np.median(rate)), "hand_drift": drift})
            print(f"{key:14s} {a.mode:10s} {n} x {S}  {k:8s} {med[k]:9.2f} ms ({min(v):.2f}-{max(v):.2f})  "
                  f"{np.median(rate):8.1f} M paths/s", flush=True)
        for k in ("probes", "probes_1"):
            r_ab = [x / y for x, y in zip(ms[k], ms["radiance"])]
            r_ac = [x / y for x, y in zip(ms[k], ms["by_hand"])]
            rows.append({"scene": key, "mode": a.mode, "call": "ratios", "of": k, "a_over_b": med[k] / med["radiance"],
                         "a_over_b_min": min(r_ab), "a_over_b_max": max(r_ab), "a_over_c": med[k] / med["by_hand"],
                         "a_over_c_min": min(r_ac), "a_over_c_max": max(r_ac)})
            print(f"{key:14s} {k:8s} (a)/(b) = {med[k] / med['radiance']:.3f} ({min(r_ab):.3f}-{max(r_ab):.3f} per round)   "
                  f"(a)/(c) = {med[k] / med['by_hand']:.3f} ({min(r_ac):.3f}-{max(r_ac):.3f})", flush=True)
        del rays, states, coeff, coeff_1, L, points, normals
        scene.close()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
