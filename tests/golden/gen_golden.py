"""Regenerate the golden fixtures of tests/golden/ from the REFERENCE's own code.

Runs only in a container that has /root/reference (the GPU box does not): builds
oracle/_ref/ref_driver (reference headers + RNG instrumentation shim, see oracle/Makefile), writes
the scenes as CRTS files with the library's named-scene builders, and asks the reference code for
  * Camera::init outputs            -> cameras.json
  * BVH node arrays + prim order    -> bvh_<scene>.npz
  * per-sample-seeded renders       -> render_<case>.npz  (per-pixel RGB, float64)
  * per-sample radiance             -> samples_<case>.npz
  * closest-hit records             -> hits_<scene>.npz
  * ray_color of probe rays         -> radiance_<scene>.npz (rays, states, depths, background,
                                       scene digest, rgb per depth)
  * closest-hit records of the edge-ray families (tests/edge_rays.py), through the default BVH
    and BVH(world, 8, 1)            -> hits_edge_rays.npz
Fixtures hold inputs and expected outputs only. Usage: python tests/golden/gen_golden.py
"""
from __future__ import annotations

import hashlib
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import cpp_raytracer_amd as crt  # noqa: E402
from cpp_raytracer_amd import camera_with  # noqa: E402

GOLD = Path(__file__).resolve().parent
REF = ROOT / "oracle" / "_ref" / "ref_driver"

# (case, scene, seed, camera overrides, base_seed, crop (r0, r1, c0, c1) or None)
RENDER_CASES = [
    ("config1", "config1", None, {}, 7, None),
    ("rtow_crop", "rtow_final", 42, dict(image_w=1200, image_h=800, samples_per_pixel=8, max_depth=50),
     11, (360, 424, 560, 624)),
    ("rtow_glass_crop", "rtow_final", 42, dict(image_w=1200, image_h=800, samples_per_pixel=16, max_depth=50),
     12, (330, 362, 580, 644)),
    ("cornell_crop", "cornell", None, dict(image_w=600, image_h=600, samples_per_pixel=4, max_depth=1000),
     13, (250, 314, 200, 264)),
    ("cornell_empty_small", "cornell_empty", None, dict(image_w=40, image_h=40, samples_per_pixel=8, max_depth=50),
     14, None),
    ("parallelograms_small", "parallelograms", None, dict(image_w=48, image_h=48, samples_per_pixel=4),
     15, None),
    ("lights_crop", "rtow_final_lights", None, dict(image_w=400, image_h=225, samples_per_pixel=16),
     16, (80, 112, 180, 244)),
    ("christmas_crop", "christmas_tree", None, dict(image_w=270, image_h=152, samples_per_pixel=8),
     17, (40, 72, 110, 174)),
]
SAMPLE_CASES = [
    ("rtow_samples", "rtow_final", 42, dict(image_w=1200, image_h=800, samples_per_pixel=16, max_depth=50),
     21, (392, 400, 592, 600)),
    ("cornell_samples", "cornell", None, dict(image_w=600, image_h=600, samples_per_pixel=16, max_depth=1000),
     22, (296, 304, 296, 304)),
]
# the generic render<T> with the Scene itself as the world (Scene::hit_by / Box::hit_by, no BVH):
# (case, scene, seed, camera overrides, base_seed, crop, nesting group or None)
LINEAR_CASES = [
    ("cornell_linear", "cornell", None, dict(image_w=600, image_h=600, samples_per_pixel=8, max_depth=1000),
     18, (250, 282, 200, 264), None),
    ("lights_nested", "rtow_final_lights", None, dict(image_w=400, image_h=225, samples_per_pixel=8),
     19, (80, 112, 180, 244), 7),
    ("boxes_nested", "cornell", None, dict(image_w=96, image_h=96, samples_per_pixel=6, max_depth=200),
     20, None, 3),
]
BVH_SCENES = [("config1", None), ("rtow_final", 42), ("cornell", None), ("parallelograms", None),
              ("christmas_tree", None), ("bvh_pathological", None), ("rtow_final_lights", None)]
HIT_SCENES = [("rtow_final", 42, 4096), ("cornell", None, 4096), ("christmas_tree", None, 2048)]


def scene_file(tmp: Path, name: str, seed, overrides: dict) -> tuple[Path, crt.SceneData]:
    d = crt.SceneData.named(name, seed)
    d.camera = camera_with(d.camera, **overrides)
    p = tmp / f"{name}_{abs(hash(json.dumps(overrides, sort_keys=True)))}.crts"
    d.save(p)
    return p, d


def run(*args) -> str:
    r = subprocess.run([str(REF), *map(str, args)], check=True, capture_output=True, text=True)
    return r.stdout


def scene_digest(d: crt.SceneData) -> str:
    return hashlib.sha256(d.materials.tobytes() + d.objects.tobytes()).hexdigest()


def ppm_edge_frame() -> np.ndarray:
    """64x64 frame for the PPM-value goldens: ordinary colours, NaN / inf / -0 / denormals /
    huge values, and pixels whose gamma-encoded value lands within a few ulps of an integer
    after scaling (where sqrt and pow(x, 0.5) could truncate differently)."""
    rng = np.random.default_rng(99)
    f = rng.uniform(0, 3, (64, 64, 3))
    flat = f.reshape(-1, 3)
    specials = [np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, 1e-310, 1e300, -1.0, 1e-8]
    for i, v in enumerate(specials):
        flat[i] = [v, 0.5, 0.25]
        flat[len(specials) + i] = [0.5, v, v]
    scale = 255 + 0.999999
    k0 = 2 * len(specials)
    for j, k in enumerate(range(0, 700)):
        x2 = (k / scale) ** 2                      # r / (1 + L) with g = b = 0
        r = x2 / (1 - 0.2126 * x2) if x2 < 1 / 0.2126 else 1e9
        r = np.nextafter(r, np.inf) if j % 3 == 1 else (np.nextafter(r, -np.inf) if j % 3 == 2 else r)
        flat[k0 + j] = [r, 0.0, 0.0]
    return f


def tie_scene(seed: int, n: int) -> crt.SceneData:
    """A random scene of spheres, parallelograms and boxes on a 0.1 grid with ~10% signed-zero
    coordinates: many equal bounds and centroids, so the BVH folds and partitions see ties."""
    from cpp_raytracer_amd import CRT_BOX, CRT_PARALLELOGRAM, CRT_SPHERE, MATERIAL_DTYPE, OBJECT_DTYPE
    rng = np.random.default_rng(seed)
    d = crt.SceneData.named("config1")
    mats = np.zeros(2, MATERIAL_DTYPE)
    mats["kind"] = 1
    mats["color"] = 0.5
    objs = np.zeros(n, OBJECT_DTYPE)
    kinds = rng.choice([CRT_SPHERE, CRT_PARALLELOGRAM, CRT_BOX], n, p=[0.6, 0.3, 0.1])
    objs["kind"] = kinds
    objs["material"] = rng.integers(0, 2, n)
    v = np.round(rng.normal(0, 3, (n, 9)), 1)
    v[rng.random((n, 9)) < 0.1] = -0.0
    v[kinds == CRT_SPHERE, 3] = np.abs(v[kinds == CRT_SPHERE, 3]) + 0.1
    box = kinds == CRT_BOX
    v[box, 3:6] = v[box, 0:3] + np.abs(v[box, 3:6]) + 0.5
    objs["v"] = v
    d.materials, d.objects = mats, objs
    return d


def gen_bvh_ties(tmp: Path) -> None:
    """The reference's BVH (oracle/_ref bvh mode) of tie-heavy random scenes."""
    out = {}
    for seed, n in TIE_CASES:
        d = tie_scene(seed, n)
        p = tmp / f"ties{seed}.crts"
        d.save(p)
        run("bvh", p, tmp / "t.bin")
        b = (tmp / "t.bin").read_bytes()
        nn, npr = np.frombuffer(b, "<u8", 2)
        nodes = np.frombuffer(b, crt.NODE_DTYPE, int(nn), 16)
        k = f"s{seed}_"
        out[k + "objects"] = d.objects
        out[k + "materials"] = d.materials
        out[k + "bounds"] = nodes["bounds"]
        out[k + "index"] = nodes["index"]
        out[k + "count"] = nodes["count"]
        out[k + "axis"] = nodes["axis"]
        out[k + "order"] = np.frombuffer(b, "<u4", int(npr), 16 + 64 * int(nn))
    np.savez_compressed(GOLD / "bvh_ties.npz", **out)


TIE_CASES = [(4, 100), (5, 3000), (7, 20000)]


def gen_ppm(tmp: Path) -> None:
    """Image::send_as_ppm integers (oracle/_ref ppm mode) for the config-1 golden render and the
    edge frame."""
    cases = {"config1": np.load(GOLD / "render_config1.npz")["rgb"], "edges": ppm_edge_frame()}
    out = {}
    for name, frame in cases.items():
        h, w, _ = frame.shape
        src, dst = tmp / f"{name}.f64", tmp / f"{name}.ppm"
        src.write_bytes(np.ascontiguousarray(frame, "<f8").tobytes())
        run("ppm", src, h, w, dst)
        text = dst.read_text().split("\n")
        assert text[0] == "P3" and text[1] == f"{w} {h}" and text[2] == "255"
        vals = np.array([list(map(int, ln.split())) for ln in text[3:3 + h * w]], np.int64)
        out[f"{name}_values"] = vals.reshape(h, w, 3).astype(np.int32)
        if name == "edges":
            out["edges_frame"] = frame
        out[f"{name}_sha256"] = np.frombuffer(hashlib.sha256(dst.read_bytes()).digest(), np.uint8)
    np.savez_compressed(GOLD / "ppm_cases.npz", **out)


def gen_linear(tmp: Path, meta: dict) -> None:
    """Renders of the Scene itself (oracle/_ref render_linear / render_nested modes)."""
    for case, name, seed, ov, base, crop, group in LINEAR_CASES:
        p, d = scene_file(tmp, name, seed, ov)
        out = tmp / "l.npy"
        if group is None:
            run("render_linear", p, base, out, *(crop or ()))
        else:
            run("render_nested", p, base, out, group, *(crop or ()))
        rgb = np.load(out)
        np.savez_compressed(GOLD / f"render_{case}.npz", rgb=rgb)
        meta["renders"][case] = {"scene": name, "seed": seed, "camera": ov, "base_seed": base,
                                 "crop": crop, "shape": list(rgb.shape), "world": "scene" if group is None
                                 else f"nested scenes (group {group})"}


def gen_radiance(tmp: Path) -> None:
    """The reference's Camera::ray_color on rays that no camera made (oracle/_ref radiance mode):
    tests/probe_sets.py's fixture_records of each scene at depths 1, 3 and 50, with the scene's own
    background and the reference's t_min = 1e-5."""
    sys.path.insert(0, str(ROOT / "tests"))
    import probe_sets as ps
    for name in ps.FIXTURE_SCENES:
        d = ps.scene_data(crt, name)
        p = tmp / f"{name}_radiance.crts"
        d.save(p)
        rays, states = ps.fixture_records(crt, name)
        src, out = tmp / "q.bin", tmp / "q.npy"
        src.write_bytes(rays.astype("<f8").tobytes() + states.astype("<u4").tobytes())
        rgb = []
        for depth in ps.FIXTURE_DEPTHS:
            run("radiance", p, src, depth, out)
            rgb.append(np.load(out))
        np.savez_compressed(GOLD / f"radiance_{name}.npz", rays=rays, states=states,
                            depths=np.array(ps.FIXTURE_DEPTHS, np.uint32), background=np.array(d.camera.background[:]),
                            scene_digest=np.array(scene_digest(d)), rgb=np.stack(rgb))


def gen_edge_rays(tmp: Path, meta: dict) -> None:
    """The reference's BVH::hit_by over (1e-5, inf) (oracle/_ref hits mode) on tests/edge_rays.py's
    families, in FAMILIES' order (`all` is a permutation of them), through both of its trees: the
    driver hands the tree's two numbers to BVH's constructor (bvh.h:756). The same rays go through
    the world's three parts (er.WORLDS: the scenes in which the leaf filters run). Per world and
    tree: t, point and normal as float64, the primitive (unique by hit time, material and normal:
    never -2 or -3) and hit_from_outside. The worlds' digests go to golden.json's worlds (scenes
    holds the named scenes only)."""
    sys.path.insert(0, str(ROOT / "tests"))
    import edge_rays as er
    w = er.world(crt)
    rays = np.concatenate([w.rays[k] for k in er.FAMILIES])
    src, dst = tmp / "e.bin", tmp / "e.npy"
    src.write_bytes(rays.astype("<f8").tobytes())
    out = {"rays": rays, "families": np.array(er.FAMILIES)}
    for part, d in w.data.items():
        p = tmp / f"edge_rays_{part}.crts"
        d.save(p)
        out[part + "_scene_digest"] = np.array(scene_digest(d))
        for tree, kw in er.TREES.items():
            run("hits", p, src, dst, kw.get("num_buckets", 32), kw.get("max_prims_in_node", 12))
            h = np.load(dst)
            assert (h[:, 7] >= -1).all(), "a hit the driver could not give to one primitive"
            out[f"{part}_{tree}_t_point_normal"] = h[:, :7]
            out[f"{part}_{tree}_prim"] = h[:, 7].astype(np.int16)
            out[f"{part}_{tree}_front"] = h[:, 8].astype(np.uint8)
        meta.setdefault("worlds", {})["edge_rays_" + part] = {"seed": er.SEED, "objects": int(len(d.objects)),
                                                              "materials": int(len(d.materials)), "sha256": scene_digest(d)}
    np.savez_compressed(GOLD / "hits_edge_rays.npz", **out)


def main() -> None:
    subprocess.run(["make", "-C", str(ROOT / "oracle"), "ref"], check=True)
    meta = {"generator": "tests/golden/gen_golden.py", "reference": "DeltaPavonis/cpp_raytracer (oracle/_ref)",
            "scenes": {}, "renders": {}, "cameras": {}}
    with tempfile.TemporaryDirectory() as td:
        tmp = Path(td)
        # scenes + cameras + BVHs
        for name, seed in BVH_SCENES:
            p, d = scene_file(tmp, name, seed, {})
            meta["scenes"][name] = {"seed": seed, "objects": int(len(d.objects)),
                                    "materials": int(len(d.materials)), "sha256": scene_digest(d)}
            cam = {}
            for line in run("camera", p).splitlines():
                k, *vals = line.split()
                cam[k] = [float(v) if k != "size" else int(v) for v in vals]
            meta["cameras"][name] = cam
            out = tmp / "bvh.bin"
            run("bvh", p, out)
            b = out.read_bytes()
            nn, npr = np.frombuffer(b, "<u8", 2)
            nodes = np.frombuffer(b, crt.NODE_DTYPE, int(nn), 16)
            order = np.frombuffer(b, "<u4", int(npr), 16 + 64 * int(nn))
            np.savez_compressed(GOLD / f"bvh_{name}.npz", bounds=nodes["bounds"], index=nodes["index"],
                                count=nodes["count"], axis=nodes["axis"], order=order)
        # per-sample-seeded renders
        for case, name, seed, ov, base, crop in RENDER_CASES:
            p, d = scene_file(tmp, name, seed, ov)
            out = tmp / "r.npy"
            args = ["render", p, base, out] + (list(crop) if crop else [])
            run(*args)
            rgb = np.load(out)
            np.savez_compressed(GOLD / f"render_{case}.npz", rgb=rgb)
            meta["renders"][case] = {"scene": name, "seed": seed, "camera": ov, "base_seed": base,
                                     "crop": crop, "shape": list(rgb.shape)}
        for case, name, seed, ov, base, crop in SAMPLE_CASES:
            p, d = scene_file(tmp, name, seed, ov)
            out = tmp / "s.npy"
            run("samples", p, base, out, *crop)
            smp = np.load(out)
            np.savez_compressed(GOLD / f"samples_{case}.npz", samples=smp)
            meta["renders"][case] = {"scene": name, "seed": seed, "camera": ov, "base_seed": base,
                                     "crop": crop, "shape": list(smp.shape), "per_sample": True}
        # closest-hit KATs: random rays from points around the scene toward its contents
        rng = np.random.default_rng(1234)
        for name, seed, n in HIT_SCENES:
            p, d = scene_file(tmp, name, seed, {})
            cam = crt.resolve_camera(d.camera)
            o = np.array(cam.origin[:]) + rng.normal(0, 0.5, (n, 3))
            tgt = np.array(cam.pixel00[:]) + rng.uniform(0, 1, (n, 1)) * np.array(cam.pixel_delta_x[:]) * d.camera.image_w \
                + rng.uniform(0, 1, (n, 1)) * np.array(cam.pixel_delta_y[:]) * d.camera.image_h
            rays = np.concatenate([o, tgt - o], axis=1)
            # a quarter of the rays start on the ground / at scene points and point anywhere
            k = n // 4
            rays[:k, 3:] = rng.normal(0, 1, (k, 3))
            rays_path = tmp / "rays.bin"
            rays_path.write_bytes(rays.astype("<f8").tobytes())
            out = tmp / "h.npy"
            run("hits", p, rays_path, out)
            np.savez_compressed(GOLD / f"hits_{name}.npz", rays=rays, hits=np.load(out))
        gen_linear(tmp, meta)
        gen_ppm(tmp)
        gen_bvh_ties(tmp)
        gen_radiance(tmp)
        gen_edge_rays(tmp, meta)
    (GOLD / "golden.json").write_text(json.dumps(meta, indent=1, sort_keys=True))
    print("golden fixtures written to", GOLD)


if __name__ == "__main__":
    if sys.argv[1:] in (["linear"], ["edge_rays"]):  # only the linear-world renders / the edge rays, merged into golden.json
        subprocess.run(["make", "-C", str(ROOT / "oracle"), "ref"], check=True)
        m = json.loads((GOLD / "golden.json").read_text())
        with tempfile.TemporaryDirectory() as td:
            {"linear": gen_linear, "edge_rays": gen_edge_rays}[sys.argv[1]](Path(td), m)
        (GOLD / "golden.json").write_text(json.dumps(m, indent=1, sort_keys=True))
    elif sys.argv[1:] in (["ppm"], ["ties"], ["radiance"]):  # only the PPM-value / tie-BVH / radiance fixtures
        subprocess.run(["make", "-C", str(ROOT / "oracle"), "ref"], check=True)
        with tempfile.TemporaryDirectory() as td:
            {"ppm": gen_ppm, "ties": gen_bvh_ties, "radiance": gen_radiance}[sys.argv[1]](Path(td))
    else:
        main()
