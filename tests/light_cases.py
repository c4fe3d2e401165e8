"""Scenes, ray sets and event tables shared by the tests of light sampling (tests/test_light_nee_model.py,
tests/test_gpu_light_nee.py). Not a test module.

The five worlds whose tables are checked: cornell (one parallelogram light), rtow_final_lights (20 emissive
spheres) and plan_worlds' cloud 300 (spheres, hollow ones among them), mixed 278 (spheres and
parallelograms) and flat 40 (axis-aligned parallelograms and Boxes); every fifth object of a plan world
is a light.

`mirror_rays` builds the paths the probe sets do not hold: from just outside a light sphere straight at
the centre of a near Metal or Dielectric sphere, so that the reflection comes back to the light: a light
hit with pb = none after a specular bounce.

EVENTS says which of the estimator's events a scene can show at all: cornell has one light, a
parallelogram, and no Metal or Dielectric, so no sample of it is hidden by another light or lies on a
sphere's far side and no light is hit after a specular bounce; christmas_tree's two lights never line up
with a Lambertian surface in these sets.
"""
import numpy as np

import light_nee_model as lm
import plan_worlds as pw
import probe_sets as ps

WORLDS = ["cornell", "rtow_final_lights", "cloud-300", "mixed-278", "flat-40"]
ALL_EVENTS = ("kept", "hidden_other", "hidden_light", "far_side", "hits_weighted", "after_specular")
EVENTS = {
    "cornell": ("kept", "hidden_other", "hits_weighted"),
    "rtow_final_lights": ALL_EVENTS,
    "christmas_tree": ("kept", "hidden_other", "far_side", "hits_weighted", "after_specular"),
}


def world(crt, name):
    """(SceneData, GpuScene keywords) of one of WORLDS or a probe_sets scene."""
    if "-" in name:
        family, n = name.split("-")
        return pw.world(crt, family, int(n))
    return ps.scene_data(crt, name), {}


def mirror_rays(d, per_light=3):
    objs, mats = d.objects, d.materials
    mk = mats["kind"][objs["material"]]
    sph = objs["kind"] == 1
    lights, spec = np.flatnonzero(sph & (mk == 4)), np.flatnonzero(sph & ((mk == 2) | (mk == 3)))
    rays = []
    for l in lights:
        c, r = np.array(objs["v"][l, :3], np.float64), abs(float(objs["v"][l, 3]))
        dist = np.linalg.norm(objs["v"][spec, :3] - c, axis=1)
        for m in spec[np.argsort(dist, kind="stable")[:per_light]]:
            to = np.array(objs["v"][m, :3], np.float64) - c
            o = c + to / np.linalg.norm(to) * (r * 1.01)
            rays.append(np.concatenate([o, np.array(objs["v"][m, :3], np.float64) - o]))
    return np.array(rays, np.float64).reshape(-1, 6)


def query(crt, name, n_s=3072, n_v=1025):
    """(rays, states) of a scene: the first n_s of its S set, n_v of its V set (4097 by default) and its
    mirror rays, which come last."""
    d = ps.scene_data(crt, name)
    s, v = ps.probe(crt, name, "S"), ps.probe(crt, name, "V")
    m = mirror_rays(d)
    rays = np.concatenate([s.rays[:n_s], v.rays[:n_v], m])
    states = np.concatenate([s.states[:n_s], v.states[:n_v], ps.states(len(m), 5) if len(m) else np.zeros(0, np.uint32)])
    return np.ascontiguousarray(rays), np.ascontiguousarray(states)


def counts(tr):
    return {k: len(getattr(tr, k)) for k in ALL_EVENTS}


def odd_lights_world(crt, only_zero=False):
    """Lights of zero weight among ordinary ones: black, negative and NaN colours, a negative intensity;
    only_zero leaves out the two lights with a positive weight."""
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE
    colors = [[0.0, 0.0, 0.0], [-1.0, -2.0, -0.5], [np.nan, 1.0, 1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 0.5], [0.1, 0.2, 0.3]]
    params = [3.0, 2.0, 1.0, -4.0, 1.5, 7.0]
    keep = range(4) if only_zero else range(6)
    mats = np.zeros(len(keep) + 1, MATERIAL_DTYPE)
    mats["kind"][0], mats["color"][0] = 1, [0.5, 0.5, 0.5]
    for j, k in enumerate(keep):
        mats["kind"][j + 1], mats["color"][j + 1], mats["param"][j + 1] = 4, colors[k], params[k]
    objs = np.zeros(len(keep) + 1, OBJECT_DTYPE)
    objs["kind"][0], objs["material"][0] = 2, 0
    objs["v"][0, :9] = [-50.0, 0.0, -50.0, 100.0, 0.0, 0.0, 0.0, 0.0, 100.0]
    for j in range(len(keep)):
        objs["material"][j + 1] = j + 1
        if j % 2:
            objs["kind"][j + 1] = 2
            objs["v"][j + 1, :9] = [3.0 * j, 4.0, 0.0, 1.5, 0.0, 0.25, 0.0, 0.0, 2.0]
        else:
            objs["kind"][j + 1] = 1
            objs["v"][j + 1, :4] = [3.0 * j, 2.0, 1.0, 0.75 if j % 4 else -0.75]
    d = crt.SceneData.named("config1")
    d.materials, d.objects = mats, objs
    return d


def one_light_world(crt, kind):
    """A single light (SPHERE: radius 1.5 at (0, 5, 0); QUAD: x in [-1, 2], z in [-0.5, 1], y = 3) over nothing."""
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE
    mats = np.zeros(1, MATERIAL_DTYPE)
    mats["kind"], mats["color"], mats["param"] = 4, [[1.0, 0.9, 0.8]], 5.0
    objs = np.zeros(1, OBJECT_DTYPE)
    if kind == lm.SPHERE:
        objs["kind"] = 1
        objs["v"][0, :4] = [0.0, 5.0, 0.0, 1.5]
    else:
        objs["kind"] = 2
        objs["v"][0, :9] = [-1.0, 3.0, -0.5, 3.0, 0.0, 0.0, 0.0, 0.0, 1.5]
    d = crt.SceneData.named("config1")
    d.materials, d.objects = mats, objs
    return d
