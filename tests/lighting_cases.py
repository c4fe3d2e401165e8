"""Scenes, maps, lightings and ray sets shared by the tests of the lit estimator (tests/test_lighting_model.py
on the CPU, tests/test_gpu_lighting*.py on the GPU). Not a test module.

Scenes: rtow_final_lights and cornell (LDS scenes) and christmas_tree (an HBM scene). cornell's probe sets
start on its surfaces and in the volume about it, and its front is open, so its paths leave through the
front and see the map from the outside of the box.

Maps: env_truth.random_map (n = 8) and a sun map (n = 8, one texel of the +Y face at env_truth.SUN over
0.5), each under both filters. A lighting is (how the environment is used, map, filter):

  sampled-random-bilinear   sampled-sun-nearest   plain-random-nearest   plain-sun-bilinear

every one of them together with the scene's light sampler. FIRST holds the two that run at every depth;
the other two run at depth 50.

`query` is light_cases.query cut to QUERY records of the S set, QUERY of the V set and the mirror rays
(light hits after a specular bounce); christmas_tree keeps the whole set. EVENTS says which of the lit estimator's events a scene can show
under a sampled map; under a plain map the four map events and the weighted escapes cannot occur, and a
bounce has the light's ray or none.
"""
import numpy as np

import env_model as em
import env_nee_model as enm
import env_truth as et
import light_cases as lc
import light_nee_model as lm
import lighting_model as lg
import probe_sets as ps

SCENES = ["rtow_final_lights", "cornell", "christmas_tree"]
BG = (0.35, 0.6, 1.25)  # three distinct channels, none of them a scene's own
T_MIN = 1e-5
QUERY = 640
SUN_AT = (2 * 8 + 3, 5)  # the +Y face, row 3, column 5: above every scene

LIGHTINGS = {
    "sampled-random-bilinear": (True, "random", em.BILINEAR),
    "sampled-sun-nearest": (True, "sun", em.NEAREST),
    "plain-random-nearest": (False, "random", em.NEAREST),
    "plain-sun-bilinear": (False, "sun", em.BILINEAR),
}
FIRST = ["sampled-random-bilinear", "plain-random-nearest"]

MAP_EVENTS = ("map_kept", "map_occluded", "map_skipped", "escapes_weighted", "both", "map_only")
# what a scene cannot show: cornell has one light, a parallelogram, and neither Metal nor Dielectric;
# christmas_tree's two lights never hide one another in these sets
MISSING = {
    "rtow_final_lights": (),
    "cornell": ("light_hidden_light",),
    "christmas_tree": ("light_hidden_light",),
}


def events(name, sampled):
    out = [e for e in lg.EVENTS if e not in MISSING[name]]
    return [e for e in out if sampled or e not in MAP_EVENTS]


def texels(which):
    return et.random_map(8) if which == "random" else et.sun_map(8, *SUN_AT)


def model_env(label):
    _, which, filt = LIGHTINGS[label]
    return em.make(texels(which), filter=filt)


def lighting(d, label):
    """The model's Lighting of a scene under LIGHTINGS[label], with the scene's lights."""
    menv = model_env(label)
    return lg.Lighting(menv, enm.tables(menv) if LIGHTINGS[label][0] else None, lm.tables(d))


def query(crt, name):
    """christmas_tree keeps light_cases' whole set: under a plain map its one weighted light hit lies past
    the first 2048 records of either set."""
    if name == "christmas_tree":
        return big_query(crt, name)
    return lc.query(crt, name, QUERY, QUERY)


def big_query(crt, name):
    """4097 records and the mirror rays: the capacity test's."""
    return lc.query(crt, name, 3072, 1025)


_MODEL = {}


def model(crt, orc, name, label, depth, key="query", rays=None, states=None):
    """(rgb, ended, Trace) of the model for a scene's query (or the rays given, under `key`) under a
    lighting at a depth, computed once a process and left unchanged."""
    k = (name, label, depth, key)
    if k not in _MODEL:
        d = ps.scene_data(crt, name)
        if rays is None:
            rays, states = query(crt, name)
        rgb, ended, tr = lg.ray_color(orc, d, rays, states, depth, BG, T_MIN, lighting(d, label), crt=crt)
        rgb.setflags(write=False)
        ended.setflags(write=False)
        _MODEL[k] = (rgb, ended, tr)
    return _MODEL[k]


def missing_events(name, label, tr):
    seen = lg.counts(tr)
    return [e for e in events(name, LIGHTINGS[label][0]) if seen[e] == 0]


# ---- the adaptive scenario under a lighting: lens_pass_model's frames and passes, cornell ----------------
# Under SCEN_LIGHTING no block is free of noise (the panorama's background is the random map), so the
# thresholds are not lens_pass_model's. From the blocks' ratios sum se / sum m on the model's radiance of the
# lens model's rays (tests/test_lighting_passes_model.py prints them): equirect, 9 blocks: the last has
# 0.0098 after 8 samples; block 7 has 0.0155 after 16 and 0.0138 after 24, block 6 0.0158 after 32 and
# 0.0141 after 40; blocks 0 to 5 never less than 0.0165: 0.0147 stops one block at the first pass, two
# later, six never. cube, 8 blocks: blocks 6 and 7 have 0.0591 and 0.0797 after 8; block 4 has 0.0930 after
# 16 and 0.0719 after 24, block 0 0.0911 after 24 and 0.0815 after 32; blocks 3 and 5 never less than
# 0.1018: 0.084.
SCEN_LIGHTING = "sampled-random-bilinear"
SCEN_THRESHOLD = {"equirect": 0.0147, "cube": 0.084}


# ---- the instance rows: env_cases.ROWS' worlds, every fifth object a light ------------------------------
def row_lighting(d, sampled):
    """The lighting of an instance row: the random map under BILINEAR, sampled or plain, and the world's lights."""
    menv = em.make(et.random_map(8), filter=em.BILINEAR)
    return lg.Lighting(menv, enm.tables(menv) if sampled else None, lm.tables(d))
