"""Seeded rays and LCG states for the radiance-query tests on rays that no camera made
(crt_radiance_async): what tests/test_gpu_radiance_probes.py sends through both routes of the GPU
entry and holds to the oracle's ray_color (oracle/crt_oracle_py.py radiance), and what
tests/test_probe_sets.py checks, without a GPU, to be worth sending. Not a test module.

A query is a Probe: rays (n, 6), states (n,) uint32 and the call's t_min.

  S  surface probes, 4096 records: the origin is the oracle's hit point of a centre ray of ray_sets'
     set A, the primitives hit taken in turn and each one's hit points round and round (so that a
     ground plane does not crowd out the small objects: with the hit points in ray order only 2 % of
     christmas_tree's records were zero at depth 2), the direction is that hit's normal plus a
     seeded unit vector, so it points into the normal's hemisphere
  I  inside starts, 2048 records in equal parts over the material kinds of the scene's objects: the
     origin is a seeded point strictly inside a primitive of that material (sphere: centre +
     u 0.9 |r| with |u| < 1; Box: 5 % to 95 % of the way between its corners; a kind that only
     parallelograms carry: a point of the face moved by -1e-3 of its unit normal), the direction a
     seeded normal vector (behind a face: of the half that points at the face)
  V  volume, 8192 records: ray_sets.set_d (origins over and beyond the scene box, normal directions,
     5 % with a zero component)
  X  scaled: the first 2048 records of S, then the first 2048 of V, directions times 2^k, the call's
     t_min 1e-5 * 2^-k, one Probe per k of X_SCALES: guard_cases.HIT_SCALES' positive members, the
     recip_core range edge at 2^500 from above, and -45 and -100 (t_min = 1e-5 * 2^100 is inside the
     ABI's limit of 2^100; -249 and below would be refused)

States are seeded uint32s with 0, 1, 0x7FFFFFFF, 0x80000000 and 0xFFFFFFFF at four records each.

Parallelogram::hit_by misses when |dot(unit normal, d)| < 1e-9, an absolute cutoff: at k = -45 and
-100 every |d| is below it, so in cornell (parallelograms and Boxes only) every first segment of
those two X calls misses in the reference. tests/test_probe_sets.py asserts exactly that there and
the 5 % shares everywhere else.

Shares measured when the sets were chosen (background BG; tests/test_probe_sets.py prints them and
holds them to 0.01): MEASURED below. Every origin of S is a hit point of set A. Total internal
reflection is the first event of 199 records of rtow_final's I, 205 of big's, 103 of mixed's and 159
of rtow_final_lights'; every material kind of every scene is a back-face first hit of at least 263
records of I (mixed's Dielectric; cornell's light 1024, its Lambertian Boxes 547).
"""
import hashlib
from dataclasses import dataclass

import numpy as np

import ray_sets as rs
from oracle import crt_oracle_py as orc

SCENES = ["rtow_final", "cornell", "mixed", "christmas_tree", "big", "rtow_final_lights"]
X_SCALES = (45, -45, 249, 251, 501, -100)
N_S, N_I, N_V, N_X = 4096, 2048, 8192, 2048
BG = (0.35, 0.6, 1.25)  # three distinct channels, none of them a scene's own
SPECIAL_STATES = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
QUADS_ONLY = ("cornell",)  # no sphere: the 1e-9 cutoff empties the X calls with k < 0

# scene -> (S exactly zero at depth 2, S non-zero at depth 50, I back-face first hits, V first hits,
#           first hits of the X calls in X_SCALES' order)
MEASURED = {
    "rtow_final": (0.173, 1.0, 0.996, 0.329, (0.353, 0.353, 0.353, 0.353, 0.327, 0.353)),
    "cornell": (0.542, 0.999, 0.767, 0.443, (0.546, 0.0, 0.546, 0.546, 0.546, 0.0)),
    "mixed": (0.138, 0.996, 0.811, 0.176, (0.276, 0.15, 0.276, 0.276, 0.276, 0.15)),
    "christmas_tree": (0.112, 1.0, 1.0, 0.509, (0.511, 0.073, 0.511, 0.511, 0.511, 0.073)),
    "big": (0.262, 1.0, 0.996, 0.227, (0.326, 0.326, 0.326, 0.326, 0.326, 0.326)),
    "rtow_final_lights": (0.143, 1.0, 0.993, 0.917, (0.641, 0.641, 0.641, 0.641, 0.067, 0.641)),
}


@dataclass
class Probe:
    rays: np.ndarray
    states: np.ndarray
    t_min: float = 1e-5


def scene_data(crt, name):
    if name == "rtow_final_lights":
        return crt.SceneData.named(name)
    return rs.scene_data(crt, name)


def scene_digest(d):
    """tests/golden/gen_golden.py's scene_digest."""
    return hashlib.sha256(d.materials.tobytes() + d.objects.tobytes()).hexdigest()


def states(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for j, v in enumerate(SPECIAL_STATES):
        s[(np.arange(4) * (n // 4) + 5 * j + 1) % n] = v
    return s


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(1))[:, None]


def set_s(crt, d):
    a = rs.set_a(crt, d)
    h = rs.oracle(d, a)
    h = h[h["prim"] >= 0]
    prims, count = np.unique(h["prim"], return_counts=True)
    by_prim = np.argsort(h["prim"], kind="stable")
    start = np.searchsorted(h["prim"][by_prim], prims)
    j = np.arange(N_S)
    p = j % len(prims)  # the primitives hit in turn, each one's hit points round and round
    i = by_prim[start[p] + (j // len(prims)) % count[p]]
    rng = np.random.default_rng(31)
    return Probe(np.concatenate([h["point"][i], h["normal"][i] + unit_vectors(rng, N_S)], 1), states(N_S, 32))


def inside_points(d, rng, objs, n):
    """n seeded points inside (or, for parallelograms, just behind) the objects `objs`, in turn, and
    the unit normals of the faces they are behind (zero for the other points)."""
    out, behind = np.empty((n, 3)), np.zeros((n, 3))
    for j in range(n):
        o = d.objects[objs[j % len(objs)]]
        v = np.array(o["v"], np.float64)
        if o["kind"] == 1:
            u = rng.normal(size=3)
            u *= rng.random() ** (1 / 3) / np.sqrt((u * u).sum())
            out[j] = v[:3] + u * (0.9 * abs(v[3]))
        elif o["kind"] == 3:
            out[j] = v[:3] + rng.uniform(0.05, 0.95, 3) * (v[3:6] - v[:3])
        else:
            n_ = np.cross(v[3:6], v[6:9])
            a, b = rng.uniform(0.05, 0.95, 2)
            behind[j] = n_ / np.sqrt((n_ * n_).sum())
            out[j] = (v[:3] + a * v[3:6] + b * v[6:9]) - 1e-3 * behind[j]
    return out, behind


def set_i(d):
    rng = np.random.default_rng(41)
    kind_of = d.materials["kind"][d.objects["material"]]
    kinds = sorted(set(kind_of.tolist()))
    share = N_I // len(kinds)
    pts, nrm = [], []
    for j, k in enumerate(kinds):
        mine = np.flatnonzero(kind_of == k)
        solid = mine[d.objects["kind"][mine] != 2]  # spheres and Boxes where the kind has any
        pick = rng.permutation(solid if len(solid) else mine)
        a, b = inside_points(d, rng, pick, share if j + 1 < len(kinds) else N_I - share * (len(kinds) - 1))
        pts.append(a)
        nrm.append(b)
    o, behind = np.concatenate(pts), np.concatenate(nrm)
    dirs = rng.normal(size=(N_I, 3))
    dirs[(dirs * behind).sum(1) < 0] *= -1  # from behind a face towards it: its back is the first hit
    perm = rng.permutation(N_I)  # every prefix holds every kind
    return Probe(np.concatenate([o[perm], dirs[perm]], 1), states(N_I, 42))


def set_v(crt, d):
    return Probe(rs.set_d(crt, d, N_V).rays, states(N_V, 52))


def set_x(s, v):
    out = []
    rays = np.concatenate([s.rays[:N_X], v.rays[:N_X]])
    st = np.concatenate([s.states[:N_X], v.states[:N_X]])
    for k in X_SCALES:
        r = rays.copy()
        r[:, 3:] *= 2.0 ** k
        out.append(Probe(r, st, 1e-5 * 2.0 ** -k))
    return out


_WORLDS, _ORACLE = {}, {}


def world(crt, name):
    """(SceneData, {"S": Probe, "I": Probe, "V": Probe, "X": [Probe per k of X_SCALES]}), once."""
    if name not in _WORLDS:
        d = scene_data(crt, name)
        s, v = set_s(crt, d), set_v(crt, d)
        sets = {"S": s, "I": set_i(d), "V": v, "X": set_x(s, v)}
        for p in [s, sets["I"], v] + sets["X"]:
            p.rays.setflags(write=False)
            p.states.setflags(write=False)
        _WORLDS[name] = (d, sets)
    return _WORLDS[name]


def probe(crt, name, key):
    """key: "S", "I", "V", or ("X", k)."""
    sets = world(crt, name)[1]
    return sets["X"][X_SCALES.index(key[1])] if isinstance(key, tuple) else sets[key]


def oracle(crt, name, key, depth, t_min=None, bg=BG):
    """The oracle's radiance of a set at a depth and t_min (None: the Probe's own), computed once per
    (scene, set, depth, t_min, background) and left unchanged."""
    p = probe(crt, name, key)
    t_min = p.t_min if t_min is None else t_min
    k = (name, key, depth, t_min, tuple(bg))
    if k not in _ORACLE:
        _ORACLE[k] = orc.radiance(world(crt, name)[0], p.rays, p.states, depth, bg, t_min)
        _ORACLE[k].setflags(write=False)
    return _ORACLE[k]


def default_states(base, n):
    """The states of a call without any: the oracle's own oracle_sample_seed(base, i, 0)."""
    return np.array([orc.sample_seed(base, i, 0) for i in range(n)], np.uint32)


# ---- the fixtures of tests/golden/gen_golden.py: the reference's own ray_color on such rays --------
FIXTURE_SCENES = ["rtow_final", "cornell", "rtow_final_lights"]
FIXTURE_DEPTHS = (1, 3, 50)


def fixture_records(crt, name):
    """1024 records in four equal parts, S and I first, then V and X: X's quarter is the S and the V
    halves of the k = -45 and k = -100 calls, 64 records each (the reference's t_min is 1e-5, below
    which every root of the calls with k > 0 lies)."""
    _, sets = world(crt, name)
    parts = [sets[k] for k in "SIV"]
    rays = [p.rays[:256] for p in parts]
    st = [p.states[:256] for p in parts]
    for k in (-45, -100):
        x = sets["X"][X_SCALES.index(k)]
        for lo in (0, N_X):
            rays.append(x.rays[lo:lo + 64])
            st.append(x.states[lo:lo + 64])
    return np.concatenate(rays), np.concatenate(st)
