"""The worlds, the case table and the numpy helpers of the range-guard tests: every fast path of the
render kernel sits behind a range guard (crt_device.hip sqrt_from_rsq, recip_exact, recip_a / div_a,
leaf_ray32_ok, trav_init; crt_quad_filter.h quad_ray32_ok, quad_record, quad_flat_box; crt_internal.h
kF32BoundMax, kF32SphereMax), and each case here puts a frame's rays or a scene's records on a known
side of one of them. tests/test_guard_cases.py checks, without a GPU, that each case is where it
claims to be; tests/test_gpu_range_guards.py renders them. Not a test module.

One unit layout (a [-4, 4]^3 cluster 12 units down -z from the camera, no ground sphere) times
S = 2^s, exactly; focus_dist F = 2^e sets the primary directions' size (d = pixel - origin, |d| in
[F, 1.1 F]). The camera looks down -z with up = +y, so its basis is the coordinate axes exactly and
d_z = -F for every centre ray."""
import numpy as np

FAMILIES = ("spheres", "flat", "rotated", "mixed")
W, H, SPP, DEPTH = 24, 16, 4, 8
FOV = float(np.deg2rad(40.0))  # vertical, in radians (Camera::init takes tan(fov / 2))
BACKGROUND = (0.55, 0.7, 0.95)
CAMS = {"origin": (0.0, 0.0, 0.0), "offset": (3.0, 2.0, 5.0), "far": (3.0, 2.0, 17.0)}
BASE_SEED = 7100


def unit_world(family):
    """(materials, objects) of the family's unit layout, the cluster centred at (0, 0, 0)."""
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE
    rng = np.random.default_rng(20 + FAMILIES.index(family))
    mats = np.zeros(5, MATERIAL_DTYPE)
    mats["kind"] = [1, 2, 2, 3, 4]  # Lambertian, mirror Metal, fuzzed Metal, Dielectric, light
    mats["color"] = [[0.8, 0.3, 0.2], [0.9, 0.9, 0.7], [0.6, 0.7, 0.9], [0.0, 0.0, 0.0], [1.0, 0.9, 0.8]]
    mats["param"] = [0.0, 0.0, 0.4, 1.5, 3.0]
    objs = []

    def obj(kind, v):
        o = np.zeros(1, OBJECT_DTYPE)[0]
        o["kind"], o["material"] = kind, len(objs) % 5
        o["v"][:len(v)] = v
        objs.append(o)

    n_sph = {"spheres": 38, "mixed": 14}.get(family, 0)
    for i in range(n_sph):
        r = rng.uniform(0.5, 1.3) * (-1 if i % 9 == 8 else 1)  # a few hollow ones
        obj(1, [*rng.uniform(-4, 4, 3), r])
    if family in ("flat", "mixed"):
        for _ in range(14 if family == "flat" else 4):  # axis-aligned parallelograms
            ax = rng.permutation(3)
            s1, s2 = np.zeros(3), np.zeros(3)
            s1[ax[0]] = rng.uniform(1.5, 4) * rng.choice([-1, 1])
            s2[ax[1]] = rng.uniform(1.5, 4) * rng.choice([-1, 1])
            v = rng.uniform(-4, 4, 3)
            obj(2, [*np.clip(v, -4 - np.minimum(s1 + s2, 0), 4 - np.maximum(s1 + s2, 0)), *s1, *s2])
        for _ in range(4 if family == "flat" else 2):  # boxes
            a = rng.uniform(-4, 1.5, 3)
            obj(3, [*a, *(a + rng.uniform(0.8, 2.5, 3))])
    if family in ("rotated", "mixed"):
        for _ in range(30 if family == "rotated" else 6):
            s1, s2 = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
            lo = -4 - np.minimum(0, np.minimum(np.minimum(s1, s2), s1 + s2))
            hi = 4 - np.maximum(0, np.maximum(np.maximum(s1, s2), s1 + s2))
            obj(2, [*np.clip(rng.uniform(-4, 4, 3), lo, np.maximum(lo, hi)), *s1, *s2])
    objs = np.array(objs, dtype=OBJECT_DTYPE)
    assert len(objs) <= 40 and set(objs["material"].tolist()) == {0, 1, 2, 3, 4}
    return mats, objs


def scene(crt, family, s=0, e=0, cam="origin", max_depth=DEPTH):
    """The family's world with the camera of CAMS[cam], everything times 2^s, focus_dist 2^e."""
    from cpp_raytracer_amd import camera_with
    from cpp_raytracer_amd._capi import D3
    mats, objs = unit_world(family)
    c = np.array(CAMS[cam])
    centre = c + np.array([0.0, 0.0, -12.0])
    S = 2.0 ** s
    v = objs["v"]
    for i, o in enumerate(objs):
        if o["kind"] == 1 or o["kind"] == 2:
            v[i, :3] += centre
        else:
            v[i, :6] += np.tile(centre, 2)
    v *= S  # exact: a power of two, nothing near the ends of the f64 range
    d = crt.SceneData.named("config1")
    d.materials, d.objects = mats, objs
    d.camera = camera_with(d.camera, image_w=W, image_h=H, samples_per_pixel=SPP, max_depth=max_depth,
                           center=D3(*(c * S)), lookat=D3(*(centre * S)), has_lookat=1, up=D3(0.0, 1.0, 0.0),
                           fov=FOV, fov_is_vertical=1, defocus_angle=0.0, focus_dist=2.0 ** e, has_focus_dist=1,
                           background=D3(*BACKGROUND))
    return d


# ---- the case table --------------------------------------------------------------------------------
# a claim is (guard of GUARDS, "in" | "out"[, the families it holds for]); side() decides it
class Case:
    def __init__(self, ladder, s, e, cam, claims=(), gstack=False, families=FAMILIES):
        self.ladder, self.s, self.e, self.cam, self.claims = ladder, s, e, cam, tuple(claims)
        self.gstack, self.families = gstack, tuple(families)
        self.id = f"{ladder}-s{s}-e{e}-{cam}"

    def claimed(self, family):
        """guard -> "in" | "out" for this family (a claim may name the families it holds for)."""
        return {c[0]: c[1] for c in self.claims if len(c) < 3 or family in c[2]}

    def __repr__(self):
        return self.id


QUADS = ("flat", "rotated", "mixed")
CASES = [
    # Ladder A: small directions, the camera at the exact origin (pixel - origin cancels otherwise)
    Case("A", 0, 0, "origin", gstack=True),
    Case("A", 0, -29, "origin", [("leaf_a_lo", "in"), ("quad_d_lo", "in")]),
    Case("A", 0, -31, "origin", [("leaf_a_lo", "out"), ("quad_d_lo", "out")]),
    Case("A", 0, -33, "origin", [("trav_d_lo", "in")]),
    Case("A", 0, -36, "origin"),  # rays on both sides of 2^-39
    Case("A", 0, -40, "origin", [("trav_d_lo", "out")]),
    Case("A", 0, -42, "origin", [("trav_d_lo", "out")]),
    Case("A", 0, -249, "origin", [("div_a_lo", "in")]),
    Case("A", 0, -251, "origin", [("div_a_lo", "out")]),
    Case("A", 0, -382, "origin", [("sqrt_lo", "in")]),
    Case("A", 0, -385, "origin", [("sqrt_lo", "out")]),
    Case("A", 0, -499, "origin", [("recip_lo", "in")]),
    Case("A", 0, -501, "origin", [("recip_lo", "out")]),
]
# Ladder B: large directions; primary t ~ 12 S / F stays above t_min = 1e-5
for cam in ("origin", "offset"):
    CASES += [
        Case("B", 12, 29, cam, [("leaf_a_hi", "in"), ("leaf_d_hi", "in")], gstack=cam == "offset"),
        Case("B", 12, 30, cam, [("leaf_a_hi", "out"), ("leaf_d_hi", "in")]),  # a alone: d_z = -2^30 is allowed
        Case("B", 12, 31, cam, [("leaf_a_hi", "out"), ("leaf_d_hi", "out")]),
        Case("B", 22, 38, cam, [("trav_d_hi", "in")]),
        Case("B", 24, 41, cam, [("trav_d_hi", "out")]),
        Case("B", 234, 249, cam, [("div_a_hi", "in")]),
        Case("B", 236, 251, cam, [("div_a_hi", "out")]),
    ]
# Ladder C: positions alone (F = 1). "offset": the scene passes each bound before the camera does;
# "far": the camera is further from the origin than any record, so |o_k| passes the bound alone.
CASES += [
    Case("C", 26, 0, "offset", [("rec_30", "in"), ("o_30", "in"), ("sn1_lo", "in")], gstack=True),
    Case("C", 27, 0, "offset", [("rec_30", "out"), ("o_30", "in")]),
    Case("C", 28, 0, "offset", [("rec_30", "out"), ("o_30", "out")]),
    Case("C", 25, 0, "far", [("rec_30", "in"), ("o_30", "in")]),
    Case("C", 26, 0, "far", [("rec_30", "in"), ("o_30", "out")]),
    Case("C", 36, 0, "offset", [("bound_40", "in"), ("o_40", "in"), ("sn1_lo", "out")]),
    Case("C", 37, 0, "offset", [("bound_40", "out"), ("o_40", "in")]),
    Case("C", 35, 0, "far", [("bound_40", "in"), ("o_40", "in")]),
    Case("C", 36, 0, "far", [("bound_40", "in"), ("o_40", "out")]),
    # tiny worlds for sn1 = |sn|_1 ~ S^-2 across 2^40; F = S keeps primary t ~ 12 above t_min
    Case("C", -19, -19, "offset", [("sn1_hi", "in")], families=QUADS),
    Case("C", -20, -20, "offset", [("sn1_hi", "in", ("flat", "mixed")), ("sn1_hi", "out", ("rotated",))], families=QUADS),
    Case("C", -21, -21, "offset", [("sn1_hi", "out")], families=QUADS),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# guard -> (bound, its sense: +1 = "inside is at or below the bound", -1 = "at or above")
GUARDS = {
    "leaf_a_lo": (2.0 ** -60, -1), "leaf_a_hi": (2.0 ** 60, +1), "leaf_d_hi": (2.0 ** 30, +1),
    "quad_d_lo": (2.0 ** -30, -1),
    "trav_d_lo": (2.0 ** -39, -1), "trav_d_hi": (2.0 ** 39, +1),
    "div_a_lo": (2.0 ** -500, -1), "div_a_hi": (2.0 ** 500, +1),
    "sqrt_lo": (2.0 ** -767, -1), "recip_lo": (2.0 ** -500, -1),
    "rec_30": (2.0 ** 30, +1), "o_30": (2.0 ** 30, +1), "bound_40": (2.0 ** 40, +1), "o_40": (2.0 ** 40, +1),
    "sn1_hi": (2.0 ** 40, +1), "sn1_lo": (2.0 ** -64, -1),
}


# ---- numpy restatements ----------------------------------------------------------------------------
def prims(d):
    """The flattened primitives of a SceneData in Scene::get_primitive_components order:
    (kind, object index, 15 doubles) with crt_prims.h's quad_prim / object_prim arithmetic."""
    out = []

    def quad(i, v, s1, s2):
        n = np.cross(s1, s2)
        m2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
        out.append((2, i, np.concatenate([v, s1, s2, n * (1 / np.sqrt(m2)), n * (1 / m2)])))

    for i, o in enumerate(d.objects):
        v = np.array(o["v"], np.float64)
        if o["kind"] == 1:
            out.append((1, i, np.concatenate([v[:4], np.zeros(11)])))
        elif o["kind"] == 2:
            quad(i, v[:3], v[3:6], v[6:9])
        else:
            mn, mx = np.minimum(v[:3], v[3:6]), np.maximum(v[:3], v[3:6])
            sx, sy, sz = (np.eye(3) * (mx - mn))
            for a, b, c in ((mn, sx, sy), (mn, sx, sz), (mn, sy, sz), (mx, -sx, -sy), (mx, -sx, -sz), (mx, -sy, -sz)):
                quad(i, a, b, c)
    return out


def log2(x):
    with np.errstate(divide="ignore"):
        return float(np.log2(x))


def measure(crt, d, hits=None):
    """The quantities the guards compare, from the centre rays of crt.resolve_camera's vectors
    (tests/denoise_model.py centre_rays) and the scene's records; with `hits` (the oracle's closest
    hits of the centre rays) the discriminants b^2 - a c of the spheres hit, as hit_sphere forms them."""
    import denoise_model as dm
    cam = crt.resolve_camera(d.camera, 0)
    rays = dm.centre_rays(cam).reshape(-1, 6)
    o, dd = rays[:, :3], rays[:, 3:]
    a = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
    ad = np.abs(dd)
    m = {"a_min": a.min(), "a_max": a.max(),
         "dmin_min": ad.min(1).min(), "dmin_max": ad.min(1).max(),  # min_k |d_k|: its range over the rays
         "dmax_min": ad.max(1).min(), "dmax_max": ad.max(1).max(),
         "o_max": np.abs(o).max()}
    P = prims(d)
    rec, corner, sn1 = [0.0], [0.0], []
    for kind, _, v in P:
        if kind == 1:
            rec.append(np.abs(v[:4]).max())
            corner.append(np.abs(v[:3]).max() + abs(v[3]))
        else:
            rec.append(np.abs(v[:9]).max())
            pts = [v[:3], v[:3] + v[3:6], v[:3] + v[6:9], v[:3] + v[3:6] + v[6:9]]
            corner.append(max(np.abs(p).max() for p in pts))
            sn1.append(np.abs(v[12:15]).sum())
    m["rec_max"], m["bound_max"] = max(rec), max(corner)
    m["sn1_min"], m["sn1_max"] = (min(sn1), max(sn1)) if sn1 else (np.nan, np.nan)
    if hits is not None:
        disc = []
        for i in np.flatnonzero(hits["prim"] >= 0):
            kind, _, v = P[int(hits["prim"][i])]
            if kind != 1:
                continue
            oc = o[i] - v[:3]
            b = dd[i, 0] * oc[0] + dd[i, 1] * oc[1] + dd[i, 2] * oc[2]
            c = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - v[3] * v[3]
            disc.append(b * b - a[i] * c)
        disc = np.array(disc) if disc else np.array([np.nan])
        m["disc_min"], m["disc_med"], m["disc_max"] = disc.min(), float(np.median(disc)), disc.max()
    return m


def side(guard, m):
    """("in" | "out" | "mixed", the deciding quantity) of a measured case at a guard. "in": every
    centre ray / record is within the guard; "out": every one (or, for the per-scene flags, at least
    one record) is beyond it."""
    bound, sense = GUARDS[guard]
    lo, hi = {
        "leaf_a_lo": ("a_min", "a_max"), "leaf_a_hi": ("a_min", "a_max"),
        "div_a_lo": ("a_min", "a_max"), "div_a_hi": ("a_min", "a_max"),
        "leaf_d_hi": ("dmax_min", "dmax_max"), "quad_d_lo": ("dmax_min", "dmax_max"),
        "trav_d_lo": ("dmin_min", "dmin_max"), "trav_d_hi": ("dmax_min", "dmax_max"),
        "sqrt_lo": ("disc_med", "disc_max"),   # in: most first hits; out: every first hit
        "recip_lo": ("a_min", "a_max"),        # on sqrt(a)
        # per-scene flags: one record beyond the bound turns the fast path off
        "rec_30": ("rec_max", "rec_max"), "bound_40": ("bound_max", "bound_max"),
        "o_30": ("o_max", "o_max"), "o_40": ("o_max", "o_max"),
        "sn1_hi": ("sn1_max", "sn1_max"), "sn1_lo": ("sn1_min", "sn1_min"),
    }[guard]
    lo, hi = m[lo], m[hi]
    if guard == "recip_lo":
        lo, hi = np.sqrt(lo), np.sqrt(hi)
    if sense > 0:
        return ("in", hi) if hi <= bound else ("out", lo) if lo > bound else ("mixed", hi)
    return ("in", lo) if lo >= bound else ("out", hi) if hi < bound else ("mixed", lo)


def quads_cut(case):
    """Parallelogram::hit_by misses when |dot(unit normal, d)| < 1e-9, an absolute cutoff: with every
    |d| below it (F <= 2^-31: |d| <= 1.1 F < 1e-9) no primary ray hits any parallelogram."""
    return case.ladder == "A" and case.e <= -31


def closest_hit_rays(family, n=4096):
    """n rays around the family's cluster (centred at the origin): random origins, N(0, 1)
    directions, 5 % of them with one component exactly zero."""
    rng = np.random.default_rng(900 + FAMILIES.index(family))
    o = rng.uniform(-6, 6, (n, 3)) + np.array([0.0, 0.0, -12.0])  # scene(cam="origin")
    d = rng.normal(size=(n, 3))
    z = rng.random(n) < 0.05
    d[z, rng.integers(0, 3, int(z.sum()))] = 0.0
    return np.concatenate([o, d], 1)


HIT_SCALES = (0, 249, -249, 251, -251, -385)  # directions times 2^k, t_min times 2^-k


def filter_expected(family, route, m):
    """Whether leaf_step's two-pass filter runs for the primary rays of a measured case
    (crt_device.hip device_render / leaf_step restated): True, False, or None when the centre rays
    lie on both sides of a per-ray guard. Sphere pairs: sphere-only scenes within kF32SphereMax, rays
    within leaf_ray32_ok. Parallelogram filters: parallelogram-only scenes within quad_record's
    range, in the LDS-scene kernels only; the flat-box one needs the f32 walk's node range and has no
    per-ray guard, the generic one has quad_ray32_ok. Mixed scenes: the plain loop."""
    def per_ray(conds):
        sides = {side(g, m)[0] for g in conds}
        return True if sides == {"in"} else False if "out" in sides else None

    if family == "spheres":
        if m["rec_max"] > 2.0 ** 30:
            return False
        return per_ray(("leaf_a_lo", "leaf_a_hi", "leaf_d_hi", "o_30"))
    if family == "mixed" or route != "lds":
        return False
    if m["rec_max"] > 2.0 ** 30 or m["sn1_max"] > 2.0 ** 40 or m["sn1_min"] < 2.0 ** -64:
        return False
    if family == "flat":
        return m["bound_max"] <= 2.0 ** 40
    return per_ray(("quad_d_lo", "leaf_d_hi", "o_30"))
