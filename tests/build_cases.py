"""The scenes, the case table and a numpy reading of a tree for the GPU scene set-up's edge tests:
the binned-SAH build of crt_bvh_gpu.hip switches algorithm at kBigTask = kChunk = 4096 primitives
(eight per-chunk / per-task kernels with the serial sah_decide above, one wave of build_level with
sah_parallel up to it), runs its small tasks kBatch = 8 levels per host round trip over a grid of
CUs x 8 resident blocks, and crt_stage_gpu.hip orders the nodes below a breadth-first top of
kTopBfs = 1024 and scans object and slot counts in tiles of 2048. Each case here puts a task, a
partition point, a level count, a node count or a scan length on a known side of one of these.
tests/test_build_cases.py checks, without a GPU and from the host tree alone, that each case is where
it claims to be; tests/test_gpu_build_edges.py builds them on the GPU. Not a test module.

The host Builder (crt_host.cpp) is the specification: tests/test_host_abi.py pins it to the
reference's BVH goldens. The GPU build is level-synchronous, so its task list is a function of the
tree: tree_tasks() reads it from an exported preorder node array."""
import sys

import numpy as np

from conftest import ROOT

K_BIG = 4096      # crt_bvh_gpu.hip kBigTask = kChunk
K_BATCH = 8       # levels per host round trip of the small phase
K_TOP = 1024      # crt_stage_gpu.hip kTopBfs
K_TILE = 2048     # crt_stage_gpu.hip kScanTile
RESIDENT = 2048   # CUs x 8 blocks of the batched levels on 256 CUs


# ---- scenes ----------------------------------------------------------------------------------------
def object_scene(crt, objs):
    """A scene of the given objects (OBJECT_DTYPE; materials 0..2 may be named) and config1's camera."""
    from cpp_raytracer_amd import MATERIAL_DTYPE, OBJECT_DTYPE
    d = crt.SceneData.named("config1")
    mats = np.zeros(3, MATERIAL_DTYPE)
    mats["kind"] = [1, 2, 4]  # Lambertian, Metal, light
    mats["color"] = [[0.7, 0.4, 0.3], [0.8, 0.8, 0.9], [1.0, 0.9, 0.8]]
    mats["param"] = [0.0, 0.1, 2.0]
    d.materials, d.objects = mats, np.ascontiguousarray(objs, dtype=OBJECT_DTYPE)
    return d


def sphere_scene(crt, centres, radii):
    """Spheres at `centres` (n, 3) with `radii` (scalar or (n,)), in this order."""
    from cpp_raytracer_amd import CRT_SPHERE, OBJECT_DTYPE
    centres = np.asarray(centres, np.float64)
    objs = np.zeros(len(centres), OBJECT_DTYPE)
    objs["kind"] = CRT_SPHERE
    objs["material"] = np.arange(len(centres)) % 3
    objs["v"][:, :3] = centres
    objs["v"][:, 3] = radii
    return object_scene(crt, objs)


def mixed_objects(seed, kinds):
    """Objects of the given kinds (1 sphere, 2 parallelogram, 3 Box) in [-20, 20]^3, in this order:
    gen_golden.tie_scene's way of filling v, without its grid and signed zeros."""
    from cpp_raytracer_amd import CRT_BOX, CRT_SPHERE, OBJECT_DTYPE
    rng = np.random.default_rng(seed)
    kinds = np.asarray(kinds, np.uint32)
    n = len(kinds)
    objs = np.zeros(n, OBJECT_DTYPE)
    objs["kind"] = kinds
    objs["material"] = rng.integers(0, 3, n)
    v = rng.uniform(-1.5, 1.5, (n, 9))
    v[:, :3] = rng.uniform(-20, 20, (n, 3))
    v[kinds == CRT_SPHERE, 3] = np.abs(v[kinds == CRT_SPHERE, 3]) + 0.1
    box = kinds == CRT_BOX
    v[box, 3:6] = v[box, 0:3] + np.abs(v[box, 3:6]) + 0.2
    objs["v"] = v
    return objs


def tie_scene(seed, n):
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    from gen_golden import tie_scene as make
    return make(seed, n)


def cloud(crt, n, seed=1, half=10.0, r=0.05, scale=1.0):
    rng = np.random.default_rng(seed)
    return sphere_scene(crt, rng.uniform(-half, half, (n, 3)) * scale, r)


def clusters(crt, a, b, order):
    """a spheres in [-1, 1]^3 and b spheres 1000 further on x, r = 0.01: `sorted` (the a first: the
    root's partition finds nothing to swap, m = 0), `reversed` (the b first) or a seeded shuffle."""
    rng = np.random.default_rng(100 + a % 7 + b % 5)
    ca = rng.uniform(-1, 1, (a, 3))
    cb = rng.uniform(-1, 1, (b, 3)) + [1000.0, 0.0, 0.0]
    c = np.concatenate([ca, cb] if order != "reversed" else [cb, ca])
    if order == "shuffle":
        c = c[np.random.default_rng(5).permutation(a + b)]
    return sphere_scene(crt, c, 0.01)


def chain(crt, n, e0, extra=None):
    """Sphere i at x = 2^(e0 + i), r = 2^(e0 + i - 2): with two buckets and leaf size 1 every split
    takes the spheres of the lower half of the centroid extent from the last one or few."""
    i = np.arange(n, dtype=np.float64)
    c = np.zeros((n, 3))
    c[:, 0] = 2.0 ** (e0 + i)
    r = 2.0 ** (e0 + i - 2)
    if extra is not None:
        c, r = np.concatenate([extra[0], c]), np.concatenate([extra[1], r])
    return sphere_scene(crt, c, r)


# ---- a tree's tasks ----------------------------------------------------------------------------------
def tree_tasks(nodes):
    """Per preorder node of an exported tree: level (the root's is 0), [lo, hi) in `order`, mid (the
    right child's lo; -1 for a leaf) and leaf. A node is inner when its count is 0 and it is not the
    last node (crt_stage_gpu.hip's `interior`); its children are the next node and nodes[i].index.
    The level-synchronous GPU build has exactly these tasks at these levels."""
    n = len(nodes)
    index, count = nodes["index"].astype(np.int64), nodes["count"].astype(np.int64)
    leaf = ~((count == 0) & (np.arange(n) + 1 < n))
    level = np.zeros(n, np.int64)
    lo, hi, mid = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for i in range(n):  # parents come before their children
        if not leaf[i]:
            level[i + 1] = level[index[i]] = level[i] + 1
    for i in range(n - 1, -1, -1):  # children come after their parents
        if leaf[i]:
            lo[i], hi[i] = index[i], index[i] + count[i]
        else:
            lo[i], mid[i], hi[i] = lo[i + 1], lo[index[i]], hi[index[i]]
            assert hi[i + 1] == lo[index[i]], i  # siblings share mid
    return {"level": level, "lo": lo, "hi": hi, "mid": mid, "leaf": leaf}


def facts(nodes):
    """What the build's switches see of a tree; every entry is derived from tree_tasks alone.
    - n, nodes, depth (levels);
    - tasks, big, small: per level, the number of tasks, of tasks above K_BIG primitives and of the
      others; last_big: the last level with a big task (-1: none);
    - big_levels: big[: last_big + 1]; small_levels: the levels after last_big (the batched small phase);
    - big_leaves: sizes of the leaves above K_BIG primitives; max_leaf;
    - big_children: (left size, right size) of every big inner task, in preorder;
    - root_split, root_mid_mod = (mid - lo) mod K_BIG of the root, last_chunk of the root;
    - mid_mods: (mid - lo) mod K_BIG of every big inner task, in preorder;
    - lines: the (level, big, small) of the build's per-level lines and the counts of its batched
      lines, which come K_BATCH at a time (zeros after the tree ends)."""
    t = tree_tasks(nodes)
    size = t["hi"] - t["lo"]
    depth = int(t["level"].max()) + 1
    is_big = size > K_BIG
    big = np.bincount(t["level"][is_big], minlength=depth)
    tasks = np.bincount(t["level"], minlength=depth)
    last_big = int(np.flatnonzero(big).max()) if big.any() else -1
    inner_big = np.flatnonzero(is_big & ~t["leaf"])
    f = {"n": int(size[0]), "nodes": len(nodes), "depth": depth,
         "tasks": tasks.tolist(), "big": big.tolist(), "small": (tasks - big).tolist(),
         "last_big": last_big, "big_levels": big[:last_big + 1].tolist(),
         "small_levels": depth - 1 - last_big,
         "big_leaves": sorted(size[is_big & t["leaf"]].tolist()),
         "max_leaf": int(size[t["leaf"]].max()),
         "big_children": [(int(t["mid"][i] - t["lo"][i]), int(t["hi"][i] - t["mid"][i])) for i in inner_big],
         "mid_mods": [int((t["mid"][i] - t["lo"][i]) % K_BIG) for i in inner_big],
         "root_split": None if t["leaf"][0] else (int(t["mid"][0]), int(size[0] - t["mid"][0])),
         "root_mid_mod": None if t["leaf"][0] else int(t["mid"][0] % K_BIG),
         "last_chunk": int((size[0] - 1) % K_BIG + 1)}
    f["max_tasks"] = int(tasks.max())
    batched = (tasks - big)[last_big + 1:].tolist()
    batched += [0] * (-len(batched) % K_BATCH)
    f["lines"] = ([(L, int(big[L]), int(tasks[L] - big[L])) for L in range(last_big + 1)], batched)
    return f


# ---- the case table ------------------------------------------------------------------------------------
class Case:
    """make(crt) -> SceneData; kw: the build parameters; claims: entries of facts() the host tree must
    show (test_build_cases.py), a callable value being a predicate; hits: a (d) case of its family."""
    def __init__(self, family, name, make, kw=None, hits=False, **claims):
        self.family, self.id, self.make, self.kw = family, f"{family}-{name}", make, dict(kw or {})
        self.hits, self.claims = hits, claims

    def __repr__(self):
        return self.id


CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


def _wide(v):
    return v > RESIDENT


# Uniform clouds in [-10, 10]^3, r = 0.05, at the default leaf size and at leaf size 1: 4095 and 4096
# are one small task, 4097 is a big one whose last chunk holds one primitive, 8192 is two whole
# chunks, 8193 two and one primitive. Leaf size 1 at 8192 has levels of more tasks than resident blocks.
for _n, _big, _last in ((4095, [], 4095), (4096, [], 4096), (4097, [1], 1), (8192, [1, 1], 4096), (8193, [1, 1], 1)):
    for _ml in (12, 1):
        _c = dict(n=_n, big_levels=_big, last_chunk=_last, big_leaves=[], max_leaf=_ml)
        if _ml == 1:
            _c["nodes"] = 2 * _n - 1
        if _n >= 8192 and _ml == 1:
            _c["max_tasks"] = _wide
        _add("cloud", f"{_n}-leaf{_ml}", lambda crt, n=_n: cloud(crt, n), {"max_prims_in_node": _ml},
             hits=(_n, _ml) == (4097, 1), **_c)

# Two clusters: the root splits at exactly a in every input order; (mid - lo) mod 4096 = 0 for
# a = 4096 and 8192 (no chunk straddles mid) and 1 for their neighbours; a 4097-child is a big task
# again, a 4096-child a small one.
for _a, _b, _big in ((4096, 4096, [1]), (4096, 4097, [1, 1]), (4097, 4096, [1, 1]), (1, 4097, [1, 1]),
                     (4097, 1, [1, 1]), (4096, 1, [1]), (8192, 4097, [1, 2, 1])):
    for _o in ("sorted", "reversed", "shuffle"):
        _add("clusters", f"{_a}-{_b}-{_o}", lambda crt, a=_a, b=_b, o=_o: clusters(crt, a, b, o),
             hits=(_a, _b, _o) == (4096, 4097, "shuffle"),
             n=_a + _b, root_split=(_a, _b), root_mid_mod=_a % K_BIG, big_levels=_big, big_leaves=[],
             max_tasks=_wide)


def _coincident(crt, far):
    c = np.tile([1.0, 2.0, 3.0], (5000 + far, 1))
    if far:
        c[-1] = [500.0, 2.0, 3.0]
    return sphere_scene(crt, c, 0.5)


def _line(crt):
    c = np.zeros((6000, 3))
    c[:, 2] = np.random.default_rng(3).uniform(-50, 50, 6000)
    return sphere_scene(crt, c, 0.05)


# Big tasks that end as leaves: no live centroid axis; every SAH cost infinite; count <= max_leaf and
# min_cost >= count. And their neighbours: one live axis only, the cost rule one primitive over.
_add("bigleaf", "coincident-5000", lambda crt: _coincident(crt, 0),
     n=5000, nodes=1, big_levels=[1], big_leaves=[5000], small_levels=0)
_add("bigleaf", "coincident-5000-and-1", lambda crt: _coincident(crt, 1),
     n=5001, nodes=3, root_split=(5000, 1), big_levels=[1, 1], big_leaves=[5000], small_levels=0)
_add("bigleaf", "overflow-5000", lambda crt: cloud(crt, 5000, seed=2, scale=1e160, r=1e150),
     n=5000, nodes=1, big_levels=[1], big_leaves=[5000], small_levels=0)
_add("bigleaf", "cost-9000-leaf6000", lambda crt: cloud(crt, 9000, seed=2, half=0.01, r=10.0),
     {"max_prims_in_node": 6000},
     n=9000, nodes=3, root_split=(3130, 5870), big_levels=[1, 1], big_leaves=[5870], small_levels=0)
_add("bigleaf", "cost-4097-leaf4097", lambda crt: cloud(crt, 4097, seed=1, half=0.01, r=10.0),
     {"max_prims_in_node": 4097}, n=4097, nodes=1, big_levels=[1], big_leaves=[4097], last_chunk=1)
_add("bigleaf", "cost-4097-leaf4096", lambda crt: cloud(crt, 4097, seed=1, half=0.01, r=10.0),
     {"max_prims_in_node": 4096}, n=4097, nodes=3, root_split=(3569, 528), big_levels=[1], big_leaves=[],
     small_levels=1)
_add("bigleaf", "line-6000", _line, hits=True, n=6000, big_levels=[1], big_leaves=[], max_leaf=1)

# sah_decide (the big path's serial sweep) at the ends of the bucket range
for _nb, _big in ((2, [1, 2]), (3, [1, 1]), (63, [1, 2]), (64, [1, 2])):
    _add("buckets", f"{_nb}", lambda crt: cloud(crt, 9000, seed=4), {"num_buckets": _nb, "max_prims_in_node": 4},
         hits=_nb == 3, n=9000, big_levels=_big, big_leaves=[], max_leaf=lambda v: v <= 4)

# Chains: depth = n for n = 2 .. 18 (every residue of the 8-level batch, its exact ends 8 and 16 and
# the 9 and 17 after them); deep paths below the breadth-first top; small levels after big ones.
for _n in range(2, 19):
    _add("chain", f"{_n}", lambda crt, n=_n: chain(crt, n, 0), {"num_buckets": 2, "max_prims_in_node": 1},
         hits=_n == 17, n=_n, depth=_n, nodes=2 * _n - 1, small_levels=_n, big_levels=[])
for _n, _depth in ((600, 327), (900, 477)):
    _add("chain", f"{_n}", lambda crt, n=_n: chain(crt, n, -400), {"num_buckets": 2, "max_prims_in_node": 1},
         n=_n, depth=_depth, nodes=2 * _n - 1, big_levels=[], small_levels=_depth)


def _cloud_and_chain(crt):
    rng = np.random.default_rng(6)
    return chain(crt, 12, 0, (rng.uniform(-1, 1, (5000, 3)) * 2.0 ** -60, np.full(5000, 2.0 ** -64)))


_add("chain", "cloud-5000-and-12", _cloud_and_chain, {"num_buckets": 2, "max_prims_in_node": 1},
     n=5012, depth=23, root_split=(5010, 2), big_levels=[1] * 7, small_levels=16, big_leaves=[])

# Node counts around the breadth-first top (a tree's node count is odd): all in the top, exactly the
# top, two nodes below it
for _n in (511, 512, 513, 514):
    _add("nodes", f"{_n}", lambda crt, n=_n: cloud(crt, n, seed=7), {"max_prims_in_node": 1},
         hits=_n == 513, n=_n, nodes=2 * _n - 1, big_levels=[])


def _scan(crt, n, other):
    k = np.random.default_rng(n).choice([1, other], n, p=[0.7, 0.3] if other == 3 else [0.6, 0.4])
    k[-1] = 3 if other == 3 else 1  # the last object is of the counted kind
    return object_scene(crt, mixed_objects(n, k))


# Scan tiles: Boxes among spheres (the per-object offset scan over the objects, the slot-rank scan
# over the primitives), spheres and parallelograms (the slot-rank scan alone) around 2048 and 4096
for _n in (2047, 2048, 2049, 4096, 4097):
    _add("scan", f"boxes-{_n}", lambda crt, n=_n: _scan(crt, n, 3), hits=_n == 2049, objects=_n, n=lambda v: v > 4800)
for _n in (2047, 2048, 2049):
    _add("scan", f"quads-{_n}", lambda crt, n=_n: _scan(crt, n, 2), hits=_n == 2049, objects=_n, n=_n, big_levels=[])

# Ties (equal bounds and centroids, signed zeros) at the task edges
for _n, _big in ((4096, [1, 1]), (4097, [1]), (8193, [1, 1, 1, 1])):
    _add("ties", f"{_n}", lambda crt, n=_n: tie_scene(9, n), hits=_n == 4097, objects=_n, big_levels=_big)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
FAMILIES = ("cloud", "clusters", "bigleaf", "buckets", "chain", "nodes", "scan", "ties")
_host = {}


def host_tree(crt, case):
    """(scene data, facts, nodes, order) of a case's host build, computed once. facts gains `objects`."""
    if case.id not in _host:
        d = case.make(crt)
        s = crt.GpuScene(d, **case.kw)
        nodes, order = s.export_bvh()
        i = s.info()
        s.close()
        f = facts(nodes)
        f["objects"] = len(d.objects)
        assert (f["n"], f["nodes"], f["depth"], f["max_leaf"]) == (i.num_primitives, i.num_nodes, i.depth, i.max_leaf_size)
        _host[case.id] = d, f, nodes, order
    return _host[case.id]
