"""The stackless walk of the five-wave LDS-scene render instances (crt_device.hip walk(), LINK) as a
Python model, against the reference's DFS with a stack (bvh.h:617-712), and the library's miss-link
table (crt_walk_links.h: crt_walk_links, crt_walk_links_validate) against the model's.

A ray's DFS order is fixed by its octant (the near child is chosen by the sign of the direction on the
split axis alone), so the node a pop returns is a function of (node, octant): miss(root) = the
sentinel, miss(near child) = the far child, miss(far child) = miss(parent). Random trees in the device
node order (root, pad, sibling pairs, sentinel) with random split axes and a node test that is monotone
in t_max and in containment (a child is entered only where its parent is: the property the f32 / f64
node test has); for all eight octants the link machine must visit the stack walk's nodes, in the plain
form and in the speculative one (a lane records its first leaf, walks on, parks at the second and
tests it again next round; rounds the wave ends before the lane parks included). CPU only; the GPU
tests (tests/test_gpu_link_walk.py) run the kernels."""
import random

import numpy as np
import pytest

import cpp_raytracer_amd as crt

import plan_worlds

INF = float("inf")


# ---- trees in device order --------------------------------------------------------------------------
def make_tree(rng, depth, near, hit, max_depth=8, leaf_p=0.25):
    hit = hit and rng.random() < 0.85
    if depth >= max_depth or (depth > 0 and rng.random() < leaf_p):
        prims = [rng.uniform(near, near + 10) if rng.random() < 0.6 else None for _ in range(rng.randint(1, 3))]
        return {"leaf": True, "near": near, "hit": hit, "prims": prims}
    ch = [make_tree(rng, depth + 1, near + rng.choice([0.0, rng.uniform(0, 3)]), hit, max_depth, leaf_p) for _ in range(2)]
    return {"leaf": False, "near": near, "hit": hit, "ch": ch, "axis": rng.randrange(3)}


def chain(rng, n, side):
    """A degenerate tree: n interior nodes in a row, the subtree always on `side` (0, 1, or None: random)."""
    node = {"leaf": True, "near": 0.0, "hit": True, "prims": [rng.uniform(0, 10)]}
    for _ in range(n):
        other = {"leaf": True, "near": 0.0, "hit": rng.random() < 0.8, "prims": [rng.uniform(0, 10), None]}
        s = rng.randrange(2) if side is None else side
        node = {"leaf": False, "near": 0.0, "hit": True, "ch": [node, other] if s == 0 else [other, node], "axis": rng.randrange(3)}
    return node


def device_order(root):
    """The nodes as the device lists them: the root at 0, an unused pad at 1, then sibling pairs
    breadth-first (the left child at an even index), the sentinel last. Returns (nodes, left) with
    left[i] = index of node i's left child (its right child is left[i] + 1), None for leaves."""
    nodes, left = [root, None], {}
    q = 0
    while q < len(nodes):
        n = nodes[q]
        if n is not None and not n["leaf"]:
            left[q] = len(nodes)
            nodes.extend(n["ch"])
        q += 1
    sentinel = {"leaf": True, "near": -INF, "hit": True, "prims": [], "sentinel": True}
    nodes.append(sentinel)
    return nodes, left


def model_links(nodes, left):
    """miss[i][o] by the recursive definition, top-down."""
    s = len(nodes) - 1
    miss = [[s] * 8 for _ in nodes]

    def down(i):
        if i not in left:
            return
        l, r = left[i], left[i] + 1
        for o in range(8):
            near, far = (r, l) if (o >> nodes[i]["axis"]) & 1 else (l, r)
            miss[near][o] = far
            miss[far][o] = miss[i][o]
        down(l)
        down(r)
    down(0)
    return miss


def enter(n, tmax):
    return n["hit"] and n["near"] < tmax


def shrink(n, tmax):
    for t in n["prims"]:
        if t is not None and t < tmax:
            tmax = t
    return tmax


def children(nodes, left, i, o):
    l, r = left[i], left[i] + 1
    return (r, l) if (o >> nodes[i]["axis"]) & 1 else (l, r)


# ---- the reference and the two state machines, plain ---------------------------------------------
def reference(nodes, left, o):
    """BVH::hit_by: pop, test at the current t_max, a leaf's primitives shrink t_max, near child first.
    Returns (nodes tested in order, [(leaf, t_max at its primitive tests)])."""
    visits, log, tmax, stack = [], [], INF, [0]
    while stack:
        i = stack.pop()
        visits.append(i)
        if not enter(nodes[i], tmax):
            continue
        if i in left:
            near, far = children(nodes, left, i, o)
            stack.append(far)
            stack.append(near)
        else:
            log.append((i, tmax))
            tmax = shrink(nodes[i], tmax)
    return visits, log


def link_plain(nodes, left, miss, o):
    """walk() LINK, plain form, with leaf_step: cur = (enter && interior) ? near : miss[cur][o]; an
    entered leaf continues at its own miss link after its primitives; the end is the sentinel."""
    s = len(nodes) - 1
    visits, log, tmax, cur = [], [], INF, 0
    for _ in range(4 * len(nodes) + 4):
        if cur == s:
            return visits, log
        visits.append(cur)
        e = enter(nodes[cur], tmax)
        if e and cur in left:
            cur = children(nodes, left, cur, o)[0]
            continue
        if e:
            log.append((cur, tmax))
            tmax = shrink(nodes[cur], tmax)
        cur = miss[cur][o]
    raise AssertionError("the link walk did not end")


# ---- the speculative form: the stack walk with its guard levels, and the link walk ----------------
def spec_walk(nodes, left, miss, o, stop, use_links):
    """One lane of walk() SPEC + leaf_step over rounds. The lane records its first entered leaf (or
    the sentinel) in `pref`, walks on with the t_max of now and parks at the next entered leaf or the
    sentinel without moving; the wave's loop may end before that (stop). Sentinel tests are logged as
    visits too. use_links: pops come from the table, else from a stack above two guard levels."""
    s = len(nodes) - 1
    visits, log, tmax, cur = [], [], INF, 0
    stack = [s, s]  # the two guard levels
    for _ in range(4 * len(nodes) + 8):
        pref, run = None, True
        for _ in range(8 * len(nodes) + 16):
            if pref is not None and (not run or stop.random() < 0.3):
                break  # every lane of the wave has a leaf recorded: the loop ends
            visits.append(cur)
            e = enter(nodes[cur], tmax)
            inner = e and cur in left
            reached = e and not inner
            top = miss[cur][o] if use_links else (stack[-1] if stack else None)
            park = reached and pref is not None
            if reached and pref is None:
                pref = cur
            if park:
                run = False  # stays at the node: tested again next round
                continue
            if inner:
                near, far = children(nodes, left, cur, o)
                if not use_links:
                    stack.append(far)
                cur = near
            else:
                if not use_links:
                    stack.pop()
                cur = top
        else:
            raise AssertionError("the speculative round did not end")
        if pref == s:
            return visits, log
        log.append((pref, tmax))
        tmax = shrink(nodes[pref], tmax)
        if cur == s and (use_links or len(stack) < 2):  # leaf_step: R.cur == sentinel / R.sp < 0
            return visits, log
    raise AssertionError("the speculative walk did not end")


def check_tree(root, stop_seed):
    nodes, left = device_order(root)
    miss = model_links(nodes, left)
    total = 0
    for o in range(8):
        want_visits, want_log = reference(nodes, left, o)
        assert link_plain(nodes, left, miss, o) == (want_visits, want_log)
        a = spec_walk(nodes, left, miss, o, random.Random(stop_seed), use_links=False)
        b = spec_walk(nodes, left, miss, o, random.Random(stop_seed), use_links=True)
        assert a == b  # the same nodes, re-tests included
        assert b[1] == want_log  # the reference's leaves at the reference's t_max
        assert set(want_visits) <= set(b[0])  # speculation only adds node visits
        total += len(want_visits)
    return total


@pytest.mark.parametrize("seed", range(4))
def test_link_walk_visits_the_stack_walks_nodes(seed):
    rng = random.Random(seed)
    total = 0
    for k in range(2500):
        total += check_tree(make_tree(rng, 0, 0.0, True), 1000 * seed + k)
    assert total > 100000


def test_link_walk_on_the_smallest_and_on_degenerate_trees():
    rng = random.Random(77)
    leaf = {"leaf": True, "near": 0.0, "hit": True, "prims": [1.0, None]}
    check_tree(leaf, 1)  # the root is a leaf
    check_tree(dict(leaf, hit=False), 2)  # ... that the ray misses
    two = {"leaf": False, "near": 0.0, "hit": True, "axis": 1,
           "ch": [dict(leaf, prims=[3.0]), dict(leaf, prims=[2.0], near=1.0)]}
    check_tree(two, 3)  # one interior node
    for side in (0, 1, None):
        for n in (1, 2, 7, 40):
            check_tree(chain(rng, n, side), n)


# ---- the library's table ---------------------------------------------------------------------------
def library_tree(scene):
    """The scene's device-order tree from its exported preorder BVH (crt_host.cpp stage(): breadth-first
    for trees this small; an interior node's left child follows it in preorder, `index` is its right
    child), as (axis per device node, left)."""
    pre, _ = scene.export_bvh()
    nn = len(pre)

    def interior(i):
        return pre[i]["count"] == 0 and not (pre[i]["flags"] & 1) and i + 1 < nn
    assert nn < 1024
    bfs, q = [0], 0
    while q < len(bfs):
        i = bfs[q]
        if interior(i):
            bfs += [i + 1, int(pre[i]["index"])]
        q += 1
    pos = {p: (0 if k == 0 else k + 1) for k, p in enumerate(bfs)}
    n_dev = nn + 2  # the pad and the sentinel
    nodes = [{"axis": 0} for _ in range(n_dev)]
    left = {}
    for p in bfs:
        if interior(p):
            left[pos[p]] = pos[p + 1]
            assert pos[int(pre[p]["index"])] == pos[p + 1] + 1
            nodes[pos[p]]["axis"] = int(pre[p]["axis"])
    return nodes, left


def small_world(n, **kw):
    d, _ = plan_worlds.world(crt, "cloud", n)
    return crt.GpuScene(d, **kw)


SCENES = {
    "rtow_final": lambda: crt.GpuScene(crt.SceneData.named("rtow_final", 42)),
    "cornell": lambda: crt.GpuScene(crt.SceneData.named("cornell")),
    "cloud1": lambda: small_world(1),
    "cloud2_one_interior": lambda: small_world(2, max_prims_in_node=1),
    "cloud40": lambda: small_world(40, max_prims_in_node=1),
}


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene_and_table(request):
    s = SCENES[request.param]()
    t = s.walk_links()
    yield request.param, s, t
    s.close()


def test_library_table_is_the_models(scene_and_table):
    name, s, t = scene_and_table
    assert t is not None and t.dtype == np.uint16 and t.shape[1] == 8
    nodes, left = library_tree(s)
    assert t.shape[0] == len(nodes) == s.launch_plan("render").num_nodes
    want = np.array(model_links(nodes, left), np.uint32) * 32
    assert np.array_equal(t, want)
    if name == "cloud1":
        assert not left  # the root is a leaf
    if name == "cloud2_one_interior":
        assert list(left) == [0]


def test_library_table_terminates_and_validates(scene_and_table):
    _, s, t = scene_and_table
    n = len(t)
    sentinel = 32 * (n - 1)
    assert np.all(t % 32 == 0) and np.all(t[n - 1] == sentinel)
    for o in range(8):
        for i in range(n):
            cur, steps = 32 * i, 0
            while cur != sentinel:
                cur = int(t[cur // 32, o])
                steps += 1
                assert steps <= n
    assert s.walk_links_valid(t)


def test_a_corrupted_table_fails_validation(scene_and_table):
    """Every single-entry corruption the validator must catch: a link to the node itself (an endless
    loop), to an earlier node, to a later but wrong node, to the sentinel too early, a misaligned or
    out-of-range reference, and a sentinel that does not link to itself. Host function only."""
    name, s, t = scene_and_table
    n = len(t)
    rng = np.random.default_rng(5)
    reachable = [i for i in range(n - 1) if i != 1]
    tried = 0
    for _ in range(40):
        i, o = int(rng.choice(reachable)), int(rng.integers(8))
        for bad in (32 * i, 0, 32 * int(rng.integers(n)), 32 * (n - 1), int(t[i, o]) + 2, 32 * n):
            if bad == t[i, o] or bad > 0xFFFF:
                continue
            c = t.copy()
            c[i, o] = bad
            assert not s.walk_links_valid(c), (name, i, o, bad)
            tried += 1
    c = t.copy()
    c[n - 1, 3] = 0
    assert not s.walk_links_valid(c)
    assert tried > 40
    with pytest.raises(crt.CrtError):
        s.walk_links_valid(t[:-1])


def test_a_tree_beyond_u16_references_has_no_table():
    d, kw = plan_worlds.world(crt, "chain32", 1)  # more than 2048 nodes
    s = crt.GpuScene(d, **kw)
    try:
        assert s.launch_plan("render").entry_bytes == 4
        assert s.walk_links() is None
        assert s.last_walk() == "none"
    finally:
        s.close()
