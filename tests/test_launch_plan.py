"""The launch plans of the render, trace and radiance kernels (crt_launch_plan: the layout steps and the
launchers' own additions, run on the host) over tests/plan_worlds.py's families, one object at a time
from 1 to past the last capacity edge, on five routes (default, CRT_NO_LDS_SCENE, + CRT_FORCE_GSTACK,
+ CRT_NO_LDS_TOP, and CRT_NO_LDS_SCENE + CRT_NO_LDS_TOP). No GPU.

Every plan is held to the properties the kernels rely on: LDS regions aligned, disjoint, in order and
inside the request; the request inside the budget its class was admitted under; both guard levels of an
LDS stack past the data and at least three levels in; the treelet made of whole sibling pairs (or the
whole array, whose odd last node keeps readable LDS behind it); entry width and sentinel; classes that
only ever move away from LDS as a family grows; trace and radiance plans equal but for the camera copy.
The edges E1..E6 found on the way are printed (run with -s) and recorded in DESIGN.md."""
import pytest

import plan_worlds as pw

LDS_SCENE, LDS_STACK, HBM_STACK, ABSENT = pw.LDS_SCENE, pw.LDS_STACK, pw.HBM_STACK, pw.ABSENT
NODE = 32  # bytes of an f32 node: refs are byte offsets, siblings differ in bit 5
# documented figures (crt_device.hip): 160 KB of LDS a CU; LDS scenes at four blocks of 256 a
# CU get 40 KB, at five waves a SIMD 32 KB; an LDS stack at most 32 KB; HBM scenes 160 KB / 4 blocks
LDS_CAP = 65536
BUDGET_SCENE, BUDGET_FIVE, BUDGET_STACK, PER_BLOCK = 40 * 1024, 32 * 1024, 32 * 1024, 40 * 1024


def regions(p):
    """The plan's LDS regions [(name, offset, bytes)] in layout order."""
    out = []
    if p["klass"] == LDS_SCENE:
        for name in ("nodes", "refs", "spheres", "quads", "quadf", "sph64"):
            out.append((name, p["lds_" + name], p["bytes_" + name]))
    else:
        out.append(("treelet", 0, p["ntop"]))
        if p["klass"] == HBM_STACK and p["kernel"] == 1 and p["ntop"] % (2 * NODE):
            out.append(("sibling", p["ntop"], NODE))  # lds_tail: the sentinel's sibling slot
    if p["klass"] != HBM_STACK:
        out.append(("guards", p["lds_stack"] - 2 * p["level"], 2 * p["level"]))
        out.append(("stack", p["lds_stack"], p["stack_bytes"]))
    for name in ("cam", "acc", "inv64"):
        if p["lds_" + name] != ABSENT:
            out.append((name, p["lds_" + name], p["bytes_" + name]))
    return out


def check_plan(p, kernel, route_name, info, where):
    level, depth = p["level"], p["depth"]
    # entry width and sentinel: u16 exactly when every ref (a byte offset into the f32 nodes) fits 16 bits
    assert p["all_nodes"] == p["num_nodes"] * NODE, where
    assert p["sentinel"] == (p["num_nodes"] - 1) * NODE, where
    assert p["entry_bytes"] == (2 if p["all_nodes"] <= 65536 else 4), where
    assert (p["entry_bytes"] == 2) == (p["sentinel"] < 65536 and p["all_nodes"] - NODE < 65536), where
    assert level == p["block"] * p["entry_bytes"] and depth == info.depth, where
    assert p["stack_bytes"] >= (depth + 1) * level and p["stack_bytes"] % 16 == 0, where
    # the route's switches
    off = pw.ROUTES[route_name]
    if "CRT_NO_LDS_SCENE" in off:
        assert p["klass"] != LDS_SCENE, where
    if "CRT_FORCE_GSTACK" in off:
        assert p["klass"] == HBM_STACK, where
    if "CRT_NO_LDS_TOP" in off:
        assert p["ntop"] == 0, where
    # an LDS stack: within its budget, and it fits an HBM scene's block with the four levels below it,
    # the rays' 1 / d and the camera copy; an HBM stack that is not forced: one of the two fails
    beside = 4 * level + p["bytes_inv64"] + (p["bytes_cam"] if kernel != "trace" else 0)
    fits = p["stack_bytes"] <= BUDGET_STACK and beside + p["stack_bytes"] <= PER_BLOCK
    if p["klass"] == LDS_STACK:
        assert fits, where
    elif p["klass"] == HBM_STACK and "CRT_FORCE_GSTACK" not in off:
        assert not fits, where
    assert p["five_waves"] in (0, 1) and (not p["five_waves"] or (kernel == "render" and p["klass"] == LDS_SCENE)), where
    # regions: 16-byte aligned, in layout order, pairwise disjoint, inside [0, total); the last one ends the request
    reg = regions(p)
    end = 0
    for name, at, size in reg:
        assert at % 16 == 0, (where, name)
        assert at >= end, (where, name, "overlaps the region before it")
        end = at + size
    total = p["total_lds"]
    assert end <= total < end + 16, (where, reg, total)
    assert total <= LDS_CAP, where  # no kernel raises the dynamic LDS cap: a larger request is a launch error
    # class budgets
    if p["klass"] == LDS_SCENE:
        budget = BUDGET_FIVE if p["five_waves"] else BUDGET_SCENE
    else:
        budget = PER_BLOCK
    assert p["budget"] == budget, where
    over = total - budget  # test_class_budgets
    # stack guards
    if p["klass"] != HBM_STACK:
        data = p["lds_sph64"] + p["bytes_sph64"] if p["klass"] == LDS_SCENE else (p["ntop"] + 15) // 16 * 16
        assert p["lds_stack"] - 2 * level >= data, where  # the second guard level lies past the data
        assert p["lds_stack"] >= 4 * level, where          # at least three levels in (level -3 is read)
        assert p["lds_stack"] - 3 * level >= 0 and p["lds_stack"] + (depth + 1) * level <= p["lds_stack"] + p["stack_bytes"], where
        assert p["hbm_stack_levels"] == 0, where
    else:
        assert p["hbm_stack_levels"] >= depth + 1 + 3, where
    # the treelet
    if p["klass"] != LDS_SCENE:
        ntop = p["ntop"]
        assert ntop <= p["all_nodes"] and (ntop % (2 * NODE) == 0 or ntop == p["all_nodes"]), where
        # the sibling read at f ^ 32 of every token below ntop: inside the staged bytes when ntop is whole
        # pairs; a whole array of an odd node count ends with the sentinel alone, and the layout keeps
        # readable LDS behind it (the guard levels, the camera copy, or the slot lds_tail adds)
        if ntop % (2 * NODE):
            assert ntop == p["all_nodes"] and total >= ntop + NODE, (where, "the sentinel's sibling is past the request")
    else:
        assert p["ntop"] == 0, where
        assert p["lds_nodes"] == 0 and p["bytes_nodes"] >= p["all_nodes"], where
        # the sentinel's sibling lies in the regions behind the nodes (at least the guard levels)
        assert total >= p["all_nodes"] + NODE, where
    return over


def check_pair(t, r, where):
    """Trace and radiance plans are equal except for what the camera copy (`extra`) explains: the
    treelet and the totals, and, where the copy does not fit beside trace's layout, the f64 spheres
    left in HBM or the next class."""
    differ = {k for k in t if t[k] != r[k]} - {"kernel", "plain_route"}
    if t["klass"] != r["klass"] or t["bytes_sph64"] != r["bytes_sph64"]:
        assert r["klass"] >= t["klass"] and r["bytes_sph64"] <= t["bytes_sph64"], where
        assert t["total_lds"] + r["bytes_cam"] > t["budget"], (where, "the camera copy fits: nothing explains the difference")
        return
    assert differ <= {"ntop", "total_lds", "lds_cam", "lds_inv64", "lds_stack"}, (where, differ)
    assert t["klass"] == r["klass"] and r["ntop"] <= t["ntop"], where
    assert r["lds_cam"] != ABSENT and t["lds_cam"] == ABSENT, where
    if "lds_stack" in differ:  # only through the smaller treelet before it
        assert t["klass"] == LDS_STACK and t["ntop"] != r["ntop"], where
    assert r["total_lds"] - t["total_lds"] <= r["bytes_cam"] + 2 * NODE, where


_SWEEP = {}


def sweep(crt, family):
    """Every plan of the family checked, once a process: (its edges, the requests above their class's
    budget as (n, kernel, route, class, depth, total, budget))."""
    if family in _SWEEP:
        return _SWEEP[family]
    last, over = {}, []

    def visit(n, info, plans):
        for (kernel, rt), p in plans.items():
            where = f"{family} n={n} {kernel} {rt}"
            by = check_plan(p, kernel, rt, info, where)
            if by > 0:
                over.append((n, kernel, rt, p["klass"], p["depth"], p["total_lds"], p["budget"]))
            # class order: as the family grows the class never moves back towards LDS. The primitives
            # grow with n, but the builder's node count and depth do not always (cloud is an HBM scene at
            # n = 528 and an LDS scene again at n = 530), so "grows" is read off the sizes the decisions read: no scene
            # with as many primitives, nodes and levels as an earlier one has a class nearer to LDS.
            seen = last.setdefault((kernel, rt), {})
            for klass, sizes in seen.items():
                if klass > p["klass"]:
                    smaller = [s for s in sizes if s[0] <= p["num_nodes"] and s[1] <= p["depth"]]
                    assert not smaller, (where, f"class {p['klass']} after class {klass} at (nodes, depth) {smaller[0]}")
            mine = seen.setdefault(p["klass"], [])
            if not any(s[0] <= p["num_nodes"] and s[1] <= p["depth"] for s in mine):
                mine.append((p["num_nodes"], p["depth"]))
        for rt in pw.ROUTES:
            check_pair(plans["trace", rt], plans["radiance", rt], f"{family} n={n} {rt}")

    edges = pw.scan(crt, family, visit, routes=tuple(pw.ROUTES))
    pw._TABLE.setdefault(family, edges)
    _SWEEP[family] = (edges, over)
    return _SWEEP[family]


@pytest.mark.parametrize("family", pw.FAMILIES + pw.DEPTH_FAMILIES)
def test_plans_along_a_family(crt, family):
    sweep(crt, family)


def test_class_budgets(crt):
    """No request is above the budget its class was admitted under: 40 KB for an LDS scene at four
    waves, 32 KB at five, 160 KB / 4 blocks = 40 KB for an HBM scene.

    Every admission counts what the launcher keeps behind the layout (the camera copy, the rays' 1 / d,
    the levels below an LDS stack), so this holds at every size; DESIGN section 6i has the sizes at
    which it did not before the admissions counted them."""
    lines = []
    for family in pw.FAMILIES + pw.DEPTH_FAMILIES:
        over = sweep(crt, family)[1]
        cells = {}
        for n, kernel, rt, klass, depth, total, budget in over:
            c = cells.setdefault((kernel, rt, klass), [n, n, 0, 0])
            c[1], c[2], c[3] = n, c[2] + 1, max(c[3], total - budget)
        for (kernel, rt, klass), (lo, hi, count, worst) in sorted(cells.items()):
            lines.append(f"{family} {kernel} {rt} class {klass}: {count} sizes in n = {lo}..{hi}, up to {worst} bytes over")
    print("\n".join(lines))
    assert not lines, "\n" + "\n".join(lines)


def test_every_edge_is_found(crt):
    tables = {f: pw.table(crt, f) for f in pw.FAMILIES + pw.DEPTH_FAMILIES}
    print("\n" + pw.format_table(tables))
    for e, k, f in pw.rows():
        lo, hi, nodes_lo, nodes_hi, depth_lo, depth_hi = tables[f][e, k]
        assert hi == lo + 1
        assert pw.edge(crt, f, k, e) == (lo, hi)
    # E1 stands at 2048 nodes
    for f in pw.FAMILIES:
        for k in pw.KERNELS:
            assert tables[f]["E1", k][2] <= 2048 < tables[f]["E1", k][3]
    # E6: a stack leaves LDS above 32 KB, and an LDS stack beside a treelet also when it does not fit
    # 40 KB with the four levels below it, the rays' 1 / d (3 x 256 doubles) and, but for trace, the
    # 224-byte camera copy. chain (u16 entries, 512-byte levels) is small enough to be an LDS scene up to
    # the 32 KB: depth + 1 = 64 | 65 for every kernel. chain32 (u32, 1024-byte levels) is an HBM scene:
    # (40960 - 4096 - 6144) / 1024 = 30 levels for trace, 29 with the camera copy.
    for k in pw.KERNELS:
        assert tables["chain"]["E6", k][4:] == (63, 64)
        levels = min(BUDGET_STACK, PER_BLOCK - 4 * 1024 - 6144 - (0 if k == "trace" else 224)) // 1024
        assert levels == (30 if k == "trace" else 29)
        assert tables["chain32"]["E6", k][4:] == (levels - 1, levels)


def test_plan_arguments(crt):
    import ctypes as C
    _, s = pw.gpu_scene(crt, "cloud", 10)
    with pytest.raises(crt.CrtError):
        s.launch_plan(3)
    assert crt.lib().crt_launch_plan(None, 0, C.byref(crt._capi.LaunchPlan())) != 0
    p = s.launch_plan("trace")
    assert p.plain_route == 1 and list(p.reserved) == [0] * 9
    s.close()
