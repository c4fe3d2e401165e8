"""The mask algebra of the hand-scheduled speculative link step (crt_device.hip link_spec_steps:
exec is the mask of the lanes still in the loop, `nop` the lanes still walking to a first leaf)
against a plain per-lane restatement of the C++ step it replaces (walk<SPEC, LINK>'s `rec`, `park`
and vsel_top_on on `on`). Every lane state of the transition table above the block is enumerated,
and random 64-lane waves, partial ones included, walk random trees through their miss links with
both forms, step by step, the f64 hand-back included. The invariants that make the block's loop
end are asserted on the way: nop is a subset of exec, a lane at the sentinel always gets `rm`, and
the trip count is the old form's. CPU only; the GPU tests run the kernel itself."""
import itertools
import random

import pytest

ALL = (1 << 64) - 1


# ---- the C++ step, one lane at a time ------------------------------------------------------------
def old_lane_step(in_loop, rec, pref, cur, enter, leaf, near, link):
    """walk<SPEC, LINK, G2 = true>'s loop body for one lane: returns (in_loop', rec', pref', cur')."""
    if not in_loop:
        return False, rec, pref, cur
    reached = enter and leaf
    park = reached and rec
    if reached and not rec:  # pref = vsel(rm & nop, cur, pref)
        pref = cur
    rec = rec or reached
    if not park:  # vsel_top_on on `on` = exec & ~pm
        cur = near if (enter and not leaf) else link
    return not park, rec, pref, cur


# ---- the block's step, on lane masks -------------------------------------------------------------
def new_mask_step(exec_, nop, em, lm):
    """The block's scalar algebra. em / lm: the v_cmp results (bits of exec only).
    Returns (exec', nop', first, im, rm): pref <- cur on `first`, then cur <- im ? near : link on
    exec'."""
    assert em & ~exec_ == 0 and lm & ~exec_ == 0
    rm = em & lm
    im = em & ~rm
    first = rm & nop
    park = rm & ~nop
    nop2 = nop & ~rm
    exec2 = exec_ & ~park
    return exec2, nop2, first, im, rm


ROWS = {  # (nop, enter, leaf) of a lane in the loop -> (in loop', nop', pref', cur'): the table above the block
    (0, 0, 0): (1, 0, "pref", "link"), (1, 0, 0): (1, 1, "pref", "link"),
    (0, 0, 1): (1, 0, "pref", "link"), (1, 0, 1): (1, 1, "pref", "link"),
    (0, 1, 0): (1, 0, "pref", "near"), (1, 1, 0): (1, 1, "pref", "near"),
    (1, 1, 1): (1, 0, "cur", "link"),
    (0, 1, 1): (0, 0, "pref", "cur"),
}


def test_every_lane_state_follows_the_table_in_both_forms():
    vals = {"pref": 11, "cur": 22, "near": 33, "link": 44}
    seen = 0
    for in_loop, nop, enter, leaf in itertools.product([0, 1], repeat=4):
        if nop and not in_loop:
            continue  # nop is a subset of exec
        old = old_lane_step(bool(in_loop), not nop, vals["pref"], vals["cur"], bool(enter), bool(leaf),
                            vals["near"], vals["link"])
        # the same lane as bit 5 of a wave whose other lanes are outside the call
        bit = 1 << 5
        exec2, nop2, first, im, rm = new_mask_step(bit * in_loop, bit * nop, bit * (enter & in_loop), bit * (leaf & in_loop))
        pref = vals["cur"] if first & bit else vals["pref"]
        cur = (vals["near"] if im & bit else vals["link"]) if exec2 & bit else vals["cur"]
        new = (bool(exec2 & bit), not (nop2 & bit), pref, cur)
        if in_loop:
            assert new == old, (in_loop, nop, enter, leaf)
            row = ROWS[(nop, enter, leaf)]
            assert (int(new[0]), int(bool(nop2 & bit)), new[2], new[3]) == (row[0], row[1], vals[row[2]], vals[row[3]])
            seen += 1
        else:  # not in exec: nothing is written, and `rec` has no meaning
            assert (new[0], new[2], new[3]) == (False, vals["pref"], vals["cur"]) and nop2 == 0
            assert old == (False, True, vals["pref"], vals["cur"])
    assert seen == 8


# ---- random waves on random trees ----------------------------------------------------------------
def make_tree(rng, n_leaves):
    """Nodes: {'leaf', 'ch' (left, right), 'parent'}; node 0 is the root, the last one the sentinel."""
    nodes = [{"leaf": n_leaves == 1, "ch": None, "parent": None}]
    leaves = [0]
    while len(leaves) < n_leaves:
        i = leaves.pop(rng.randrange(len(leaves)))
        a, b = len(nodes), len(nodes) + 1
        nodes[i].update(leaf=False, ch=(a, b))
        nodes += [{"leaf": True, "ch": None, "parent": i}, {"leaf": True, "ch": None, "parent": i}]
        leaves += [a, b]
    nodes.append({"leaf": True, "ch": None, "parent": None})  # the sentinel
    return nodes


def links_of(nodes, swap):
    """near child and miss link of every node for one traversal order (swap[i]: right child first)."""
    sent = len(nodes) - 1
    near, link = [None] * len(nodes), [sent] * len(nodes)
    link[sent] = sent
    order = [0]
    for i in order:
        if nodes[i]["ch"]:
            a, b = nodes[i]["ch"]
            n, f = (b, a) if swap[i] else (a, b)
            near[i], link[n], link[f] = n, f, link[i]
            order += [a, b]
    return near, link


def run_wave(seed):
    rng = random.Random(seed)
    nodes = make_tree(rng, rng.randint(1, 40))
    sent = len(nodes) - 1
    orders = [links_of(nodes, [rng.random() < 0.5 for _ in nodes]) for _ in range(8)]  # the octants
    lane_oct = [rng.randrange(8) for _ in range(64)]
    # a lane enters a node with a probability, and a child only where it enters the parent
    p_enter = rng.choice([0.3, 0.6, 0.9])
    hit = [[False] * len(nodes) for _ in range(64)]
    for l in range(64):
        for i, n in enumerate(nodes[:-1]):
            up = True if n["parent"] is None else hit[l][n["parent"]]
            hit[l][i] = up and rng.random() < p_enter
        hit[l][sent] = True
    cur = [0] * 64
    done = 0
    call = rng.choice([ALL, rng.getrandbits(64) | 1, 1, (1 << 15) - 1])  # full and partial waves
    steps = rounds = 0
    while call & ~done:
        mask = call & ~done
        rounds += 1
        # --- old form: per-lane state, the wave's loop ends when no lane walks to a first leaf
        o_in = [bool(mask >> l & 1) for l in range(64)]
        o_rec, o_pref, o_cur = [False] * 64, [None] * 64, list(cur)
        # --- new form
        exec_, nop, n_pref, n_cur = mask, mask, [None] * 64, list(cur)
        trips_old = trips_new = 0
        while True:
            lanes = [l for l in range(64) if exec_ >> l & 1]
            assert nop & ~exec_ == 0 and exec_ != 0  # the loop's test never runs on an empty exec
            assert [l for l in range(64) if o_in[l]] == lanes
            enter = {l: hit[l][n_cur[l]] for l in lanes}
            # the f64 hand-back: some lanes undecided; the block leaves with in = exec and dec = 0
            # there, the gap's sign on the loop's other lanes, 1 outside; C++ fills in the zeros
            und = [l for l in lanes if rng.random() < 0.05]
            if und:
                dec = [1.0] * 64
                for l in lanes:
                    dec[l] = 0.0 if l in und else (0.5 if enter[l] else -0.5)
                slow = [l for l in range(64) if mask >> l & 1 and dec[l] == 0.0]
                assert slow == und  # the f64 test runs on the loop's undecided lanes alone
                for l in slow:
                    dec[l] = 1.0 if enter[l] else -1.0
                enter = {l: dec[l] > 0 for l in lanes}  # re-entered with exec = in
                assert enter == {l: hit[l][n_cur[l]] for l in lanes}
            em = sum(1 << l for l in lanes if enter[l])
            lm = sum(1 << l for l in lanes if nodes[n_cur[l]]["leaf"])
            sm = sum(1 << l for l in lanes if n_cur[l] == sent)
            exec2, nop2, first, im, rm = new_mask_step(exec_, nop, em, lm)
            assert sm & ~rm == 0  # a lane at the sentinel always gets rm
            for l in lanes:
                near, link = orders[lane_oct[l]]
                if first >> l & 1:
                    n_pref[l] = n_cur[l]
                nxt_near, nxt_link = near[n_cur[l]], link[n_cur[l]]
                o_in[l], o_rec[l], o_pref[l], o_cur[l] = old_lane_step(
                    True, o_rec[l], o_pref[l], o_cur[l], enter[l], nodes[o_cur[l]]["leaf"], nxt_near, nxt_link)
                if exec2 >> l & 1:
                    n_cur[l] = nxt_near if im >> l & 1 else nxt_link
            exec_, nop = exec2, nop2
            trips_new += 1
            trips_old += 1
            assert n_cur == o_cur and n_pref == o_pref
            for l in range(64):
                if mask >> l & 1:
                    assert o_rec[l] == (not nop >> l & 1)  # `rec` is the complement of nop
            # the old loop: `if (park) break` per lane, then `if (nop == 0) break` for the wave
            old_running = any(o_in) and any(o_in[l] and not o_rec[l] for l in range(64))
            new_running = nop != 0
            assert old_running == new_running
            if not new_running:
                break
        assert trips_old == trips_new
        steps += trips_new
        for l in range(64):
            if mask >> l & 1:
                assert n_pref[l] is not None  # every lane leaves with a node recorded
                if n_pref[l] == sent:
                    done |= 1 << l
        cur = n_cur
        assert rounds < 10000
    return steps


@pytest.mark.parametrize("seeds", [range(0, 60), range(1000, 1060)])
def test_random_waves_walk_alike_in_both_forms(seeds):
    steps = sum(run_wave(s) for s in seeds)
    assert steps > 300
