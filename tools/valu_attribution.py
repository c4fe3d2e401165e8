"""Per-phase VALU instruction attribution of one render-kernel instance.

Static opcode mix per basic block of a `hipcc -S` listing (blocks split at labels and after branches;
the loop each block belongs to from LLVM's "in Loop: Header=" comments), times the dynamic
frequency of each phase's loop body from the instrumented pass (bench.py's `instrumented_counts`:
wave iterations of the walk, of the leaf filter, of the candidates' exact tests, of shading).
The phase loops are found by their loop header and by content:
  walk      the loop (ds_read_b128 / global_load of nodes) with v_fma_f32 and v_min3_f32, without its
            f64 fallback sub-blocks: x wave_iters_walk; the fallback: x wave_iters_slow
  pass1     the loop with v_pk_fma_f32 (the packed sphere filter): x wave_iters_leaf / 2
  pass2     the loop with v_rsq_f64 and v_ffbh_u32 (hit_sphere on the next candidate): x wave_iters_candidates
  rest      everything else (shade, path start, traversal set-up, draws): SQ_INSTS_VALU minus the above
Classes: f64, f32 (arith and transcendental), pk_f32, int (add/sub/mul/mad/cvt/mbcnt), cmp/cndmask,
min/max/med3, bit/shift (and/or/xor/bfe/lshl/lshr/bitop3/perm), mov/lane (mov, readlane, writelane).
The SQ_INSTS_VALU_* hardware classes count f32 / f64 add, mul, fma, trans, INT32, INT64, CVT; the rest
(cmp/cndmask, min/max, bit ops, movs, packed f32) is the counters' unclassified "other".
Beside the VALU count, every phase's line ends with its issue slots per iteration: scalar ALU / branch
instructions, s_nop, s_waitcnt, and all instructions of any kind. A wave issues about one
instruction of any kind every four cycles, so with five waves a SIMD a loop is sized by its issue
slots as much as by its VALU.
A loop that an inline-asm statement owns (the speculative link step, link_spec_steps) is unknown to
LLVM: inside an asm statement blocks are also split at numeric local labels, and the blocks from a
label `N:` to a backward branch `Nb` are that loop's body. Where the walk's LLVM loop holds such a
body, the body alone is the "walk step" (x wave_iters_walk) and the statement's other blocks (entry,
exit, hand-back to the f64 test and re-entry) are listed as "walk block entry / hand-back", static
counts only: they run once per call or per f64 hand-back.
usage: python tools/valu_attribution.py listing.s kernel_substring bench.json [pmc.json]
(bench.json: the line of a `bench.py --full` run)"""
import collections
import json
import re
import sys

CLASSES = ["f64", "f32", "pk_f32", "int", "cmp/cndmask", "min/max", "bit/shift", "mov/lane"]


def cls(op):
    if not op.startswith("v_"):
        return None
    if "f64" in op:
        return "f64"
    if op.startswith("v_pk_"):
        return "pk_f32"
    if op.startswith(("v_cmp", "v_cndmask")):
        return "cmp/cndmask"
    if op.startswith(("v_min", "v_max", "v_med")):
        return "min/max"
    if op.startswith(("v_bfe", "v_lshl", "v_lshr", "v_ashr", "v_alignbit", "v_bfi", "v_perm", "v_bitop",
                      "v_and", "v_or", "v_xor", "v_not", "v_bfrev")):
        return "bit/shift"
    if op.startswith(("v_mov", "v_readlane", "v_writelane", "v_readfirstlane", "v_accvgpr", "v_swap")):
        return "mov/lane"
    if "f32" in op or "f16" in op:
        return "f32"
    return "int"


def blocks_of(path, name):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and name in l and ":" in l.split(";")[0])
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur, header, in_asm = [], None, None, False
    for l in lines[start + 1:end]:
        if "#ASMSTART" in l or "#ASMEND" in l:
            in_asm = "#ASMSTART" in l
            continue
        m = re.match(r"^(\d+):", l)
        if m and in_asm and cur is not None:  # a local label of an asm statement: a block of its own
            cur = {"label": cur["label"].split("@")[0].rstrip("+") + "@" + m.group(1), "loop": cur["loop"], "ins": [], "local": m.group(1)}
            blocks.append(cur)
            continue
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", l)
        if m:
            h = re.search(r"Header=(BB\d+_\d+)", m.group(2))
            header = h.group(1) if h else ("BB" + m.group(1)[4:] if "Loop Header" in m.group(2) or "Parent Loop" in m.group(2) else None)
            cur = {"label": m.group(1), "loop": header, "ins": []}
            blocks.append(cur)
            continue
        s = l.strip()
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        if cur is None:
            cur = {"label": "entry", "loop": None, "ins": []}
            blocks.append(cur)
        ins = s.split(";")[0].strip()
        cur["ins"].append(ins)
        if ins.startswith(("s_cbranch", "s_branch")):  # a new basic block after a branch
            back = re.fullmatch(r"(\d+)b", ins.split()[-1])
            # a conditional one: the blocks since that local label are the body of an asm-owned
            # loop (an unconditional `s_branch Nb` is a jump into it, the re-entry after a hand-back)
            if back and in_asm and ins.startswith("s_cbranch"):
                i = max(k for k, b in enumerate(blocks) if b.get("local") == back.group(1))
                for b in blocks[i:]:
                    b["asm_loop"] = True
            cur = {"label": cur["label"] + "+", "loop": cur["loop"], "ins": []}
            blocks.append(cur)
    return blocks


def slots(ins_list):
    """Issue slots of a list of instructions: (scalar ALU / branch, s_nop, s_waitcnt, all)."""
    ops = [x.split()[0] for x in ins_list]
    nop = sum(o == "s_nop" for o in ops)
    wait = sum(o.startswith("s_waitcnt") for o in ops)
    salu = sum(o.startswith("s_") for o in ops) - nop - wait
    return salu, nop, wait, len(ops)


def mix(ins_list):
    c = collections.Counter()
    for x in ins_list:
        k = cls(x.split()[0])
        if k:
            c[k] += 1
    return c


def main():
    path, name, bench = sys.argv[1], sys.argv[2], json.load(open(sys.argv[3]))
    pmc = json.load(open(sys.argv[4])) if len(sys.argv) > 4 else None
    cnt = bench["instrumented_counts"]["timed_walk"]
    blocks = blocks_of(path, name)
    loops = collections.defaultdict(list)
    for b in blocks:
        if b["loop"]:
            loops[b["loop"]].append(b)

    def has(bs, *ops):
        text = " ".join(x.split()[0] for b in bs for x in b["ins"])
        return all(o in text for o in ops)

    walk = next(bs for bs in loops.values() if has(bs, "v_fma_f32", "v_min3_f32") and not has(bs, "v_pk_fma_f32"))
    pass1 = next(bs for bs in loops.values() if has(bs, "v_pk_fma_f32"))
    pass2 = next(bs for bs in loops.values() if has(bs, "v_rsq_f64", "v_ffbh_u32"))  # 31 - clz(candidates)
    walk_main = [b for b in walk if not any("f64" in x.split()[0] for x in b["ins"])]
    walk_f64 = [b for b in walk if any("f64" in x.split()[0] for x in b["ins"])]
    walk_edge = []
    if any(b.get("asm_loop") for b in walk_main):  # the step is the asm statement's own loop
        walk_edge = [b for b in walk_main if not b.get("asm_loop")]
        walk_main = [b for b in walk_main if b.get("asm_loop")]
    # pass 2: every block of the loop, the root's divisions included (an upper bound: they run
    # where the discriminant admits a root in range, most candidates)
    pass2_main = pass2
    rows = [
        ("walk step", walk_main, cnt["wave_iters_walk"]),
        ("walk f64 fallback", walk_f64, cnt["wave_iters_slow"]),
        ("leaf pass 1 (pair)", pass1, cnt["wave_iters_leaf"] / 2),
        ("leaf pass 2 (candidate)", pass2_main, cnt["wave_iters_candidates"]),
    ]
    if walk_edge:
        rows.insert(1, ("walk block entry / hand-back", walk_edge, 0))
    out, total = [], collections.Counter()
    print(f"{'phase':28s} {'iters':>10s} {'VALU/it':>8s} " + " ".join(f"{c:>11s}" for c in CLASSES) + f" {'dynamic':>10s}"
          f" {'salu/br':>8s} {'s_nop':>6s} {'waitcnt':>8s} {'slots/it':>9s} {'dyn slots':>10s}")
    for label, bs, it in rows:
        ins = [x for b in bs for x in b["ins"]]
        m = mix(ins)
        n = sum(m.values())
        salu, nop, wait, allins = slots(ins)
        dyn = {c: m[c] * it for c in CLASSES}
        total.update(dyn)
        out.append({"phase": label, "wave_iterations": it, "valu_per_iteration": n, "per_iteration": dict(m),
                    "dynamic": dyn, "salu_branch_per_iteration": salu, "s_nop_per_iteration": nop,
                    "s_waitcnt_per_iteration": wait, "issue_slots_per_iteration": allins,
                    "dynamic_issue_slots": allins * it})
        print(f"{label:28s} {it:10.3e} {n:8d} " + " ".join(f"{m[c]:11d}" for c in CLASSES) + f" {n * it:10.3e}"
              f" {salu:8d} {nop:6d} {wait:8d} {allins:9d} {allins * it:10.3e}")
    # the walk step's memory instructions per iteration: a stack instance reads the node (two
    # ds_read_b128, or global loads) and the stack top and stores the far child; a link instance
    # (render_kernel LINK) reads the node and its u16 miss link and stores nothing
    mem = collections.Counter()
    for b in walk_main:
        for x in b["ins"]:
            op = x.split()[0]
            for k in ("ds_read", "ds_write", "global_load", "global_store", "scratch_"):
                if op.startswith(k):
                    mem[k.rstrip("_")] += 1
    print(f"{'walk step memory ops':26s} " + " ".join(f"{k} {v}" for k, v in sorted(mem.items())))
    out.append({"phase": "walk step memory ops", "per_iteration": dict(mem)})
    acc = sum(total.values())
    print(f"{'sum of the four':26s} {'':10s} {'':8s} " + " ".join(f"{total[c]:11.3e}" for c in CLASSES) + f" {acc:10.3e}")
    if pmc:
        insts = pmc["SQ_INSTS_VALU"]
        print(f"SQ_INSTS_VALU {insts:.3e}; the rest (shade, path start, traversal set-up, draws): {insts - acc:.3e}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
