"""Static instruction counts of the persistent rollout kernel's substep loop (compile only, no GPU):
    python tools/loop_copies.py [--targs "1, 8, 4, 32"] [--flags "-DNAME=VALUE ..."] [--keep DIR] [--json]
Builds a translation unit that instantiates ONE so100_rollout_fused<targs> with the product's HIPFLAGS (read from csrc/Makefile) plus
-S --cuda-device-only, splits the kernel's ISA into basic blocks and reports, per region and per block, how many instructions are
VALU / packed VALU / copies (v_mov*, v_accvgpr_*, v_readlane / v_writelane) / LDS / SALU / s_nop / waits, and beside them two
kinds of issue slot that compute nothing (counted inside the categories above, not in addition to them): `lit`, an s_mov_b32 / s_mov_b64
of a literal (a constant re-materialised for a packed instruction, which takes no literal operand), and `zero`, fp32 VALU arithmetic
(mul / add / sub / fma / fmac ..., packed or not) with a literal +0 / -0 source (a product or sum the compiler may not fold without
fast-math):
  * the substep loop between its barriers: the loop is the shortest cycle of workgroup barriers in the kernel's control-flow graph
    (two per substep, three with pad contacts); region "b1->b2" is the first half of a substep (RNEA || CRBA + factor), "b2->b1" the
    second half, the back edge and the sin/cos update of the next substep;
  * the back-edge block: where the loop's backward branch lands, up to that block's end;
  * the step tail: from the loop's exit to the barrier that ends the env step (poses, obs, reset), per block; a block that is the
    fall-through of s_cbranch_execz (the reset of finished episodes) is marked: a wave skips it unless one of its lanes takes the branch.
Wave 0's path through a substep is every block of the loop but the RNEA block (the big block of the first half without a reciprocal)
and the first substep's exact sin/cos block (the one with v_floor); wave 1's leg is the RNEA block.
  * the pre-step region, in the variants that run substep 0's first half beside the sampling (physics_phase_mw: PRE; recognised by a loop
    without an exact sin/cos block): from the last barrier in front of it to substep 0's one barrier, per block; the two blocks with
    v_floor are wave 1's (sin/cos + RNEA) and wave 2's (sin/cos + CRBA + factor: the one with a reciprocal), the rest is wave 0's
    sampling, rollout row and env_step_pre.  That last barrier is the one behind the VALU heads in the 64-row kernels and layer 2's in the
    32-row kernels, whose heads (the two blocks with v_mfma_f32_4x4x1) run inside the region, on waves 0 and 3.
The same kind of tool as tools/rnea_count.sh."""
import argparse, json, os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so100_mujoco_rl_amd", "csrc")
CATS = ("valu", "pk", "copy", "lds", "salu", "nop", "wait", "other")
SUBS = ("lit", "zero")                                        # subsets of salu / of valu + pk
ARITH = re.compile(r"v_(pk_)?(mul|add|sub|subrev|fma|fmac|fmaak|fmamk|mad|mac)_f32")
NUMBER = re.compile(r"-?(0x[0-9a-fA-F]+|\d+(\.\d*)?(e[-+]?\d+)?)$")
ZEROS = ("0", "-0", "0.0", "-0.0", "0x0", "0x80000000")
SIG = ("so100::SimParams, float*, const float*, float*, float*, uint8_t*, uint8_t*, float*, float*, int32_t*, "
       "so100::PolicyWeights, so100::RolloutArgs")


def hipflags():
    """the product's compiler and flags, as csrc/Makefile expands them"""
    out = subprocess.check_output(["make", "-s", "-C", CSRC, "--eval=__flags: ; @echo $(HIPCC) $(HIPFLAGS)", "__flags"], text=True)
    words = out.split()
    return words[0], words[1:]


def compile_isa(targs, extra, keep=None):
    hipcc, flags = hipflags()
    d = keep or tempfile.mkdtemp(prefix="loop_copies_")
    os.makedirs(d, exist_ok=True)
    src, asm = os.path.join(d, "one.hip"), os.path.join(d, "one.s")
    with open(src, "w") as f:
        f.write('#include "so100_kernels.hpp"\n')
        f.write(f"template __global__ void so100::so100_rollout_fused<{targs}>({SIG});\n")
    cmd = [hipcc] + flags + extra + ["-S", "--cuda-device-only", "-I", CSRC, "-o", asm, src]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(r.returncode)
    usage = {}
    for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]"):
        m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", r.stderr)
        if m: usage[key] = int(m.group(1))
    txt = open(asm).read()
    if not keep: shutil.rmtree(d, ignore_errors=True)
    return txt, usage


def classify(op):
    if op.startswith(("v_mov", "v_accvgpr_", "v_readlane", "v_writelane")): return "copy"
    if op.startswith("v_pk_"): return "pk"
    if op.startswith("v_"): return "valu"
    if op.startswith("ds_"): return "lds"
    if op == "s_nop": return "nop"
    if op.startswith("s_waitcnt"): return "wait"
    if op == "s_barrier": return "other"
    if op.startswith("s_"): return "salu"
    return "other"


def operands(ins):
    """the operands of one instruction line, destination first, without trailing modifiers (op_sel:[..], neg_lo:[..], clamp, ...)"""
    rest = ins.split(None, 1)[1] if " " in ins or "\t" in ins else ""
    rest = re.sub(r"\s+\w+:\[[^\]]*\]", "", rest)
    return [o.strip() for o in rest.split(",")]


def is_lit(ins):
    op = ins.split()[0]
    return op in ("s_mov_b32", "s_mov_b64") and bool(NUMBER.match(operands(ins)[-1].split()[0]))


def is_zero(ins):
    return bool(ARITH.match(ins.split()[0])) and any(o.split()[0] in ZEROS for o in operands(ins)[1:] if o)


class Block:
    def __init__(self, name):
        self.name, self.ins, self.succ, self.barrier = name, [], [], False
    def counts(self):
        c = dict.fromkeys(CATS, 0)
        for i in self.ins: c[classify(i.split()[0])] += 1
        c["total"] = len(self.ins)
        c["accw"] = sum(i.startswith("v_accvgpr_write") for i in self.ins)
        c["lit"] = sum(is_lit(i) for i in self.ins)
        c["zero"] = sum(is_zero(i) for i in self.ins)
        return c


def parse_blocks(txt):
    """Basic blocks of the (only) kernel, in layout order.  A block ends at a label, behind a branch and behind s_barrier, so that a
    barrier is always the last instruction of its node."""
    body = txt[txt.index("so100_rollout_fused"):]
    body = body[body.index(":\n") + 2:]
    blocks, cur, fresh = [], Block("entry"), 0
    blocks.append(cur)
    def start(name):
        nonlocal cur
        nb = Block(name)
        if cur.fall: cur.succ.append(name)
        blocks.append(nb); cur = nb; cur.fall = True
    cur.fall = True
    for line in body.split("\n"):
        s = line.strip()
        if s.startswith(".Lfunc_end") or s.startswith(".section"): break
        m = re.match(r"(\.LBB\d+_\d+):", s)
        if m: start(m.group(1)); continue
        if not line.startswith("\t") or s.startswith((".", ";")): continue
        s = s.split(";")[0].strip()
        op = s.split()[0]
        if not cur.fall:                       # code behind an unconditional branch without a label of its own
            fresh += 1; start(f"anon{fresh}")
        cur.ins.append(s)
        if op == "s_branch":
            cur.succ.append(s.split()[1]); cur.fall = False
        elif op.startswith("s_cbranch"):
            cur.succ.append(s.split()[1])
            fresh += 1; start(f"{cur.name}+{fresh}")
        elif op == "s_endpgm":
            cur.fall = False
        elif op == "s_barrier":
            cur.barrier = True
            fresh += 1; start(f"{cur.name}+{fresh}")
    return blocks


def analyse(txt):
    blocks = parse_blocks(txt)
    by = {b.name: b for b in blocks}
    order = {b.name: i for i, b in enumerate(blocks)}
    pred = {b.name: [] for b in blocks}
    for b in blocks:
        b.succ = [s for s in b.succ if s in by]
        for s in b.succ: pred[s].append(b.name)
    bars = [b.name for b in blocks if b.barrier]

    def reach(src, nxt, through_src=False):
        """nodes reachable from the successors of src without leaving a barrier node (barrier nodes are included, not crossed)"""
        seen, todo = set(), list(nxt[src])
        while todo:
            n = todo.pop()
            if n in seen: continue
            seen.add(n)
            if not stop(n): todo.extend(nxt[n])
        return seen
    succ = {b.name: b.succ for b in blocks}
    stop = lambda n: by[n].barrier
    fwd = {b: reach(b, succ) for b in bars}                 # from behind barrier b up to and including the next barrier nodes
    def back(b):                                            # nodes from which barrier node b is reached without crossing another barrier
        seen, todo = {b}, list(pred[b])
        while todo:
            n = todo.pop()
            if n in seen or by[n].barrier: continue
            seen.add(n); todo.extend(pred[n])
        return seen
    bwd = {b: back(b) for b in bars}
    region = lambda a, b: sorted(fwd[a] & bwd[b], key=order.get)
    bnext = {a: [b for b in bars if b in fwd[a]] for a in bars}
    # the substep loop: the shortest cycle (length >= 2) in the graph of barriers
    best = None
    for a in bars:
        paths = [[a]]
        for _ in range(3):
            new = []
            for p in paths:
                for n in bnext[p[-1]]:
                    if n == a and len(p) >= 2:
                        if best is None or len(p) < len(best): best = p
                    elif n not in p: new.append(p + [n])
            paths = new
    if best is None: raise SystemExit("no barrier cycle found: not the persistent rollout kernel?")
    best = sorted(best, key=order.get)
    halves = [(best[i], best[(i + 1) % len(best)]) for i in range(len(best))]
    loop = set()
    regions = {}
    for i, (a, b) in enumerate(halves):
        r = region(a, b)
        regions[f"b{i + 1}->b{(i + 1) % len(best) + 1}"] = r
        loop.update(r)
    # back-edge block: where a backward branch between two blocks of the loop lands
    landing = None
    for n in sorted(loop, key=order.get, reverse=True):
        for s in by[n].succ:
            if s in loop and order[s] < order[n] and (landing is None or order[s] < order[landing]): landing = s
    # step tail: behind the loop's last barrier, outside the loop, up to the next barrier
    last = best[-1]
    tail = sorted((fwd[last] - loop), key=order.get)
    # roles
    first = regions["b1->b2"]
    big = [n for n in first if "v_rcp_f32_e32" not in " ".join(by[n].ins)]
    rnea = max(big, key=lambda n: len(by[n].ins)) if big else None
    exact = [n for n in loop if any(i.startswith("v_floor_f32") for i in by[n].ins)]
    # pre-step region (PRE variants: no exact sin/cos inside the loop): between the two barriers in front of the loop's first one
    pre, pre_roles = [], {}
    if not exact:
        entry = [b for b in bars if b not in best and best[0] in fwd[b]]
        heads = [b for e in entry for b in bars if b not in best and b != e and e in fwd[b]]
        if entry and heads:
            pre = region(heads[0], entry[0])
            for n in pre:
                txt_ = " ".join(by[n].ins)
                if "v_floor_f32" in txt_: pre_roles[n] = "wave 2: sin/cos + CRBA + factor" if "v_rcp_f32" in txt_ else "wave 1: sin/cos + RNEA"
                elif "v_mfma_f32_4x4x1" in txt_: pre_roles[n] = "a head on the matrix cores: wave 0 the means, wave 3 the value"
    # blocks a wave skips when none of its lanes takes the branch: the fall-through of a block that ends in s_cbranch_execz
    guarded = {n for n in by for q in pred[n] if by[q].ins and by[q].ins[-1].startswith("s_cbranch_execz") and by[q].ins[-1].split()[1] != n}
    return dict(by=by, order=order, regions=regions, loop=loop, landing=landing, tail=tail, rnea=rnea, exact=exact, barriers=best, guarded=guarded, pre=pre, pre_roles=pre_roles)


def total(by, names):
    c = dict.fromkeys(CATS + SUBS + ("total", "accw"), 0)
    for n in names:
        for k, v in by[n].counts().items(): c[k] += v
    return c


def summary(txt, usage=None):
    a = analyse(txt)
    by = a["by"]
    out = {"usage": usage or {}, "regions": {}, "blocks": {}}
    for name, r in a["regions"].items():
        out["regions"][name] = total(by, r)
        out["blocks"][name] = [(n, by[n].counts()) for n in r if by[n].ins]
    out["loop"] = total(by, a["loop"])
    out["back_edge_block"] = {"name": a["landing"], "holds_barrier": bool(a["landing"] and by[a["landing"]].barrier),
                              **(by[a["landing"]].counts() if a["landing"] else total(by, []))}
    out["tail"] = total(by, a["tail"])
    out["blocks"]["tail"] = [(n, by[n].counts()) for n in a["tail"] if by[n].ins]
    out["pre"] = total(by, a["pre"])
    out["blocks"]["pre"] = [(n, by[n].counts()) for n in a["pre"] if by[n].ins]
    out["pre_roles"] = a["pre_roles"]
    out["pre_wave0"] = total(by, [n for n in a["pre"] if n not in a["pre_roles"]])
    out["guarded"] = sorted(a["guarded"], key=a["order"].get)
    out["tail_unguarded"] = total(by, [n for n in a["tail"] if n not in a["guarded"]])
    out["rnea_block"] = {"name": a["rnea"], **(by[a["rnea"]].counts() if a["rnea"] else total(by, []))}
    w0 = [n for n in a["loop"] if n != a["rnea"] and n not in a["exact"]]
    out["wave0_path"] = total(by, w0)
    return out


def fmt(c):
    return "  ".join(f"{k} {c[k]:4d}" for k in ("total",) + CATS + SUBS)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--targs", default="1, 8, 4, 32", help="template arguments of so100_rollout_fused (KIND, FL, NW, ROWS)")
    ap.add_argument("--flags", default="", help="further compiler arguments")
    ap.add_argument("--keep", default=None, help="directory to keep one.hip / one.s in")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    txt, usage = compile_isa(args.targs, args.flags.split(), args.keep)
    s = summary(txt, usage)
    if args.json:
        print(json.dumps(s)); return
    print(f"so100_rollout_fused<{args.targs}> {args.flags}".rstrip())
    print("  " + "  ".join(f"{k}: {v}" for k, v in usage.items()))
    for name, c in s["regions"].items():
        print(f"region {name:8s} {fmt(c)}")
        for n, bc in s["blocks"][name]:
            tag = " (RNEA, wave 1)" if n == s["rnea_block"]["name"] else " (back edge lands here)" if n == s["back_edge_block"]["name"] else ""
            print(f"    {n:22s} {fmt(bc)}{tag}")
    print(f"loop, all blocks   {fmt(s['loop'])}")
    print(f"wave 0's path      {fmt(s['wave0_path'])}")
    print(f"wave 1's RNEA block {fmt(s['rnea_block'])}")
    be = s["back_edge_block"]
    print(f"back-edge block {be['name']}{' (holds barrier 1: no block of its own)' if be['holds_barrier'] else ''}  {fmt(be)}  v_accvgpr_write {be['accw']}")
    if s["blocks"]["pre"]:
        print(f"pre-step region    {fmt(s['pre'])}")
        for n, bc in s["blocks"]["pre"]:
            if bc["total"] >= 8 or n in s["pre_roles"]: print(f"    {n:22s} {fmt(bc)}{' (' + s['pre_roles'][n] + ')' if n in s['pre_roles'] else ''}")
        print(f"pre-step region without the blocks of waves 1 and 2 and the matrix-core heads (wave 0: sample, row, env_step_pre; wave 3: the row's observation columns)  {fmt(s['pre_wave0'])}")
    print(f"step tail          {fmt(s['tail'])}")
    for n, bc in s["blocks"]["tail"]:
        if bc["total"] >= 8:
            print(f"    {n:22s} {fmt(bc)}{' (skipped unless a lane takes the branch: s_cbranch_execz)' if n in s['guarded'] else ''}")
    print(f"step tail without the blocks behind s_cbranch_execz  {fmt(s['tail_unguarded'])}")


if __name__ == "__main__":
    main()
