"""The back end issues its row / DC loads by inline asm and waits for them by hand (back_end_pairs, jsnoop_kernels.hip): the compiler does not know that
those registers are in flight.  This check compiles the kernels to assembly and, for every k_idct_color<1..4> instance:

1. lists every instruction that READS a register a `global_load_*` of the MCU loop writes: only the masking `v_and_b32` (rows), the `v_add_u32` of the DC
   word and the loads themselves may appear; a `v_mov` / copy of such a register would read it before its data has landed;
2. walks back from every hand `s_waitcnt vmcnt(2*np)` -- around the loop's back edge and into the loop's entry -- to the load that writes the register
   the wait guards, and counts the VMEM instructions (global_load*, global_store*, global_atomic*, buffer_*, flat_*) issued in between on the path with
   the FEWEST of them (a branch on vcc / scc may go either way: the plane stores behind `want_planes` count for nothing).  vmcnt drains in issue order, so
   the wait covers the load only if that count is at least 2*np.  An `s_cbranch_execz` is taken as not taken (the lanes it tests are never all off: the
   DIB store's `p < total` holds for lanes 0..15 of any MCU); every counted store behind one is printed, so the reliance shows in the output.

usage: python tools/check_inflight_regs.py [file.s]   (CPU only, ~1 min; file.s: check that assembly instead of compiling the kernels)"""
import heapq, os, re, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_kernels.hip")
NP = {1: 3, 2: 2, 3: 2, 4: 2}                                   # pairs per MCU of k_idct_color<LAYOUT>: (EH * EV + 2 + 1) / 2 blocks
VMEM = re.compile(r"(global_load|global_store|global_atomic|buffer_|flat_)\w*$")
HAND_LOAD = re.compile(r"\s+global_load_(dword|sshort) (v\d+), v\d+, s\[")


def compile_asm(out):
    """hipcc -S of the kernels for gfx950, device side only, with the product's flags."""
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "--cuda-device-only", "-S",
                           "-I" + os.path.dirname(SRC), "-o", out, SRC], stderr=subprocess.DEVNULL)


def kernels(text):
    """(layout, lines of the function) for every k_idct_color<1..4>; <0>, the any-layout kernel, leaves loads and waits to the compiler."""
    for m in re.finditer(r"^(_Z12k_idct_colorILi([1-4])E\w+):\s*; @.*?^\.Lfunc_end", text, re.S | re.M):
        yield int(m.group(2)), m.group(0).split("\n")


def check_copies(body):
    loads = [l for l in body if re.match(r"\s+global_load_(dword|sshort) v\d+, v\d+, s\[", l)]
    regs = sorted({re.match(r"\s+global_load_\w+ (v\d+),", l).group(1) for l in loads[7:]} or {re.match(r"\s+global_load_\w+ (v\d+),", l).group(1) for l in loads})
    readers = {}
    for l in body:
        l2 = l.split(";")[0]
        mm = re.match(r"\s+(\w+)\s+(.*)", l2)
        if not mm or mm.group(1).startswith("global_load") or mm.group(1) == "s_waitcnt": continue
        ops = [o.strip() for o in mm.group(2).split(",")]
        for r in regs:
            if r in ops[1:]:
                readers.setdefault(r, set()).add(mm.group(1))
    ok = all(v <= {"v_and_b32_e32", "v_add_u32_e32"} for v in readers.values())
    return ok, regs, readers


def parse(body):
    """Instructions of a function as (opcode, operands, source line number), labels -> index of the instruction that follows them."""
    ins, labels = [], {}
    for n, l in enumerate(body):
        s = l.split(";")[0].strip()
        if not s:
            continue
        lm = re.match(r"^([.\w$]+):$", s)
        if lm:
            labels[lm.group(1)] = len(ins)
            continue
        if s.startswith("."):                                    # directives
            continue
        op, _, rest = s.partition(" ")
        ins.append((op, [o.strip() for o in re.split(r",\s*", rest) if o.strip()] if rest else [], n))
    return ins, labels


def predecessors(ins, labels):
    """Control-flow predecessors of every instruction, without the taken edge of an s_cbranch_execz (see the module docstring)."""
    pred = [[] for _ in ins]
    for i, (op, args, _) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            t = labels.get(args[0])
            if t is not None and t < len(ins) and op != "s_cbranch_execz":
                pred[t].append(i)
        if op not in ("s_branch", "s_endpgm", "s_setpc_b64") and i + 1 < len(ins):
            pred[i + 1].append(i)
    return pred


def refetch_of(ins, pred, i):
    """The loop's entry issues its last DC load twice -- the second one in the DIB store's place, so that the first wait of the loop finds 2*np
    operations behind its load: when load i is such a repeat (the VMEM instruction straight before it loads the same register from the same base and
    offset), its value has landed with the first one, which is the load a wait must cover.  Returns that first load's index, or None."""
    op, args, _ = ins[i]
    j = i
    while pred[j] == [j - 1]:
        j -= 1
        if VMEM.match(ins[j][0]):
            oj, aj, _ = ins[j]
            return j if oj == op and aj[0] == args[0] and aj[2:] == args[2:] else None
    return None


def check_waits(layout, body):
    """Returns (ok, report lines) for the hand vmcnt(2*np) waits of one k_idct_color instance."""
    np_ = NP[layout]
    want = 2 * np_
    ins, labels = parse(body)
    pred = predecessors(ins, labels)
    raw_lines = body
    # the hand loads: global_load_dword / _sshort with an SGPR base between ;;#ASMSTART and ;;#ASMEND
    asm_idx, inside = set(), False
    for n, l in enumerate(raw_lines):
        if ";;#ASMSTART" in l: inside = True
        elif ";;#ASMEND" in l: inside = False
        if inside:
            asm_idx.add(n)
    hand_dst = {ins[i][1][0] for i in range(len(ins)) if ins[i][2] in asm_idx and HAND_LOAD.match(raw_lines[ins[i][2]])}
    waits = [i for i, (op, args, n) in enumerate(ins) if op == "s_waitcnt" and n in asm_idx and args == ["vmcnt(%d)" % want]]
    out, ok = [], True
    if len(waits) != 2 * np_:
        return False, ["  expected %d hand waits vmcnt(%d), found %d" % (2 * np_, want, len(waits))]
    for w in waits:
        g = None
        for j in range(w + 1, len(ins)):                         # the register this wait guards: the first one of the hand loads read after it
            op, args, _ = ins[j]
            if op.startswith("global_load") or op == "s_waitcnt":
                continue
            hit = [a for a in args[1:] if a in hand_dst]
            if hit:
                g = hit[0]
                break
        if g is None:
            return False, ["  line %d: no register read behind the wait" % (ins[w][2] + 1)]
        # 0/1-weight shortest paths backwards: VMEM instructions strictly between a load of g and the wait, fewest first.  Every load of g the walk
        # reaches is reported (the one of the previous iteration, round the back edge, and the one of the loop's entry); the walk ends at each.
        found, dist = {}, {}
        heap = [(0, p, (p,)) for p in pred[w]]
        while heap:
            d, i, path = heapq.heappop(heap)
            if i in dist:
                continue
            dist[i] = d
            op, args, _ = ins[i]
            if op.startswith("global_load") and args and args[0] == g and refetch_of(ins, pred, i) is None:
                found[i] = (d, path)
                continue
            nd = d + (1 if VMEM.match(op) else 0)
            for p in pred[i]:
                if p not in dist:
                    heapq.heappush(heap, (nd, p, path + (p,)))
        if not found:
            out.append("  line %d: vmcnt(%d) guards %s: no load of it reaches the wait" % (ins[w][2] + 1, want, g))
            ok = False
            continue
        for ld, (d, path) in sorted(found.items(), key=lambda kv: -kv[0]):
            counted = [i for i in path[:-1] if VMEM.match(ins[i][0])]
            good = d >= want
            ok = ok and good
            out.append("  line %d: vmcnt(%d) guards %s, loaded at line %d: %d VMEM instructions between -> %s" %
                       (ins[w][2] + 1, want, g, ins[ld][2] + 1, d, "covered" if good else "SHORT"))
            skipping = {}                                        # execz branches passed on the path (forward) whose target is not reached yet
            for i in reversed(path):
                for j in [j for j, t in skipping.items() if t == i]:
                    del skipping[j]
                if i in counted and ins[i][0].startswith("global_load") and ins[i][1][0] == g:
                    out.append("    the load at line %d repeats the one at line %d (the loop's entry, in the DIB store's place)" % (ins[i][2] + 1, ins[refetch_of(ins, pred, i)][2] + 1))
                if i in counted and ins[i][0].startswith("global_store") and skipping:
                    out.append("    counted store at line %d (%s) sits behind the s_cbranch_execz at line %d" % (ins[i][2] + 1, ins[i][0], ins[max(skipping)][2] + 1))
                if ins[i][0] == "s_cbranch_execz" and ins[i][1][0] in labels:
                    skipping[i] = labels[ins[i][1][0]]
    return ok, out


def main(argv):
    if len(argv) > 1:
        text = open(argv[1]).read()
    else:
        d = tempfile.mkdtemp(prefix="jsnoop_regs_")                 # a private directory: no clash with another user's run
        try:
            out = os.path.join(d, "jsnoop_kernels_check.s")
            compile_asm(out)
            text = open(out).read()
        finally:
            shutil.rmtree(d, ignore_errors=True)
    bad = 0
    seen = 0
    for layout, body in kernels(text):
        seen += 1
        ok, regs, readers = check_copies(body)
        print("k_idct_color<%d>: in-flight registers %s; read by %s -> %s" % (layout, regs, {k: sorted(v) for k, v in readers.items()}, "ok" if ok else "CHECK"))
        wok, lines = check_waits(layout, body)
        print("k_idct_color<%d>: hand waits vmcnt(%d): %s" % (layout, 2 * NP[layout], "all covered" if wok else "NOT COVERED"))
        print("\n".join(lines))
        bad += (0 if ok else 1) + (0 if wok else 1)
    if seen != 4:
        print("expected the four one-layout instances k_idct_color<1..4>, found %d" % seen)
        bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
