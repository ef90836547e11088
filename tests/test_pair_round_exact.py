"""CPU: the exact form of the back end's term rounds (PAIR_EXACT_ASM in jpegsnoop_amd/csrc/jsnoop_pair_round.h, gen_exact in tools/gen/gen_pair_round.py).

One text runs all rounds of a pair and never reads past the end of the lists: a round entered with nl terms left issues exactly min(nl, 16) table reads and
ceil(min(nl, 16) / 2) coefficient pairs.  A read that is skipped changes every later `s_waitcnt lgkmcnt(N)` of its path, so the text has a path per way out
(twelve tails, three short lists) -- here EVERY list length 1..64 is replayed, branches followed, against an in-order LDS queue with symbolic values in the
registers:

* no instruction reads or overwrites a register with a read in flight, and nothing is in flight when the text is left;
* per round, the reads issued are exactly the invariant's; table read s takes row word s (row_newbcast:s) of the round's row words, coefficient pair j comes
  from list offset round * 64 + 8 j;
* acc0 / acc1 come out as ((0 + c0 t0) + c1 t1) + ... over terms 0..n-1, in this order, and nothing else;
* every line of the text is on the path of some length.

And the check itself is checked: a wait count off by one (every wait, one at a time), a tail that multiplies the wrong ring register, one read too many each
make it fail."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_pair_round.h")
LENGTHS = list(range(1, 65))


def exact_text():
    txt = open(HDR).read()
    m = re.search(r"#define PAIR_EXACT_ASM \\\n((?:    \".*\n)+)", txt)
    assert m, "PAIR_EXACT_ASM not in the header"
    return [re.match(r'\s*"(.*?)\\n\\t"', l).group(1) for l in m.group(1).strip().split("\n")]


def regs_of(tok):
    m = re.match(r"v\[(\d+):(\d+)\]$", tok)
    if m:
        return ["v%d" % i for i in range(int(m.group(1)), int(m.group(2)) + 1)]
    return [tok] if re.match(r"v\d+$", tok) or tok in ("%[rw]", "%[ad]", "%[ah]", "%[arw]", "%[l8]", "%[acc0]", "%[acc1]") else []


def parse(lines):
    prog, labels = [], {}
    for l in lines:
        m = re.match(r"(\.L\w+)%=:$", l)
        if m:
            labels[m.group(1)] = len(prog)
            continue
        op, _, rest = l.partition(" ")
        mods = dict(re.findall(r"(row_newbcast|offset):(\d+)", rest))
        args = [a.strip() for a in re.split(r" row_newbcast| offset", rest)[0].split(",") if a.strip()]
        prog.append((op, args, {k: int(v) for k, v in mods.items()}, l))
    return prog, labels


class Bad(AssertionError):
    pass


def expected(n, which):
    acc = 0
    for k in range(n):
        acc = ("add", acc, ("mul", ("c", k), (which, k)))
    return acc


def replay(prog, labels, n):
    """Runs the text for a pair whose longer list has n terms.  Returns the set of program indices executed."""
    reg = {"%[acc0]": 0, "%[acc1]": 0, "%[ah]": ("ah", 0), "%[arw]": ("arw", 0), "%[l8]": "l8"}
    nl, ro, scc = n, 0, False
    inflight = []                                                 # (destination registers, values), issue order
    rounds = {}                                                   # round -> {"T": [s ...], "C": [j ...], "RW": count}
    seen, pc, budget = set(), 0, 5000

    def free(r, l, what):
        if any(r in d for d, _ in inflight):
            raise Bad("%s: %s %s while an LDS read to it is in flight" % (l, what, r))

    def get(r, l):
        free(r, l, "reads")
        if r not in reg:
            raise Bad("%s: reads %s, which holds nothing" % (l, r))
        return reg[r]

    while pc < len(prog):
        budget -= 1
        assert budget, "the text does not end"
        op, a, mod, l = prog[pc]
        seen.add(pc)
        pc += 1
        if op == "s_waitcnt":
            cnt = int(re.search(r"lgkmcnt\((\d+)\)", l).group(1))
            if cnt > 15:
                raise Bad(l + ": lgkmcnt has four bits")
            while len(inflight) > cnt:
                dst, val = inflight.pop(0)
                reg.update(zip(dst, val))
        elif op == "ds_read_b32":                                 # the round's row words: %[arw] itself (round 0) or %[ad] = %[arw] + ro
            addr = get(a[1], l)
            if not (isinstance(addr, tuple) and addr[0] == "arw" and addr[1] % 64 == 0 and "offset" not in mod):
                raise Bad(l + ": row words read at %r" % (addr,))
            free(a[0], l, "overwrites")
            r = addr[1] // 64
            rounds.setdefault(r, {"T": [], "C": [], "RW": 0})["RW"] += 1
            inflight.append(([a[0]], [("rw", r)]))
        elif op == "ds_read_b64":
            dst = regs_of(a[0])
            for d in dst:
                free(d, l, "overwrites")
            addr = get(a[1], l)
            if isinstance(addr, tuple) and addr[0] == "ah":      # coefficient pair: list offset from the half's base
                off = addr[1] + mod.get("offset", 0)
                r, j = off // 64, (off % 64) // 8
                if off % 8 or r not in rounds:
                    raise Bad(l + ": coefficient pair at list offset %d" % off)
                rounds[r]["C"].append(j)
                inflight.append((dst, [("c", 16 * r + 2 * j), ("c", 16 * r + 2 * j + 1)]))
            elif isinstance(addr, tuple) and addr[0] == "row":    # table pair of a term
                rounds[addr[1] // 16]["T"].append(addr[1] % 16)
                inflight.append((dst, [("t0", addr[1]), ("t1", addr[1])]))
            else:
                raise Bad(l + ": reads at %r" % (addr,))
        elif op == "v_add_u32_dpp":                               # row word of term s of the round, broadcast, + the lane's column offset
            rw = get(a[1], l)
            if not (isinstance(rw, tuple) and rw[0] == "rw" and get(a[2], l) == "l8" and 0 <= mod["row_newbcast"] < 16):
                raise Bad(l + ": address from %r" % (rw,))
            free(a[0], l, "overwrites")
            reg[a[0]] = ("row", 16 * rw[1] + mod["row_newbcast"])
        elif op == "v_add_u32":                                   # the next round's addresses
            free(a[0], l, "overwrites")
            if a[0] == "%[ah]" and a[2] == "%[ah]":
                base = get("%[ah]", l)
                reg["%[ah]"] = ("ah", base[1] + int(a[1]))
            elif a[0] == "%[ad]" and a[1] == "%[ro]" and a[2] == "%[arw]":
                reg["%[ad]"] = ("arw", get("%[arw]", l)[1] + ro)
            else:
                raise Bad("unexpected " + l)
        elif op in ("v_mul_f32", "v_add_f32"):
            x, y = get(a[1], l), get(a[2], l)
            free(a[0], l, "overwrites")
            reg[a[0]] = ("mul" if op == "v_mul_f32" else "add", x, y)
        elif op in ("s_cmp_le_u32", "s_cmp_lt_u32"):
            assert a[0] == "%[nl]"
            scc = nl <= int(a[1]) if op == "s_cmp_le_u32" else nl < int(a[1])
        elif op == "s_sub_u32":
            assert a[0] == a[1] == "%[nl]" and nl > int(a[2])
            nl -= int(a[2])
        elif op == "s_add_u32":
            assert a[0] == a[1] == "%[ro]"
            ro += int(a[2])
        elif op == "s_cbranch_scc1":
            if scc:
                pc = labels[a[0].replace("%=", "")]
        elif op == "s_branch":
            pc = labels[a[0].replace("%=", "")]
        else:
            raise AssertionError("unexpected line " + l)
    if inflight:
        raise Bad("left with %d LDS reads in flight" % len(inflight))
    # the reads issued are exactly the invariant's
    nr = (n + 15) // 16
    if sorted(rounds) != list(range(nr)):
        raise Bad("rounds run: %r" % sorted(rounds))
    for r in range(nr):
        m = min(n - 16 * r, 16)
        got = rounds[r]
        if got["T"] != list(range(m)) or got["C"] != list(range((m + 1) // 2)) or got["RW"] != 1:
            raise Bad("n = %d, round %d: %d terms, reads issued %r" % (n, r, m, got))
    for name, which in (("%[acc0]", "t0"), ("%[acc1]", "t1")):
        if reg[name] != expected(n, which):
            raise Bad("n = %d: %s is not the sum of terms 0..%d in order" % (n, name, n - 1))
    return seen


@pytest.fixture(scope="module")
def text():
    prog, labels = parse(exact_text())
    cover = {}                                                    # program index -> a list length whose path runs it
    for n in LENGTHS:
        for i in replay(prog, labels, n):
            cover.setdefault(i, n)
    return prog, labels, cover


def test_every_list_length_reads_exactly_its_terms_and_sums_them_in_order(text):
    prog, labels, cover = text
    assert sorted(cover) == list(range(len(prog))), [prog[i][3] for i in range(len(prog)) if i not in cover]
    # what the text is made of: twelve tails, three short lists, one loop
    assert sorted(labels) == sorted([".Lxr", ".Lxs", ".Lxs1", ".Lxs2", ".Lxe"] + [".Lxt%d" % s for s in range(12)])
    assert labels[".Lxe"] == len(prog)


def fails(prog, labels, lengths):
    for n in lengths:
        try:
            replay(prog, labels, n)
        except Bad:
            return True
    return False


def test_a_wait_count_off_by_one_fails(text):
    prog, labels, cover = text
    waits = [i for i, p in enumerate(prog) if p[0] == "s_waitcnt"]
    assert len(waits) == (1 + 16) + 12 * 4 + (4 + 3 + 2)         # the main path, the tails, the short lists: one wait per step and one for the row words
    for i in waits:
        op, a, mod, l = prog[i]
        cnt = int(re.search(r"\((\d+)\)", l).group(1))
        mutated = list(prog)
        mutated[i] = (op, a, mod, "s_waitcnt lgkmcnt(%d)" % (cnt + 1))
        assert fails(mutated, labels, [cover[i]]), "line %d (%s) may wait for one read less" % (i, l)


def test_a_tail_that_consumes_the_wrong_ring_register_fails(text):
    prog, labels, cover = text
    first_tail = labels[".Lxt0"]
    muls = [i for i, p in enumerate(prog) if p[0] == "v_mul_f32" and i >= first_tail]
    assert len(muls) == 2 * (12 * 4 + 3 + 2 + 1)
    for i in muls:
        op, a, mod, l = prog[i]
        t = int(a[0][1:])
        other = "v%d" % (54 + (t - 54 + 2) % 10)                  # the next table pair of the ring
        mutated = list(prog)
        mutated[i] = (op, [other, a[1], other], mod, l + " (mutated)")
        assert fails(mutated, labels, [cover[i]]), l
        c = int(a[1][1:])
        mutated[i] = (op, [a[0], "v%d" % (c ^ 1 if c < 52 else c - 4), a[2]], mod, l + " (mutated)")     # the pair's other word / another pair
        assert fails(mutated, labels, [cover[i]]), l


def test_one_read_too_many_fails(text):
    prog, labels, cover = text
    for name in [".Lxt%d" % s for s in range(12)] + [".Lxs", ".Lxs1", ".Lxs2"]:
        at = labels[name]
        while prog[at][0] != "v_mul_f32":
            at += 1
        n = cover[at]
        nl = (n - 1) % 16 + 1
        s = nl                                                    # the term behind the list's end
        if s < 16:
            extra = [("v_add_u32_dpp", ["%[ad]", "%[rw]", "%[l8]"], {"row_newbcast": s}, "extra table address"),
                     ("ds_read_b64", ["v[%d:%d]" % (54 + 2 * (s % 5), 55 + 2 * (s % 5)), "%[ad]"], {}, "extra table read")]
            mutated = prog[:at + 2] + extra + prog[at + 2:]
            lab = {k: v + (2 if v > at + 2 else 0) for k, v in labels.items()}
            assert fails(mutated, lab, [n]), name
        j = (nl + 1) // 2                                         # the coefficient pair behind the list's end
        if j < 8:
            extra = [("ds_read_b64", ["v[%d:%d]" % (48 + 2 * (j % 3), 49 + 2 * (j % 3)), "%[ah]"], {"offset": 8 * j}, "extra coefficient read")]
            mutated = prog[:at + 2] + extra + prog[at + 2:]
            lab = {k: v + (1 if v > at + 2 else 0) for k, v in labels.items()}
            assert fails(mutated, lab, [n]), name


def test_the_kernel_runs_the_exact_form_only():
    src = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_kernels.hip")).read()
    assert src.count("PAIR_EXACT_ASM") >= 1 and not re.search(r"PAIR_ROUND_ASM_|PAIR_ROUND\(", src)
